"""The keypoint fit restated in numpy (include/ht_mi355x.h "keypoint fit"): the constraint rows of a keypoint table against 3-D points and pixels,
the residuals, and the step loop over the C restatement of the solver (oracle_lib).  Every function takes a dtype: np.float32 evaluates one rounding per operation in the
written order (what k_keypoint_rows must equal bit for bit), np.float64 is the yardstick.  Test infrastructure only; shares no code with the kernels.  The quaternion
algebra is tests/joints_ref.py's.

A model is anything with nb and com [nb,3] (joints_ref.Model).  A table is (bones [K], offsets [K,3], rel [K]).  States are the solver's: [B,nb,13] = centre-of-mass
position, quaternion xyzw, linear and angular momentum (ht_get_state).  A row is the 16 floats of ht_fit_rows."""
import ctypes as C

import numpy as np

import joints_ref as jr

FLT_MAX = float(np.finfo(np.float32).max)
KEEP_MOMENTA = 1
WRONG = ("rel", "origin", "limits")


def _v(a):
    return tuple(a[..., i] for i in range(3))


def _evaluate(model, state, table, kind, xyz, pix, weights, cams, dtype, wrong):
    """per keypoint k, over the frames: dict(bone, off [3], present [B], ray, X, and for a point t, dv; for a pixel pc, ax, ay, d0, d1)"""
    T = np.dtype(dtype).type
    two = T(2)
    state = np.asarray(state, dtype); B = state.shape[0]
    bones, off, rel = (np.asarray(a) for a in table)
    K = len(bones)
    kind = np.zeros(K, np.int32) if kind is None else np.asarray(kind, np.int32).reshape(K)
    out = []
    for k in range(K):
        b = int(bones[k])
        o = off[k].astype(dtype); com = np.asarray(model.com[b]).astype(dtype)
        if wrong == "rel":
            o = o + com if rel[k] == 0 else o      # converted the other way
        elif rel[k] == 0:
            o = o - com                            # the states are centre-of-mass poses
        q = tuple(state[:, b, 3 + i] for i in range(4))
        r = jr.qrot(q, tuple(np.full(B, o[i], dtype) for i in range(3)), two)
        X = tuple(state[:, b, i] + r[i] for i in range(3))
        w = np.ones(B, dtype) if weights is None else np.asarray(weights, dtype).reshape(B, K)[:, k]
        e = dict(bone=b, off=o, ray=bool(kind[k]), X=X, w=w)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if not kind[k]:
                t = _v(np.asarray(xyz, dtype).reshape(B, K, 3)[:, k])
                e["present"] = (w > 0) & np.isfinite(t[0]) & np.isfinite(t[1]) & np.isfinite(t[2])
                e["p0"] = t
                e["dv"] = tuple(X[i] - t[i] for i in range(3))
            else:
                uv = np.asarray(pix, dtype).reshape(B, K, 2)[:, k]; cam = np.asarray(cams, dtype).reshape(B, 12)
                e["present"] = (w > 0) & np.isfinite(uv[:, 0]) & np.isfinite(uv[:, 1])
                d = ((uv[:, 0] - cam[:, 2]) / cam[:, 0], (uv[:, 1] - cam[:, 3]) / cam[:, 1], np.ones(B, dtype))      # deprojectz(p, 1)
                ray = jr.normalize(jr.qrot(tuple(cam[:, 8 + i] for i in range(4)), d, two))
                qz = jr.quat_from_to_z(ray, T)
                pc = tuple(np.zeros(B, dtype) for i in range(3)) if wrong == "origin" else tuple(cam[:, 5 + i] for i in range(3))
                relv = tuple(X[i] - pc[i] for i in range(3))
                e["p0"] = pc; e["rayv"] = ray
                e["ax"], e["ay"] = jr.qxdir(qz, two), jr.qydir(qz, two)
                e["d0"], e["d1"] = jr.dot3(relv, e["ax"]), jr.dot3(relv, e["ay"])
        out.append(e)
    return out


def rays(pix, cams, dtype=np.float32):
    """the rays of pixels pix [B,K,2] in cams [B,12] -> [B,K,3]: normalize(qrot(qc, deprojectz(p, 1)))"""
    T = np.dtype(dtype).type
    pix = np.asarray(pix, dtype); B, K = pix.shape[:2]; cam = np.asarray(cams, dtype).reshape(B, 12)
    out = np.zeros((B, K, 3), dtype)
    for k in range(K):
        d = ((pix[:, k, 0] - cam[:, 2]) / cam[:, 0], (pix[:, k, 1] - cam[:, 3]) / cam[:, 1], np.ones(B, dtype))
        r = jr.normalize(jr.qrot(tuple(cam[:, 8 + i] for i in range(4)), d, T(2)))
        for i in range(3):
            out[:, k, i] = r[i]
    return out


def rows(model, state, table, kind=None, xyz=None, pix=None, weights=None, cams=None, max_force=FLT_MAX, ray_radius=0.01, ray_force=100000.0, dtype=np.float32, wrong=None):
    """-> the frames' rows, a list of [n_f,16] arrays: three rows a present point target (ConstrainPositionNailed, physics.h:342-346), four a present pixel target (a
    dead-zone pair on each axis across its ray, physics.h:337-338), absent keypoints compacted out, table order.  wrong: a deliberately WRONG variant, kept to show
    that the tests notice it -- "rel" converts the offsets the other way, "origin" starts the rays at the origin instead of the camera, "limits" swaps the limits
    of a pair."""
    T = np.dtype(dtype).type
    ev = _evaluate(model, state, table, kind, xyz, pix, weights, cams, dtype, wrong)
    B = np.asarray(state).shape[0]
    unit = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    blocks = []      # per keypoint its rows over the frames [B,n,16]
    with np.errstate(invalid="ignore", over="ignore"):
        for e in ev:
            if not e["ray"]:
                f = T(max_force) * e["w"]
                rws = [(unit[i], e["dv"][i], -f, f) for i in range(3)]
            else:
                fr = T(ray_force) * e["w"]; z = np.zeros(B, dtype)
                lo, hi = ((-fr, z), (z, fr)) if wrong == "limits" else ((z, fr), (-fr, z))
                rws = []
                for a, d in ((e["ax"], e["d0"]), (e["ay"], e["d1"])):
                    rws += [(a, d + T(ray_radius), lo[0], lo[1]), (a, d - T(ray_radius), hi[0], hi[1])]
            blk = np.zeros((B, len(rws), 16), dtype)
            blk[:, :, 0] = -1; blk[:, :, 1] = e["bone"]
            for i in range(3):
                blk[:, :, 2 + i] = e["p0"][i][:, None]; blk[:, :, 5 + i] = e["off"][i]
            for j, (n, td, fmin, fmax) in enumerate(rws):
                for i in range(3):
                    blk[:, j, 8 + i] = n[i]
                blk[:, j, 11] = td; blk[:, j, 13] = fmin; blk[:, j, 14] = fmax
            blocks.append(blk)
    return [np.concatenate([blk[f] for blk, e in zip(blocks, ev) if e["present"][f]] + [np.zeros((0, 16), dtype)]) for f in range(B)]


def residuals(model, state, table, kind=None, xyz=None, pix=None, weights=None, cams=None, dtype=np.float32, wrong=None):
    """[B,K]: a point's distance sqrt(dx dx + dy dy + dz dz) to its target, a pixel's distance sqrt(d d + d' d') to its ray, -1 for an absent keypoint"""
    ev = _evaluate(model, state, table, kind, xyz, pix, weights, cams, dtype, wrong)
    B = np.asarray(state).shape[0]
    out = np.zeros((B, len(ev)), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, e in enumerate(ev):
            if e["ray"]:
                r = np.sqrt(e["d0"] * e["d0"] + e["d1"] * e["d1"])
            else:
                dv = e["dv"]; r = np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
            out[:, k] = np.where(e["present"], r, -1)
    return out


def mean_residual(resid):
    """per frame, over the present keypoints (NaN for a frame without any)"""
    r = np.asarray(resid, np.float64); m = r >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m, r, 0).sum(axis=-1) / m.sum(axis=-1)


def user_poses(model, state, dtype=np.float32):
    """GetPoseUser of states [B,nb,13] -> [B,nb,7]: pos + qrot(q, -com)"""
    T = np.dtype(dtype).type
    state = np.asarray(state, dtype); B, nb = state.shape[:2]
    out = state[:, :, :7].copy()
    for b in range(nb):
        com = np.asarray(model.com[b]).astype(dtype)
        r = jr.qrot(tuple(state[:, b, 3 + i] for i in range(4)), tuple(np.full(B, -com[i], dtype) for i in range(3)), T(2))
        for i in range(3):
            out[:, b, i] = state[:, b, i] + r[i]
    return out


# ---- the loop over the C restatement of the solver ----------------------------------------------------------------------------------------------------
def linears(ol, rws):
    """rows [n,16] -> the restatement's ho_linear array"""
    L = (ol.Linear * max(1, len(rws)))()
    for i, r in enumerate(rws):
        L[i].rb0 = int(r[0]); L[i].rb1 = int(r[1]); L[i].position0 = ol.v3(r[2:5]); L[i].position1 = ol.v3(r[5:8]); L[i].normal = ol.v3(r[8:11])
        L[i].targetdist = float(r[11]); L[i].targetspeednobias = float(r[12]); L[i].forcelimit = ol.F2(float(r[13]), float(r[14])); L[i].friction_master = int(r[15])
    return L


def oracle_step(ol, orc, which, state, rws):
    """one step on one frame: state [nb,13] -> state after HandModelEnhancements (the joint ranges) and FitPointCloud({}, rows)"""
    orc.set_state(which, state)
    m = orc.model(which)
    A = (ol.Angular * 16)(); n = C.c_int(0); z = ol.F3(0, 0, 0)
    orc.L.ho_enhancements(orc.h, m, A, C.byref(n), 0, z, z, 0)
    assert n.value == 0
    orc.L.ho_fit_pointcloud(orc.h, m, None, 0, linears(ol, rws), len(rws), A, 0, 1.0)
    return orc.get_state(which)


def fit_loop(ol, orc, model, state, table, steps=6, flags=0, which=0, **kw):
    """ht_fit_keypoints on the restatement, frame by frame: states [B,nb,13] -> (the states before step 0 .. after the last step [steps + 1,B,nb,13], resid [B,2,K]).
    kw: rows' arguments (kind, xyz, pix, weights, cams, max_force, ray_radius, ray_force, wrong).  Without KEEP_MOMENTA the momenta are zeroed on entry and after every
    step (handtrack.h:686-687)."""
    cur = np.array(state, np.float32)
    if not flags & KEEP_MOMENTA:
        cur[:, :, 7:13] = 0
    rk = {k: v for k, v in kw.items() if k not in ("max_force", "ray_radius", "ray_force")}
    trace = [cur.copy()]
    first = residuals(model, cur, table, **rk)
    for _ in range(steps):
        rws = rows(model, cur, table, **kw)
        for f in range(len(cur)):
            cur[f] = oracle_step(ol, orc, which, cur[f], rws[f])
        if not flags & KEEP_MOMENTA:
            cur[:, :, 7:13] = 0
        trace.append(cur.copy())
    return np.stack(trace), np.stack([first, residuals(model, cur, table, **rk)], axis=1)
