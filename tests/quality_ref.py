"""Tracking accuracy restated in numpy (include/ht_mi355x.h "tracking accuracy"): keypoint tables, keypoints in 3-D and in pixels, visibility,
keypoint errors, depth comparison and the composite's pose conversion.  Every function takes a dtype: np.float32 evaluates one rounding per operation in the written
order (what the kernels must equal bit for bit), np.float64 is the yardstick.  Test infrastructure only; shares no code with the kernels.  qrot / qmul / qconj and the
centre-of-mass handling are tests/joints_ref.py's, the mirror is tests/mirror_ref.py's.

A model is anything with nb, nj, rb0, rb1 [nj], p1 [nj,3] and com [nb,3] (joints_ref.Model, or Chain below).  A table is (bones [K], offsets [K,3], rel [K])."""
import numpy as np

import joints_ref as jr

COM_POSES = 1
FEATURE8, SKELETON = 0, 1
VISIBLE, OCCLUDED, NOTHING, OUTSIDE, BEHIND = 0, 1, 2, 3, 4
IDENTITY_BITS = np.array([0, 0, 0, 0, 0, 0, 1], np.float32).view(np.uint32)


class Chain:
    """a hand-written model: bodies 0..nb-1, joints as (rb0, rb1, p1)"""

    def __init__(self, com, joints):
        self.com = np.array(com, np.float32).reshape(-1, 3); self.nb = len(self.com); self.nj = len(joints)
        self.rb0 = np.array([j[0] for j in joints], np.int32); self.rb1 = np.array([j[1] for j in joints], np.int32)
        self.p1 = np.array([j[2] for j in joints], np.float32).reshape(-1, 3)


# ---- item 1: the tables ------------------------------------------------------------------------------------------------------------------------
def feature8(scales=()):
    """handmodelfeaturepoints (handtrack.h:77-81), rel = 1; scales: the factors ht_scale was called with, applied in order as fp32 multiplications"""
    off = np.zeros((8, 3), np.float32); off[1] = (-0.03, 0, -0.03); off[2] = (0.03, 0, -0.03)
    for s in scales:
        off = off * np.float32(s)
    return np.array([1, 1, 1, 4, 7, 10, 13, 16], np.int32), off, np.ones(8, np.int32)


def skeleton(model):
    """body 0's user origin; per joint in model order its child-side anchor (rbi1, p1); per leaf body (no joint's rbi0) in body order (b, com[b]); all rel = 0"""
    bones, off = [0], [np.zeros(3, np.float32)]
    for j in range(model.nj):
        bones.append(int(model.rb1[j])); off.append(np.asarray(model.p1[j], np.float32))
    parents = set(int(b) for b in model.rb0)
    for b in range(model.nb):
        if b not in parents:
            bones.append(b); off.append(np.asarray(model.com[b], np.float32))
    return np.array(bones, np.int32), np.array(off, np.float32).reshape(-1, 3), np.zeros(len(bones), np.int32)


def builtin(model, which, scales=()):
    return feature8(scales) if which == FEATURE8 else skeleton(model)


# ---- items 2-4: keypoints -------------------------------------------------------------------------------------------------------------------------
def keypoints(model, poses, table, dtype=np.float32, com_poses=False, hands=None, cams=None, depth=None, near_tol=0.0, far_tol=0.0, wrong=None):
    """poses [B,nb,7] -> dict(xyz [B,K,3]; with cams [B,12]: pix [B,K,2], zc [B,K]; with depth u16[B,h,w]: vis u8[B,K] and the sampled pixel ixy i64[B,K,2], -1 where
    none is sampled).  wrong: a deliberately WRONG variant, kept to show that the tests notice it -- "rel" converts the offsets the other way, "trunc" truncates where
    floorf(u + 0.5f) belongs, "nocam" forgets the camera's pose."""
    T = np.dtype(dtype).type
    poses = np.asarray(poses, dtype); B = poses.shape[0]
    bones, off, rel = (np.asarray(a) for a in table)
    K = len(bones)
    two = T(2)
    left = np.zeros(B, bool) if hands is None else np.asarray(hands).reshape(B) != 0
    out = dict(xyz=np.zeros((B, K, 3), dtype))
    if cams is not None:
        cams = np.asarray(cams, dtype).reshape(B, 12)
        out["pix"] = np.zeros((B, K, 2), dtype); out["zc"] = np.zeros((B, K), dtype)
        if depth is not None:
            depth = np.asarray(depth); h, w = depth.shape[-2:]
            out["vis"] = np.zeros((B, K), np.uint8); out["ixy"] = np.full((B, K, 2), -1, np.int64)
    for k in range(K):
        b = int(bones[k])
        o = off[k].astype(dtype); com = model.com[b].astype(dtype)
        add = (rel[k] == 1 and not com_poses); sub = (rel[k] == 0 and com_poses)
        if wrong == "rel":
            add, sub = sub, add
        if add:
            o = o + com
        elif sub:
            o = o - com
        ox = np.where(left, -o[0], o[0]).astype(dtype)      # the sign bit
        ov = (ox, np.full(B, o[1], dtype), np.full(B, o[2], dtype))
        q = tuple(poses[:, b, 3 + i] for i in range(4))
        r = jr.qrot(q, ov, two)
        X = tuple(poses[:, b, i] + r[i] for i in range(3))
        for i in range(3):
            out["xyz"][:, k, i] = X[i]
        if cams is None:
            continue
        if wrong == "nocam":
            v = X
        else:
            qc = jr.qconj(tuple(cams[:, 8 + i] for i in range(4)))
            v = jr.qrot(qc, tuple(X[i] - cams[:, 5 + i] for i in range(3)), two)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            u = (v[0] / v[2] * cams[:, 0] + cams[:, 2], v[1] / v[2] * cams[:, 1] + cams[:, 3])
            out["pix"][:, k, 0], out["pix"][:, k, 1], out["zc"][:, k] = u[0], u[1], v[2]
            if depth is None:
                continue
            ux, uy = u[0] + T(0.5), u[1] + T(0.5)
            behind = ~(v[2] > 0)
            outside = ~((ux >= 0) & (ux < T(w))) | ~((uy >= 0) & (uy < T(h)))
            ok = ~behind & ~outside
            if wrong == "trunc":
                ix, iy = np.where(ok, u[0], 0).astype(np.int64), np.where(ok, u[1], 0).astype(np.int64)
            else:
                ix, iy = np.floor(np.where(ok, ux, 0)).astype(np.int64), np.floor(np.where(ok, uy, 0)).astype(np.int64)
            d = depth[np.arange(B), iy, ix].astype(dtype) * cams[:, 4]
            code = np.where(d < v[2] - T(near_tol), OCCLUDED, np.where(d > v[2] + T(far_tol), NOTHING, VISIBLE))
            out["vis"][:, k] = np.where(behind, BEHIND, np.where(outside, OUTSIDE, code))
            out["ixy"][:, k, 0], out["ixy"][:, k, 1] = np.where(ok, ix, -1), np.where(ok, iy, -1)
    return out


# ---- item 5: errors ---------------------------------------------------------------------------------------------------------------------------------
def errors(a, b, thr=(), dtype=np.float32):
    """a, b [B,K,3] -> dict(dist [B,K], frame [B,2] (mean, max), sum_kp f64[K], hits_kp i64[T], hits_frame i64[T]); a NaN distance makes its frame's mean and max NaN
    and hits nothing"""
    T = np.dtype(dtype).type
    a, b = np.asarray(a, dtype), np.asarray(b, dtype); B, K = a.shape[:2]
    thr = np.asarray(thr, dtype).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (a[..., i] - b[..., i] for i in range(3))
        dist = np.sqrt((dx * dx + dy * dy) + dz * dz).astype(dtype)
        s = np.zeros(B, dtype)
        for k in range(K):
            s = s + dist[:, k]
        frame = np.stack([s / T(K), np.max(dist, axis=1) if K else np.zeros(B, dtype)], -1).astype(dtype)
        hits_kp = np.array([(dist <= t).sum() for t in thr], np.int64).reshape(len(thr))
        hits_frame = np.array([(frame[:, 1] <= t).sum() for t in thr], np.int64).reshape(len(thr))
    return dict(dist=dist, frame=frame, sum_kp=dist.astype(np.float64).sum(axis=0), hits_kp=hits_kp, hits_frame=hits_frame)


# ---- item 6: depth comparison -------------------------------------------------------------------------------------------------------------------------
def depth_compare(a, b, lo, hi, tol):
    """a, b u16[B,h,w] -> info i64[B,8]: n_a, n_b, n_both, n_close, sum |a-b|, sum (a-b)^2, max |a-b| over the pixels in both, 0"""
    a, b = np.asarray(a, np.uint16).astype(np.int64), np.asarray(b, np.uint16).astype(np.int64); B = a.shape[0]
    a, b = a.reshape(B, -1), b.reshape(B, -1)
    ia, ib = (a >= lo) & (a < hi), (b >= lo) & (b < hi)
    both = ia & ib
    d = np.abs(a - b) * both
    info = np.zeros((B, 8), np.int64)
    info[:, 0], info[:, 1], info[:, 2], info[:, 3] = ia.sum(1), ib.sum(1), both.sum(1), (both & (d <= tol)).sum(1)
    info[:, 4], info[:, 5], info[:, 6] = d.sum(1), (d * d).sum(1), d.max(1) if d.shape[1] else 0
    return info


# ---- item 7: the composite's conversion ---------------------------------------------------------------------------------------------------------------
def identity_cams(cams):
    """which cameras' poses are (0,0,0, 0,0,0,1) bit for bit"""
    return (np.ascontiguousarray(np.asarray(cams, np.float32).reshape(-1, 12)[:, 5:12]).view(np.uint32) == IDENTITY_BITS).all(axis=1)


def pose_to_render(model, poses, cams, dtype=np.float32, com_poses=False):
    """poses [B,nb,7] -> the centre-of-mass poses in each frame's camera that ht_render_depth takes"""
    T = np.dtype(dtype).type
    poses = np.array(poses, dtype); B = poses.shape[0]
    ident = identity_cams(cams)
    cams = np.asarray(cams, dtype).reshape(B, 12)
    two = T(2)
    out = poses.copy()
    qi = jr.qconj(tuple(cams[:, 8 + i] for i in range(4)))
    for b in range(model.nb):
        q = tuple(poses[:, b, 3 + i] for i in range(4))
        pos = tuple(poses[:, b, i] for i in range(3))
        if not com_poses:
            r = jr.qrot(q, tuple(np.full(B, model.com[b, i], dtype) for i in range(3)), two)
            pos = tuple(pos[i] + r[i] for i in range(3))
        p2 = jr.qrot(qi, tuple(pos[i] - cams[:, 5 + i] for i in range(3)), two)
        q2 = jr.qmul(qi, q)
        for i in range(3):
            out[:, b, i] = np.where(ident, pos[i], p2[i])
        for i in range(4):
            out[:, b, 3 + i] = np.where(ident, q[i], q2[i])
    return out
