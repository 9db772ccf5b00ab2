"""A view's extrinsics from the tracked hand (include/ht_mi355x.h "a view's extrinsics") restated in numpy, operation for operation: the cloud is
views_ref.view_cloud's, closest() is the oracle's ho_closest (independent C, pinned to the reference), the per-point terms are float32 scalars in csrc/ht_math.hpp's forms,
the 29 sums are float64 in the header's order (a thread's points at stride 256, the wave's butterfly, the four waves as (w0 + w1) + (w2 + w3), the slots in slot order), the
Cholesky step is written out in Python floats (IEEE float64: + - * / and sqrt only).  No code is shared with the kernels.  Test infrastructure only."""
import ctypes as C
import math

import numpy as np

import kpfit_inputs as ki
import oracle_lib as ol
import views_ref as vr

F, D = np.float32, np.float64
RIG, PER_SLOT = 0, 1
STATS = 27
FEW_INLIERS, BAD_PIVOT = 1, 2
THREADS = 256


def options(**kw):
    """ht_calib_default's figures for a tracker with the stock parameters (drangey 0.7, subsample_fraction 4), then the fields given"""
    o = dict(range_lo=0.1, range_hi=0.7, fraction=4, mode=RIG, iterations=10, max_dist=0.03, damping=1e-3, min_points=12, centre=(0.0, 0.0, 0.0))
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def cloud(depth, cam, o):
    """the view's cloud in its camera's own space [n,3]: ht_fuse_views' for V = 1, an identity pose and no plane"""
    c = np.array(cam, F); c[5:12] = (0, 0, 0, 0, 0, 0, 1)
    return np.ascontiguousarray(vr.view_cloud(depth, c, None, o["range_lo"], o["range_hi"], o["fraction"], 0.0)[0][:, :3])


def place(T32, p):
    """x = pos + qrot(q, p) in float32 for points p [n,3]"""
    r = vr.qrot(T32[3:7], (p[:, 0], p[:, 1], p[:, 2]))
    return np.stack([T32[i] + r[i] for i in range(3)], axis=1).astype(F)


def planes_of(orc, x):
    """closest(bodies, x) of every point through ho_closest on the oracle's model 0 -> [n,4]"""
    m = orc.model(0); out = np.zeros((len(x), 4), F); p = ol.F4()
    for i, v in enumerate(x):
        orc.L.ho_closest(m, ol.F3(float(v[0]), float(v[1]), float(v[2])), C.byref(p))
        out[i] = (p.x, p.y, p.z, p.w)
    return out


def terms(x, pl, centre, max_dist):
    """per point (float32) r, J, the weight; then the 29 float64 terms [n,29]"""
    n = [pl[:, i] for i in range(3)]
    r = ((n[0] * x[:, 0] + n[1] * x[:, 1]) + n[2] * x[:, 2]) + pl[:, 3]
    d = [x[:, i] - F(centre[i]) for i in range(3)]
    m = [d[1] * n[2] - d[2] * n[1], d[2] * n[0] - d[0] * n[2], d[0] * n[1] - d[1] * n[0]]
    J = [v.astype(D) for v in n + m]
    with np.errstate(invalid="ignore"):
        inl = np.abs(r) <= F(max_dist)
    r64 = r.astype(D); md2 = D(F(max_dist)) * D(F(max_dist))
    cols = [np.where(inl, J[i] * J[j], 0.0) for i in range(6) for j in range(i, 6)] + [np.where(inl, J[i] * r64, 0.0) for i in range(6)]
    r2 = r64 * r64
    cols += [np.where(r2 < md2, r2, md2), np.where(inl, 1.0, 0.0)]
    return np.stack(cols, axis=1) if len(x) else np.zeros((0, 29), D)


def block_sum(t):
    """[n,29] -> [29] in the block's order"""
    k = (len(t) + THREADS - 1) // THREADS
    pad = np.zeros((k * THREADS, 29), D); pad[:len(t)] = t      # (a thread's sum is never -0.0, so the padding's + 0.0 changes no bit)
    acc = np.zeros((THREADS, 29), D)
    for j in range(k):
        acc = acc + pad[j * THREADS:(j + 1) * THREADS]
    v = acc.reshape(4, 64, 29)
    while v.shape[1] > 1:
        half = v.shape[1] // 2
        v = v[:, :half] + v[:, half:]
    v = v[:, 0]
    return (v[0] + v[1]) + (v[2] + v[3])


def step(S, T, o, last):
    """the sums S [29] (+ the point count) and T (7 Python floats) -> (T', |dt|, |dw|, flag)"""
    flag = FEW_INLIERS if S[28] < float(o["min_points"]) else 0
    if last or flag:
        return T, 0.0, 0.0, flag
    L = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            L[j][i] = float(S[k]); k += 1
    scale = 1.0 + float(F(o["damping"]))
    for i in range(6):
        L[i][i] = L[i][i] * scale
    ok = True
    for j in range(6):
        v = L[j][j]
        for k in range(j):
            v -= L[j][k] * L[j][k]
        if not v > 0.0:
            ok = False; v = 1.0
        pj = math.sqrt(v)
        L[j][j] = pj
        for i in range(j + 1, 6):
            u = L[i][j]
            for k in range(j):
                u -= L[i][k] * L[j][k]
            L[i][j] = u / pj
    y = [0.0] * 6; d = [0.0] * 6
    for i in range(6):
        v = -float(S[21 + i])
        for k in range(i):
            v -= L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k][i] * d[k]
        d[i] = v / L[i][i]
    c = [float(F(v)) for v in o["centre"]]
    hx, hy, hz = d[3] * 0.5, d[4] * 0.5, d[5] * 0.5
    hl = math.sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0)
    ax, ay, az, aw = hx / hl, hy / hl, hz / hl, 1.0 / hl
    bx, by, bz, bw = T[3:7]
    q = [ax * bw + aw * bx + ay * bz - az * by, ay * bw + aw * by + az * bx - ax * bz, az * bw + aw * bz + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]
    ql = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [v / ql for v in q]
    px, py, pz = T[0] - c[0], T[1] - c[1], T[2] - c[2]
    X = (aw * aw + ax * ax - ay * ay - az * az, (ax * ay + az * aw) * 2.0, (az * ax - ay * aw) * 2.0)
    Y = ((ax * ay - az * aw) * 2.0, aw * aw - ax * ax + ay * ay - az * az, (ay * az + ax * aw) * 2.0)
    Z = ((az * ax + ay * aw) * 2.0, (ay * az - ax * aw) * 2.0, aw * aw - ax * ax - ay * ay + az * az)
    pos = [(c[i] + ((X[i] * px + Y[i] * py) + Z[i] * pz)) + d[i] for i in range(3)]
    new = pos + q
    if not (ok and all(math.isfinite(v) for v in new + d)):
        return T, 0.0, 0.0, flag | BAD_PIVOT
    return new, math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), math.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]), flag


def calibrate(orc, depth, cams, poses, o):
    """depth u16[B,h,w], cams [B,12] (the guess in [:,5:12]), poses [B,nb,7] centre-of-mass poses -> (T_out f32[N,7], stats f64[iterations + 1,N,27])"""
    depth = np.asarray(depth); cams = np.asarray(cams, F); poses = np.ascontiguousarray(poses, F)
    B = len(depth); per = o["mode"] == PER_SLOT; N = B if per else 1
    with np.errstate(all="ignore"):
        clouds = [cloud(depth[b], cams[b], o) for b in range(B)]
    T = [[float(D(v)) for v in cams[s, 5:12]] for s in range(N)]
    stats = np.zeros((o["iterations"] + 1, N, STATS), D)
    for it in range(o["iterations"] + 1):
        part = np.zeros((B, 30), D)
        for b in range(B):
            T32 = np.array(T[b if per else 0], D).astype(F)
            orc.L.ho_set_pose(orc.h, 0, ol.fptr(poses[b]))
            with np.errstate(all="ignore"):
                x = place(T32, clouds[b])
                part[b, :29] = block_sum(terms(x, planes_of(orc, x), o["centre"], o["max_dist"]))
            part[b, 29] = len(clouds[b])
        for s in range(N):
            S = part[s].copy()
            if not per:
                for b in range(1, B):
                    S = S + part[b]
            T[s], ndt, ndw, flag = step(S, T[s], o, it == o["iterations"])
            stats[it, s, :6] = (S[28], S[29], S[27], ndt, ndw, flag)
            stats[it, s, 6:] = S[:21]
    return np.array(T, D).astype(F), stats


# ---- scenes and measures ------------------------------------------------------------------------------------------------------------------------------------------
def rig_scene(name, frames, w, h, degrees):
    """views_ref.two_view_scene with a FIXED second camera (the rig is fixed and the hand moves): the orbit of frames[0]'s scene, every frame rendered from it
    -> dict(depth [B,2,h,w], cams [B,2,12], truth [B,nb,7])"""
    first = vr.two_view_scene(name, frames[:1], w, h, degrees)
    P = ki.truths(name); cam0, cam1 = first["cams"][0]
    depth = [first["depth"][0]] + [np.stack([vr.render(name, P[f % len(P)], cam0, w, h), vr.render(name, P[f % len(P)], cam1, w, h)]) for f in frames[1:]]
    return dict(depth=np.stack(depth), cams=np.tile(first["cams"][0], (len(frames), 1, 1)), truth=np.stack([P[f % len(P)] for f in frames]))


def perturbed(cam, degrees, shift, axis=(1.0, 1.0, 0.0)):
    """`cam` with its pose turned by `degrees` about `axis` through the camera's own position and then moved by `shift` metres along (1,-1,1)/sqrt 3"""
    a = np.asarray(axis, D); a = a / np.linalg.norm(a); t = np.deg2rad(degrees) / 2.0
    dq = np.concatenate([a * np.sin(t), [np.cos(t)]])
    out = np.array(cam, F)
    out[8:12] = vr._qmul(dq, np.asarray(cam[8:12], D)).astype(F)
    out[5:8] = (np.asarray(cam[5:8], D) + np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0) * shift).astype(F)
    return out


def rigid_error(Ta, Tb, pts):
    """the mean distance (metres) between where two transforms put the points [n,3]"""
    pa = np.array([Ta[:3] + vr.qrot64(np.asarray(Ta[3:7], D), p) for p in pts.astype(D)]); pb = np.array([Tb[:3] + vr.qrot64(np.asarray(Tb[3:7], D), p) for p in pts.astype(D)])
    return float(np.linalg.norm(pa - pb, axis=1).mean())
