"""The hand's size from tracked frames (include/ht_mi355x.h "the hand's size") restated in numpy, operation for operation: the cloud is
views_ref.view_cloud's through calib_ref.cloud, closest() is the oracle's ho_closest (independent C, pinned to the reference), the per-point terms are float32 scalars in
csrc/ht_math.hpp's forms, the 37 sums are float64 in the header's order (a thread's points at stride 256, the wave's butterfly, the four waves as (w0 + w1) + (w2 + w3)),
the steps -- the scalar, the damped 7 x 7 and the Schur complement over the slots in slot order -- are written out in Python floats (IEEE float64: + - * / and sqrt only).
No code is shared with the kernels.  Test infrastructure only."""
import math

import numpy as np

import calib_ref as cr
import oracle_lib as ol

F, D = np.float32, np.float64
SHARED, PER_SLOT = 0, 1
STATS, SLOT_STATS = 6, 3
FEW_INLIERS, BAD_PIVOT, CLAMPED = 1, 2, 4
THREADS = 256
NSUM = 37
COST, INL = 35, 36


def row_len(N, B):
    return N * STATS + B * SLOT_STATS


def options(**kw):
    """ht_size_default's figures for a tracker with the stock parameters (drangey 0.7, subsample_fraction 4), then the fields given"""
    o = dict(range_lo=0.1, range_hi=0.7, fraction=4, mode=SHARED, free_pose=1, iterations=10, max_dist=0.03, damping=1e-3, min_points=12, scale0=1.0, scale_lo=0.5, scale_hi=2.0)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def at(i, j):
    """entry (i, j), i <= j, of the 7 x 7 upper triangle stored row by row"""
    return i * 7 - i * (i - 1) // 2 + (j - i)


def pulled(y, w, s):
    """u = w + (y - w) * (float)(1.0 / s) in float32; -> (e, u)"""
    inv = F(1.0 / s)
    e = [y[:, i] - w[i] for i in range(3)]
    return e, np.stack([w[i] + e[i] * inv for i in range(3)], axis=1).astype(F)


def terms(e, u, pl, s, max_dist):
    """per point (float32) r, J, the weight; then the 37 float64 terms [n,37]"""
    n = [pl[:, i] for i in range(3)]
    r0 = ((n[0] * u[:, 0] + n[1] * u[:, 1]) + n[2] * u[:, 2]) + pl[:, 3]
    r = F(s) * r0
    m = [e[1] * n[2] - e[2] * n[1], e[2] * n[0] - e[0] * n[2], e[0] * n[1] - e[1] * n[0]]
    j6 = r - ((n[0] * e[0] + n[1] * e[1]) + n[2] * e[2])
    J = [v.astype(D) for v in n + m + [j6]]
    with np.errstate(invalid="ignore"):
        inl = np.abs(r) <= F(max_dist)
    r64 = r.astype(D); md2 = D(F(max_dist)) * D(F(max_dist))
    cols = [np.where(inl, J[i] * J[j], 0.0) for i in range(7) for j in range(i, 7)] + [np.where(inl, J[i] * r64, 0.0) for i in range(7)]
    r2 = r64 * r64
    cols += [np.where(r2 < md2, r2, md2), np.where(inl, 1.0, 0.0)]
    return np.stack(cols, axis=1) if len(u) else np.zeros((0, NSUM), D)


def block_sum(t):
    """[n,K] -> [K] in the block's order"""
    K = t.shape[1]; k = (len(t) + THREADS - 1) // THREADS
    pad = np.zeros((k * THREADS, K), D); pad[:len(t)] = t      # (a thread's sum is never -0.0, so the padding's + 0.0 changes no bit)
    acc = np.zeros((THREADS, K), D)
    for j in range(k):
        acc = acc + pad[j * THREADS:(j + 1) * THREADS]
    v = acc.reshape(4, 64, K)
    while v.shape[1] > 1:
        half = v.shape[1] // 2
        v = v[:, :half] + v[:, half:]
    v = v[:, 0]
    return (v[0] + v[1]) + (v[2] + v[3])


def cholesky(L):
    """the lower triangle in L (lists), in place; -> every pivot was > 0"""
    n = len(L); ok = True
    for j in range(n):
        v = L[j][j]
        for k in range(j):
            v -= L[j][k] * L[j][k]
        if not v > 0.0:
            ok = False; v = 1.0
        pj = math.sqrt(v)
        L[j][j] = pj
        for i in range(j + 1, n):
            u = L[i][j]
            for k in range(j):
                u -= L[i][k] * L[j][k]
            L[i][j] = u / pj
    return ok


def substitute(L, rhs):
    n = len(L); y = [0.0] * n; d = [0.0] * n
    with np.errstate(all="ignore"):
        for i in range(n):
            v = rhs[i]
            for k in range(i):
                v -= L[i][k] * y[k]
            y[i] = _div(v, L[i][i])
        for i in range(n - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, n):
                v -= L[k][i] * d[k]
            d[i] = _div(v, L[i][i])
    return d


def _div(a, b):
    return float(D(a) / D(b))      # IEEE: no ZeroDivisionError


def moved(T, d, c):
    """the update of "a view's extrinsics" about c -> the new T, or None when a figure is not finite"""
    hx, hy, hz = d[3] * 0.5, d[4] * 0.5, d[5] * 0.5
    hl = math.sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0)
    ax, ay, az, aw = hx / hl, hy / hl, hz / hl, 1.0 / hl
    bx, by, bz, bw = T[3:7]
    q = [ax * bw + aw * bx + ay * bz - az * by, ay * bw + aw * by + az * bx - ax * bz, az * bw + aw * bz + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]
    ql = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [_div(v, ql) for v in q]
    px, py, pz = T[0] - c[0], T[1] - c[1], T[2] - c[2]
    X = (aw * aw + ax * ax - ay * ay - az * az, (ax * ay + az * aw) * 2.0, (az * ax - ay * aw) * 2.0)
    Y = ((ax * ay - az * aw) * 2.0, aw * aw - ax * ax + ay * ay - az * az, (ay * az + ax * aw) * 2.0)
    Z = ((az * ax + ay * aw) * 2.0, (ay * az - ax * aw) * 2.0, aw * aw - ax * ax - ay * ay + az * az)
    pos = [(c[i] + ((X[i] * px + Y[i] * py) + Z[i] * pz)) + d[i] for i in range(3)]
    new = pos + q
    return new if all(math.isfinite(v) for v in new + list(d)) else None


def _dot6(a, b):
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]


def _clamped(sn, o, flag):
    lo, hi = float(F(o["scale_lo"])), float(F(o["scale_hi"]))
    if sn < lo:
        return lo, flag | CLAMPED
    if sn > hi:
        return hi, flag | CLAMPED
    return sn, flag


def _finite(*v):
    return all(math.isfinite(x) for x in v)


def step_slot(S, s, T, c, o, last):
    """PER_SLOT: the slot's sums S [38], its scale and transform -> (s', T', dsigma taken, slot flag, scale flag)"""
    flag = FEW_INLIERS if S[INL] < float(o["min_points"]) else 0
    if last or flag:
        return s, T, 0.0, flag, flag
    damp = 1.0 + float(F(o["damping"]))
    with np.errstate(all="ignore"):
        if o["free_pose"]:
            L = [[0.0] * 7 for _ in range(7)]
            for i in range(7):
                for j in range(i, 7):
                    L[j][i] = float(S[at(i, j)])
                L[i][i] = L[i][i] * damp
            ok = cholesky(L)
            d = substitute(L, [-float(S[28 + i]) for i in range(7)])
        else:
            ok = float(S[27]) > 0.0
            d = [0.0] * 6 + [_div(-float(S[34]), float(S[27]) * damp)]
        cand = float(D(s) + D(s) * D(d[6]))
    ok = ok and _finite(d[6], cand)
    new = T
    if ok and o["free_pose"]:
        new = moved(T, d[:6], c)
        ok = new is not None
    if not ok:
        return s, T, 0.0, flag | BAD_PIVOT, flag | BAD_PIVOT
    sn, sflag = _clamped(cand, o, flag)
    return sn, new, d[6], flag, sflag


def pieces(S, o, last):
    """SHARED: a slot's Schur pieces (z, v, a - c.z, h - c.v, flag)"""
    z = [0.0] * 6; v = [0.0] * 6; sa = sb = 0.0
    flag = FEW_INLIERS if S[INL] < float(o["min_points"]) else 0
    if not last and not flag:
        if o["free_pose"]:
            damp = 1.0 + float(F(o["damping"]))
            L = [[0.0] * 6 for _ in range(6)]
            for i in range(6):
                for j in range(i, 6):
                    L[j][i] = float(S[at(i, j)])
                L[i][i] = L[i][i] * damp
            c = [float(S[at(i, 6)]) for i in range(6)]; g = [float(S[28 + i]) for i in range(6)]
            ok = cholesky(L)
            z = substitute(L, c); v = substitute(L, g)
            with np.errstate(all="ignore"):
                sa = float(D(S[27]) - D(_dot6(c, z))); sb = float(D(S[34]) - D(_dot6(c, v)))
        else:
            sa, sb = float(S[27]), float(S[34]); ok = sa > 0.0
        if not (ok and _finite(sa, sb)):
            flag |= BAD_PIVOT
    return z, v, sa, sb, flag


def estimate(orc, depth, cams, poses, o):
    """depth u16[B,h,w], cams [B,12], poses [B,nb,7] centre-of-mass poses -> (scale f32[N], T f32[B,7], stats f64[iterations + 1, row_len(N, B)])"""
    depth = np.asarray(depth); cams = np.asarray(cams, F); poses = np.ascontiguousarray(poses, F)
    B = len(depth); per = o["mode"] == PER_SLOT; N = B if per else 1
    co = dict(range_lo=o["range_lo"], range_hi=o["range_hi"], fraction=o["fraction"])
    with np.errstate(all="ignore"):
        clouds = [cr.cloud(depth[b], cams[b], co) for b in range(B)]
    T = [[float(D(v)) for v in cams[b, 5:12]] for b in range(B)]
    s = [float(D(F(o["scale0"])))] * N
    wrist = [[float(D(v)) for v in poses[b, 0, :3]] for b in range(B)]
    stats = np.zeros((o["iterations"] + 1, row_len(N, B)), D)
    damp = 1.0 + float(F(o["damping"]))
    for it in range(o["iterations"] + 1):
        last = it == o["iterations"]
        part = np.zeros((B, NSUM + 1), D)
        for b in range(B):
            T32 = np.array(T[b], D).astype(F)
            orc.L.ho_set_pose(orc.h, 0, ol.fptr(poses[b]))
            sb = s[b if per else 0]
            with np.errstate(all="ignore"):
                y = cr.place(T32, clouds[b])
                e, u = pulled(y, poses[b, 0, :3], sb)
                part[b, :NSUM] = block_sum(terms(e, u, cr.planes_of(orc, u), sb, o["max_dist"]))
            part[b, NSUM] = len(clouds[b])
        row = stats[it]; srec = row[N * STATS:].reshape(B, SLOT_STATS)
        if per:
            for b in range(B):
                s0 = s[b]
                s[b], T[b], ds, flag, sflag = step_slot(part[b], s[b], T[b], wrist[b], o, last)
                row[b * STATS:(b + 1) * STATS] = (part[b, INL], part[b, NSUM], part[b, COST], abs(ds), s0, sflag)
                srec[b] = (part[b, INL], part[b, COST], flag)
            continue
        pc = [pieces(part[b], o, last) for b in range(B)]
        SS = HH = 0.0; inl = pts = cost = 0.0; usable = 0
        with np.errstate(all="ignore"):
            for b in range(B):
                if pc[b][4] == 0:
                    SS = float(D(SS) + D(pc[b][2])); HH = float(D(HH) + D(pc[b][3])); usable += 1
                inl += part[b, INL]; pts += part[b, NSUM]; cost = float(D(cost) + part[b, COST])
        s0 = s[0]; ds = 0.0; go = False
        flag = 0 if usable else FEW_INLIERS if all(q[4] == FEW_INLIERS for q in pc) else BAD_PIVOT      # no usable slot
        if not last and not flag:
            with np.errstate(all="ignore"):
                d = _div(-HH, float(D(SS) * D(damp))); cand = float(D(s0) + D(s0) * D(d))
            if SS > 0.0 and _finite(d, cand):
                go = True; ds = d; s[0], flag = _clamped(cand, o, flag)
            else:
                flag |= BAD_PIVOT
        row[:STATS] = (inl, pts, cost, abs(ds), s0, flag)
        for b in range(B):
            z, v, _, _, f = pc[b]
            if go and not f and o["free_pose"]:
                with np.errstate(all="ignore"):
                    d = [-float(D(v[i]) + D(z[i]) * D(ds)) for i in range(6)]
                new = moved(T[b], d, wrist[b])
                if new is None:
                    f |= BAD_PIVOT
                else:
                    T[b] = new
            srec[b] = (part[b, INL], part[b, COST], f)
    return np.array(s, D).astype(F), np.array(T, D).astype(F), stats


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def stretched(poses, s):
    """centre-of-mass poses [.., nb, 7] stretched about body 0's position by the k_scale_state rule (float32: p0 + (p - p0) * s, body 0 untouched)"""
    p = np.array(poses, F); p0 = p[..., :1, :3].copy()
    out = p.copy()
    out[..., 1:, :3] = p0 + (p[..., 1:, :3] - p0) * F(s)
    return out
