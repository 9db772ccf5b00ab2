"""PhysicsUpdate (physics.h:543-587) in float64, batched over scenes: the plain statement that the solver fuzz (tests/test_solve_ref.py,
tests/test_gpu_solve_fuzz.py) measures the fp32 restatement (oracle/ho_physics.c:184-286) and k_solve against.  numpy only; nothing of the oracle is imported.

    rbinitvelocity (damping; gravity is zero) -> `iterations` sweeps (every linear row, then every angular row, in row order; a friction row's limits
    from its master's current impulse sum x the larger body friction / deltaT; an angular row with targetspin == -FLT_MAX is skipped) -> RK4 orientation with
    the FLT_EPSILON/4 flush -> RemoveBias of both row kinds -> `iterations_post` sweeps -> commit.

Row order and batching.  Two rows that touch disjoint bodies commute exactly, in any arithmetic: each body sees the same operations on the same operands in the same
order.  So the rows of a scene are placed in levels (level = 1 + the highest level of an earlier row sharing a body; a friction row shares its master's bodies), and one
numpy step applies level L of every scene at once.  That is the row order of the reference, bit for bit in float64, without a Python loop over (scene, row).

Rows are [n,16] (rb0 rb1 position0 position1 normal targetdist targetspeednobias forcelimit(2) friction_master) and [n,8] (rb0 rb1 axis targetspin mintorque maxtorque), as
htfx.load gives the golden rows; a batch is a list of such arrays, shorter lists being padded with rows whose limits are zero (they are never scheduled).

mutant= (for this reference only): ("swap", i) rows i and i + 1 of the list [linear rows | angular rows] in the other order (i may be a per-scene sequence, -1 = none);
("post",) one post-sweep fewer; ("nobias",) no RemoveBias on angular rows; ("stale_friction",) friction limits from the master's sum at the start of the sweep;
("drop_last_run",) without the last run of consecutive angular rows on one body pair."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
FLT_EPS = float(np.finfo(np.float32).eps)


def _qdirs(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    xd = np.stack([w * w + x * x - y * y - z * z, (x * y + z * w) * 2, (z * x - y * w) * 2], -1)
    yd = np.stack([(x * y - z * w) * 2, w * w - x * x + y * y - z * z, (y * z + x * w) * 2], -1)
    zd = np.stack([(z * x + y * w) * 2, (y * z - x * w) * 2, w * w - x * x - y * y + z * z], -1)
    return xd, yd, zd


def qmat(q):
    """[...,3,3] rotation matrix (columns = qxdir, qydir, qzdir)"""
    return np.stack(_qdirs(q), -1)


def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([ax * bw + aw * bx + ay * bz - az * by, ay * bw + aw * by + az * bx - ax * bz, az * bw + aw * bz + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def _normalize(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def _world_inertia(q, tinv):
    M = qmat(q)
    return M @ tinv @ np.swapaxes(M, -1, -2)


def _rkupdateq(s, tinv, angular, dt):
    def diffq(o):
        sn = _normalize(o)
        half = 0.5 * np.einsum("...ij,...j->...i", _world_inertia(sn, tinv), angular)
        return qmul(np.concatenate([half, np.zeros_like(half[..., :1])], -1), sn)
    d1 = diffq(s); d2 = diffq(s + d1 * (dt / 2)); d3 = diffq(s + d2 * (dt / 2)); d4 = diffq(s + d3 * dt)
    return _normalize(s + d1 * (dt / 6) + d2 * (dt / 3) + d3 * (dt / 3) + d4 * (dt / 6))


def angular_runs(ang):
    """first rows of the runs of consecutive angular rows on one body pair, and the row count behind them: [r0, r1, ..., n]"""
    heads = [i for i in range(len(ang)) if i == 0 or int(ang[i][0]) != int(ang[i - 1][0]) or int(ang[i][1]) != int(ang[i - 1][1])]
    return heads + [len(ang)]


def _levels(scenes_bodies, orders, nb):
    """per scene: rows in execution order -> lists of (level -> rows); returns {level: (scene indices, row indices)} as arrays"""
    out = {}
    for s, (bodies, order) in enumerate(zip(scenes_bodies, orders)):
        last = [0] * nb
        for i in order:
            b0, b1 = bodies[i]
            lv = 1 + max(last[b0] if b0 >= 0 else 0, last[b1] if b1 >= 0 else 0)
            if b0 >= 0: last[b0] = lv
            if b1 >= 0: last[b1] = lv
            out.setdefault(lv, ([], []))
            out[lv][0].append(s); out[lv][1].append(i)
    return [(np.array(out[k][0], np.intp), np.array(out[k][1], np.intp)) for k in sorted(out)]


def _pad(rows, width):
    n = max([len(r) for r in rows] + [1])
    buf = np.zeros((len(rows), n, width), np.float64)
    buf[:, :, 0] = -1.0; buf[:, :, 1] = 0.0; buf[:, :, 4 if width == 8 else 10] = 1.0      # a row on body 0 from the world along z whose limits are zero
    for s, r in enumerate(rows):
        if len(r):
            buf[s, :len(r)] = np.asarray(r, np.float64).reshape(-1, width)
    return buf


def physics_update(state, lin, ang, body_f, physics, mutant=None):
    """state [S,nb,13] (or [nb,13] with lin [n,16] and ang [n,8] of one scene) -> (state float64, linear impulse sums, angular torque sums), the sums as lists of
    per-scene arrays in the caller's row order"""
    state = np.asarray(state, np.float64)
    single = state.ndim == 2
    if single:
        state, lin, ang = state[None], [lin], [ang]
    lin = [np.asarray(r, np.float64).reshape(-1, 16) for r in lin]; ang = [np.asarray(r, np.float64).reshape(-1, 8) for r in ang]
    S, nb = state.shape[0], state.shape[1]
    mutant = tuple(mutant) if mutant else ("none",)
    if mutant[0] == "drop_last_run":
        ang = [a[:angular_runs(a)[-2]] if len(a) else a for a in ang]
    body_f = np.asarray(body_f, np.float64); ph = np.asarray(physics, np.float64)
    dt = ph[0]; iterations, post = int(ph[12]), int(ph[13])
    if mutant[0] == "post":
        post -= 1
    massinv, fric = body_f[:, 1], body_f[:, 5]
    tinv = np.swapaxes(body_f[:, 17:26].reshape(nb, 3, 3), 1, 2) * massinv[:, None, None]      # tensorinv_massless (stored by columns) * massinv

    nl = [len(r) for r in lin]; na = [len(r) for r in ang]
    LR, AR = _pad(lin, 16), _pad(ang, 8)
    lorder = [list(range(n)) for n in nl]; aorder = [list(range(n)) for n in na]
    if mutant[0] == "swap":
        idx = mutant[1] if np.ndim(mutant[1]) else [mutant[1]] * S
        for s, i in enumerate(idx):
            i = int(i)
            if 0 <= i < nl[s] - 1: lorder[s][i], lorder[s][i + 1] = lorder[s][i + 1], lorder[s][i]
            elif i >= nl[s] and i - nl[s] < na[s] - 1: k = i - nl[s]; aorder[s][k], aorder[s][k + 1] = aorder[s][k + 1], aorder[s][k]
            else: assert i < 0, "swap: rows %d and %d are not two rows of one kind in scene %d" % (i, i + 1, s)
    lsteps = _levels([[(int(r[0]), int(r[1])) for r in rows] for rows in lin], lorder, nb)
    asteps = _levels([[(int(r[0]), int(r[1])) for r in rows] for rows in ang], aorder, nb)

    # ---- rbinitvelocity (physics.h:500-519): damping; gravity and gravscale are zero for the tracker
    pos, q = state[:, :, 0:3].copy(), state[:, :, 3:7].copy()
    damp = np.power(1.0 - np.maximum(body_f[:, 4], ph[11]), dt)
    P = state[:, :, 7:10] * damp[None, :, None]; L = state[:, :, 10:13] * damp[None, :, None]
    assert not np.any(ph[2:5]), "gravity is zero for the tracker"
    Iinv = _world_inertia(q, tinv[None])

    lrb0, lrb1 = LR[:, :, 0].astype(np.intp), LR[:, :, 1].astype(np.intp)
    lfm = LR[:, :, 15].astype(np.intp)
    lsum = np.zeros(LR.shape[:2]); lts = LR[:, :, 11] / dt
    arb0, arb1 = AR[:, :, 0].astype(np.intp), AR[:, :, 1].astype(np.intp)
    aspin = AR[:, :, 5].copy(); atorque = np.zeros(AR.shape[:2])

    def rot(s, b, v):      # qrot(orientation of body b, v) for b >= 0, v itself for the world
        return np.where((b >= 0)[:, None], np.einsum("kij,kj->ki", qmat(q[s, np.maximum(b, 0)]), v), v)

    def linear_iter(s, i, stale):
        b0, b1 = lrb0[s, i], lrb1[s, i]; m0, m1 = b0 >= 0, b1 >= 0; c0, c1 = np.maximum(b0, 0), np.maximum(b1, 0)
        row = LR[s, i]; n = row[:, 8:11]
        lo, hi = row[:, 13].copy(), row[:, 14].copy()
        fr = lfm[s, i] != 0
        if fr.any():
            src = stale if stale is not None else lsum
            mu = np.maximum(np.where(m0, fric[c0], 0.0), np.where(m1, fric[c1], 0.0))
            lim = mu * src[s, np.where(fr, i + lfm[s, i], i)] / dt
            hi = np.where(fr, lim, hi); lo = np.where(fr, -lim, lo)
        r0, r1 = rot(s, b0, row[:, 2:5]), rot(s, b1, row[:, 5:8])
        I0, I1 = Iinv[s, c0], Iinv[s, c1]
        v0 = np.where(m0[:, None], np.cross(np.einsum("kij,kj->ki", I0, L[s, c0]), r0) + P[s, c0] * massinv[c0][:, None], 0.0)
        v1 = np.where(m1[:, None], np.cross(np.einsum("kij,kj->ki", I1, L[s, c1]), r1) + P[s, c1] * massinv[c1][:, None], 0.0)
        vn = ((v1 - v0) * n).sum(-1)
        d0 = massinv[c0] + (np.cross(np.einsum("kij,kj->ki", I0, np.cross(r0, n)), r0) * n).sum(-1)
        d1 = massinv[c1] + (np.cross(np.einsum("kij,kj->ki", I1, np.cross(r1, n)), r1) * n).sum(-1)
        impulse = (-lts[s, i] - vn) / (np.where(m0, d0, 0.0) + np.where(m1, d1, 0.0))
        impulse = np.minimum(hi * dt - lsum[s, i], impulse)
        impulse = np.maximum(lo * dt - lsum[s, i], impulse)
        imp = n * impulse[:, None]
        k = m0; P[s[k], b0[k]] -= imp[k]; L[s[k], b0[k]] += np.cross(r0[k], -imp[k])
        k = m1; P[s[k], b1[k]] += imp[k]; L[s[k], b1[k]] += np.cross(r1[k], imp[k])
        lsum[s, i] += impulse

    def angular_iter(s, i):
        on = aspin[s, i] != -FLT_MAX
        s, i = s[on], i[on]
        if not len(s):
            return
        b0, b1 = arb0[s, i], arb1[s, i]; m0, m1 = b0 >= 0, b1 >= 0; c0, c1 = np.maximum(b0, 0), np.maximum(b1, 0)
        ax = AR[s, i, 2:5]
        Ia0, Ia1 = np.einsum("kij,kj->ki", Iinv[s, c0], ax), np.einsum("kij,kj->ki", Iinv[s, c1], ax)
        spin0 = (np.einsum("kij,kj->ki", Iinv[s, c0], L[s, c0]) * ax).sum(-1); spin1 = (np.einsum("kij,kj->ki", Iinv[s, c1], L[s, c1]) * ax).sum(-1)
        current = np.where(m1, spin1, 0.0) - np.where(m0, spin0, 0.0)
        s2t = 1.0 / (np.where(m0, (ax * Ia0).sum(-1), 0.0) + np.where(m1, (ax * Ia1).sum(-1), 0.0))
        dtq = (aspin[s, i] - current) * s2t
        dtq = np.minimum(dtq, AR[s, i, 7] * dt - atorque[s, i])
        dtq = np.maximum(dtq, AR[s, i, 6] * dt - atorque[s, i])
        k = m0; L[s[k], b0[k]] -= ax[k] * dtq[k, None]
        k = m1; L[s[k], b1[k]] += ax[k] * dtq[k, None]
        atorque[s, i] += dtq

    def sweeps(count):
        for _ in range(count):
            stale = lsum.copy() if mutant[0] == "stale_friction" else None
            for s, i in lsteps: linear_iter(s, i, stale)
            for s, i in asteps: angular_iter(s, i)

    sweeps(iterations)
    # ---- rbcalcnextpose (physics.h:521-531): the pose is taken here, before RemoveBias and the post-sweeps
    pos_next = pos + P * massinv[None, :, None] * dt
    o = _rkupdateq(q, tinv[None], L, dt)
    o[..., :3] = np.where(np.abs(o[..., :3]) < FLT_EPS / 4.0, 0.0, o[..., :3])
    lts = np.minimum(lts, LR[:, :, 12])                                                   # physics.h:288
    if mutant[0] != "nobias":
        aspin = np.where(AR[:, :, 6] < 0, 0.0, np.minimum(aspin, 0.0))                    # physics.h:250
    sweeps(post)
    out = np.concatenate([pos_next, o, P, L], -1)
    sums = [lsum[s, :nl[s]].copy() for s in range(S)], [atorque[s, :na[s]].copy() for s in range(S)]
    if single:
        return out[0], sums[0][0], sums[1][0]
    return out, sums[0], sums[1]
