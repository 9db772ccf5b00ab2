"""The joint coordinates restated in numpy (include/ht_mi355x.h "joint coordinates"): read-out, forward kinematics, limits and
the sampler.  Every function takes a dtype: np.float32 evaluates one rounding per operation in the order of oracle/ho_math.h (what the kernels must equal
bit for bit), np.float64 is the yardstick the float32 statement is measured against.  Test infrastructure only; shares no code with the kernels.

Quaternions and vectors are tuples of arrays (x, y, z[, w]) so that every operation stands where it is evaluated."""
import math

import numpy as np

import htfx


class Model:
    """The joint table of a baked model file: rb0 / rb1 [nj], p0 / p1 / rmin / rmax [nj,3], frame [nj,4], com [nb,3]."""

    def __init__(self, path):
        m = htfx.load(path)
        self.nb, self.nj = int(m["nb"][0]), int(m["nj"][0])
        ji, jf = m["joint_i"].reshape(self.nj, 2), m["joint_f"].reshape(self.nj, 16).astype(np.float32)
        self.rb0, self.rb1 = ji[:, 0].copy(), ji[:, 1].copy()
        self.p0, self.p1, self.rmin, self.rmax, self.frame = jf[:, 0:3], jf[:, 3:6], jf[:, 6:9].copy(), jf[:, 9:12].copy(), jf[:, 12:16]
        self.com = m["body_f"].reshape(self.nb, 26)[:, 7:10].astype(np.float32)
        self.deltaT, self.biasfactorjoint = np.float32(m["physics"][0]), np.float32(m["physics"][6])


# ---- ho_math.h ---------------------------------------------------------------------------------------------------------
def qmul(a, b):
    return (a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1], a[1] * b[3] + a[3] * b[1] + a[2] * b[0] - a[0] * b[2],
            a[2] * b[3] + a[3] * b[2] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2])


def qconj(q):
    return (-q[0], -q[1], -q[2], q[3])


def qxdir(q, two):
    return (q[3] * q[3] + q[0] * q[0] - q[1] * q[1] - q[2] * q[2], (q[0] * q[1] + q[2] * q[3]) * two, (q[2] * q[0] - q[1] * q[3]) * two)


def qydir(q, two):
    return ((q[0] * q[1] - q[2] * q[3]) * two, q[3] * q[3] - q[0] * q[0] + q[1] * q[1] - q[2] * q[2], (q[1] * q[2] + q[0] * q[3]) * two)


def qzdir(q, two):
    return ((q[2] * q[0] + q[1] * q[3]) * two, (q[1] * q[2] - q[0] * q[3]) * two, q[3] * q[3] - q[0] * q[0] - q[1] * q[1] + q[2] * q[2])


def qrot(q, v, two):
    x, y, z = qxdir(q, two), qydir(q, two), qzdir(q, two)
    return tuple((x[i] * v[0] + y[i] * v[1]) + z[i] * v[2] for i in range(3))


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def dot4(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]


def normalize(v):
    n = np.sqrt(dot4(v, v) if len(v) == 4 else dot3(v, v))
    return tuple(c / n for c in v)


def quat_from_to_z(b, T):
    """quat_from_to((0,0,1), b), geometric.h:319-328, its d <= -1 branch included"""
    zero, one, two = np.zeros_like(b[0]), np.ones_like(b[0]), T(2)
    v0 = normalize((zero, zero, one))
    v1 = normalize(b)
    c = (v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0])
    d = dot3(v0, v1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt((one + d) * two)
        q = (c[0] / s, c[1] / s, c[2] / s, s / two)
    o = normalize((one * one - zero * zero, zero * zero - one * one, one * zero - one * zero))      # orth((0,0,1)) = normalize(cross((1,1,0), (0,0,1)))
    flip = d <= -one
    return tuple(np.where(flip, a, b_) for a, b_ in zip((o[0], o[1], o[2], zero), q))


def cb_of(like, T):
    z, o = np.zeros_like(like), np.ones_like(like)
    return normalize((z, -o, z, o))


def _q(a):
    return tuple(a[..., i] for i in range(4))


def _v(a):
    return tuple(a[..., i] for i in range(3))


# ---- definition 3: the limits ----------------------------------------------------------------------------------------------
def _sinf(x):
    return np.float32(math.sin(float(x)))      # the double sine rounded once: a correctly rounded sinf


def limits(model, ignore_swap=False, y_lock_sine=False):
    """(lo [nj,3], hi [nj,3], swapped [nj], unbounded [nj,3]) in float32.  An unbounded axis carries the sampler's +-sin(90 deg / 2)."""
    f = np.float32
    lo, hi = np.zeros((model.nj, 3), f), np.zeros((model.nj, 3), f)
    sw, unb = np.zeros(model.nj, bool), np.zeros((model.nj, 3), bool)
    wide = _sinf((f(90.0) * f(3.14) / f(180.0)) / f(2.0))
    for j in range(model.nj):
        lmin, lmax = model.rmin[j].astype(f), model.rmax[j].astype(f)
        jmin, jmax = (lmin * f(3.14)) / f(180.0), (lmax * f(3.14)) / f(180.0)
        if jmin[0] == 0 and jmax[0] == 0 and jmin[2] < jmax[2] and not ignore_swap:
            sw[j] = True
            lmin, lmax = np.array([lmin[2], lmin[1], 0], f), np.array([lmax[2], lmax[1], 0], f)
            jmin, jmax = (lmin * f(3.14)) / f(180.0), (lmax * f(3.14)) / f(180.0)
        if jmax[0] == jmin[0]:
            lo[j, 0] = hi[j, 0] = _sinf(jmin[0] / f(2))
        elif jmax[0] - jmin[0] < f(360.0) * f(3.14) / f(180.0):
            lo[j, 0], hi[j, 0] = _sinf(jmin[0] / f(2)), _sinf(jmax[0] / f(2))
        else:
            lo[j, 0], hi[j, 0], unb[j, 0] = -wide, wide, True
        if jmax[1] == jmin[1]:
            lo[j, 1] = hi[j, 1] = _sinf(jmin[1] / f(2)) if y_lock_sine else jmin[1]
        else:
            lo[j, 1], hi[j, 1] = _sinf(jmin[1] / f(2)), _sinf(jmax[1] / f(2))
        if jmin[2] == jmax[2]:
            lo[j, 2] = hi[j, 2] = 0
        else:
            lo[j, 2], hi[j, 2] = _sinf(jmin[2] / f(2)), _sinf(jmax[2] / f(2))
    return lo, hi, sw, unb


# ---- definitions 1, 2, 4: the read-out --------------------------------------------------------------------------------------
def to_user(model, poses, T):
    """centre-of-mass poses -> user poses: PositionUser = position + qrot(q, -com), physics.h:142"""
    p, q = _v(poses[..., :3]), _q(poses[..., 3:])
    com = tuple(-model.com[:, i].astype(T) for i in range(3))
    r = qrot(q, com, T(2))
    out = poses.copy()
    for i in range(3):
        out[..., i] = p[i] + r[i]
    return out


def coords(model, poses, dtype=np.float32, com_poses=False, swapped=None, canonical=False):
    """poses [B,nb,7] -> (coords [B,nj,3], gaps [B,nj]).  swapped: the joints' swap flags (default: the model's own); canonical: a WRONG variant that
    flips r to w >= 0, kept to show that the tests notice it."""
    T = np.dtype(dtype).type
    poses = np.asarray(poses, dtype)
    if swapped is None:
        swapped = limits(model)[2]
    B = poses.shape[0]
    c = np.zeros((B, model.nj, 3), dtype); gaps = np.zeros((B, model.nj), dtype)
    user = to_user(model, poses, T) if com_poses else poses
    two = T(2)
    for j in range(model.nj):
        a, b = user[:, model.rb0[j]], user[:, model.rb1[j]]
        q0, q1 = _q(a[:, 3:]), _q(b[:, 3:])
        F = tuple(np.full(B, model.frame[j, i], dtype) for i in range(4))
        Jb, Jf = qmul(q0, F), q1
        if swapped[j]:
            cb = cb_of(q0[0], T)
            Jb, Jf = qmul(Jb, cb), qmul(Jf, cb)
        r = qmul(qconj(Jb), Jf)
        if canonical:
            sg = np.where(r[3] < 0, T(-1), T(1)); r = tuple(x * sg for x in r)
        s = quat_from_to_z(qzdir(r, two), T)
        t = qmul(qconj(s), r)
        c[:, j, 0], c[:, j, 1], c[:, j, 2] = s[0], s[1], t[2]
        p0 = tuple(np.full(B, model.p0[j, i], dtype) for i in range(3)); p1 = tuple(np.full(B, model.p1[j, i], dtype) for i in range(3))
        r0, r1 = qrot(q0, p0, two), qrot(q1, p1, two)
        d = tuple((a[:, i] + r0[i]) - (b[:, i] + r1[i]) for i in range(3))
        gaps[:, j] = np.sqrt(dot3(d, d))
    return c, gaps


# ---- definition 5: forward kinematics ------------------------------------------------------------------------------------------
COS40 = math.cos(float(np.float32(40.0) * np.float32(3.14) / np.float32(180.0)))      # handtrack.h:437, in double
TIP_JOINTS, KNUCKLE_JOINTS = (6, 9, 12, 15), (4, 7, 10, 13)                        # handtrack.h:417, 434: joint j attaches bone j + 1


def _child(q0, F, sw, cx, cy, cz, T):
    zero, one = np.zeros_like(cx), np.ones_like(cx)
    ws = (one - cx * cx) - cy * cy; ws = np.sqrt(np.where(zero < ws, ws, zero))
    wt = one - cz * cz; wt = np.sqrt(np.where(zero < wt, wt, zero))
    q = qmul(q0, F)
    if sw:
        q = qmul(q, cb_of(cx, T))
    q = qmul(qmul(q, (cx, cy, zero, ws)), (zero, zero, cz, wt))
    if sw:
        q = qmul(q, qconj(cb_of(cx, T)))
    return normalize(q)


def pose(model, roots, c, dtype=np.float32, com_poses=False, swapped=None, enhanced=False):
    """roots [B,7], c [B,nj,3] -> poses [B,nb,7] (user poses, or centre-of-mass poses in and out with com_poses).  enhanced (the sampler's flag):
    HandModelEnhancements' couplings rewrite c on the way, and (poses, c) is returned."""
    T = np.dtype(dtype).type
    roots, c = np.asarray(roots, dtype), np.array(c, dtype)
    if swapped is None:
        swapped = limits(model)[2]
    B = roots.shape[0]
    zero, one, two = np.zeros(B, dtype), np.ones(B, dtype), T(2)
    out = np.zeros((B, model.nb, 7), dtype)
    out[:, 0] = roots
    if com_poses:
        r = qrot(_q(roots[:, 3:]), tuple(np.full(B, -model.com[0, i], dtype) for i in range(3)), two)
        for i in range(3):
            out[:, 0, i] = roots[:, i] + r[i]
    placed = {0}
    for j in range(model.nj):
        assert model.rb0[j] in placed and model.rb1[j] not in placed, "joints are not in top-down order"
        placed.add(model.rb1[j])
        par = out[:, model.rb0[j]]
        q0 = _q(par[:, 3:])
        F = tuple(np.full(B, model.frame[j, i], dtype) for i in range(4))
        if enhanced and j in TIP_JOINTS:      # handtrack.h:417-420, acos and sin in double, the literals 3.14159f and 3.14f
            cs = dot3(qzdir(_q(out[:, j - 1, 3:]), two), qzdir(_q(out[:, j, 3:]), two))
            cs = np.minimum(np.maximum(cs, zero), one)
            deg = (np.arccos(cs.astype(np.float64)) * 180.0 / float(np.float32(3.14159)) / 2.0).astype(dtype)
            c[:, j, 0] = np.sin((((deg * T(3.14)) / T(180.0)) / T(2.0)).astype(np.float64)).astype(dtype)
        cx, cy, cz = c[:, j, 0], c[:, j, 1], c[:, j, 2]
        q1 = _child(q0, F, swapped[j], cx, cy, cz, T)
        if enhanced and j in KNUCKLE_JOINTS:      # :434-440: not "up" on the built pose: y locked at 0, one rebuild
            up = dot3(qydir(_q(out[:, 1, 3:]), two), qydir(q1, two)).astype(np.float64) > COS40
            c[:, j, 1] = np.where(up, cy, zero)
            q2 = _child(q0, F, swapped[j], cx, c[:, j, 1], cz, T)
            q1 = tuple(np.where(up, a, b) for a, b in zip(q1, q2))
        r0 = qrot(q0, tuple(np.full(B, model.p0[j, i], dtype) for i in range(3)), two)
        r1 = qrot(q1, tuple(np.full(B, model.p1[j, i], dtype) for i in range(3)), two)
        for i in range(3):
            out[:, model.rb1[j], i] = (par[:, i] + r0[i]) - r1[i]
        for i in range(4):
            out[:, model.rb1[j], 3 + i] = q1[i]
    if com_poses:
        for b in range(model.nb):
            r = qrot(_q(out[:, b, 3:]), tuple(np.full(B, model.com[b, i], dtype) for i in range(3)), two)
            for i in range(3):
                out[:, b, i] = out[:, b, i] + r[i]
    return (out, c) if enhanced else out


# ---- definition 6: the sampler -----------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _mix(x):
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def uniform24(seed, sample, joint, axis):
    """the 24-bit integer k of u = k * 2^-24 for (seed, sample, joint, axis), in Python integers"""
    h = _mix(_mix((seed ^ (sample * 0x9E3779B97F4A7C15)) & _M64) ^ (((joint * 3 + axis + 1) * 0xD6E8FEB86659FD93) & _M64))
    return h >> 40


def sample_coords(model, B, seed, first_index, spread, dtype=np.float32, lim=None):
    T = np.dtype(dtype).type
    lo, hi = (lim or limits(model))[:2]
    c = np.zeros((B, model.nj, 3), dtype)
    for j in range(model.nj):
        for a in range(3):
            l, h = T(lo[j, a]), T(hi[j, a])
            if l == h:
                c[:, j, a] = l
                continue
            u = np.array([uniform24(seed, first_index + i, j, a) for i in range(B)], np.float64).astype(dtype) * T(2.0 ** -24)
            c[:, j, a] = (l + h) * T(0.5) + ((u - T(0.5)) * (h - l)) * T(spread)
    return c


def sample_poses(model, roots, seed, first_index, spread, dtype=np.float32, com_poses=False, enhanced=False):
    """(poses [B,nb,7], coords [B,nj,3]) of ht_sample_poses"""
    c = sample_coords(model, len(roots), seed, first_index, spread, dtype)
    if enhanced:
        return pose(model, roots, c, dtype, com_poses, enhanced=True)
    return pose(model, roots, c, dtype, com_poses), c


# ---- the reference's rows from the coordinates (physics.h:367-391), for the comparison with the oracle ----------------------------
def row_targetspins(model, c):
    """targetspin of every row ConstrainAngularRangeW emits, in its order, predicted from float32 coordinates c [nj,3] and the model table's limits.
    Returns (spins, kinds): kind 'lock' for an equality row, 'side' for a one-sided one."""
    f = np.float32
    dt, bias = model.deltaT, model.biasfactorjoint
    spins, kinds = [], []
    for j in range(model.nj):
        lmin, lmax = model.rmin[j].astype(f), model.rmax[j].astype(f)
        jmin, jmax = (lmin * f(3.14)) / f(180.0), (lmax * f(3.14)) / f(180.0)
        if jmin[0] == 0 and jmax[0] == 0 and jmin[2] < jmax[2]:
            lmin, lmax = np.array([lmin[2], lmin[1], 0], f), np.array([lmax[2], lmax[1], 0], f)
            jmin, jmax = (lmin * f(3.14)) / f(180.0), (lmax * f(3.14)) / f(180.0)

        def two_sided(comp, a):      # the sums are formed in double and rounded once (the reference's sin is the double overload)
            spins.append(f(2 * (-float(comp) + math.sin(float(jmin[a] / f(2)))) / float(dt))); kinds.append("side")
            spins.append(f(2 * (float(comp) - math.sin(float(jmax[a] / f(2)))) / float(dt))); kinds.append("side")
        cx, cy, cz = f(c[j, 0]), f(c[j, 1]), f(c[j, 2])
        if jmax[0] == jmin[0]:
            spins.append(f(2 * (-float(cx) + math.sin(float(jmin[0] / f(2)))) / float(dt))); kinds.append("lock")
        elif jmax[0] - jmin[0] < f(360.0) * f(3.14) / f(180.0):
            two_sided(cx, 0)
        if jmax[1] == jmin[1]:
            spins.append(bias * f(2) * (-cy + jmin[1]) / dt); kinds.append("lock")
        else:
            two_sided(cy, 1)
        if jmin[2] == jmax[2]:
            spins.append(bias * f(2) * -cz / dt); kinds.append("lock")
        else:
            two_sided(cz, 2)
    return np.array(spins, f), kinds
