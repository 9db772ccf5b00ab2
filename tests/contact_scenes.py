"""Seeded contact scenes for the narrow phase (csrc/ht_gjk.hip against oracle/ho_gjk.c against the reference's answers in tests/golden/contact_fuzz_*.htfx).

NumPy only: neither a GPU nor the oracle is needed.  Every draw comes from splitmix64 (the generator oracle/ref_harness.cpp uses for its own cases), every pose is built
with +, -, *, / and sqrt on IEEE doubles and rounded once to float32, so the scenes are the same on every machine; the fixtures hold their digests.

A pair scene is 16 numbers (body a < b, pose of a, pose of b: position 3, quaternion xyzw 4); every other body is parked 10 m apart (pair_states).  A whole scene is a
pose [nb, 7] per body.  Every family function returns its scenes in that compact form; states(family) expands them to [n, nb, 13] with zero momenta.

Families (tests/test_contact_scenes_ref.py asserts what each is there for):
  a   stock hand, one pair: random poses at centre distances 0 .. 4 cm, and planes / edges / vertices of b opposed to planes / edges of a at gaps around the cut-off
  b   stock hand, one pair at two neighbouring float32 centre distances between which the contact appears (the distances are found by bisection when the fixture is made)
  c   stock hand scaled by 10, one deeply overlapping pair: the large polytopes
  d17 / d26   a subset of bodies within 1 mm of one point, chosen so that the broad phase keeps an exact number of candidate pairs
  e17 / e26   every body drawn about one point
  f   the box and the prism of the 3-body chain scaled by 10, planes opposed with small tilts: contact patches of more than one sample
"""
import hashlib
import math
import os

import numpy as np

import htfx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = {"hand17": os.path.join(GOLDEN, "model_hand17.htfx"), "hand26": os.path.join(GOLDEN, "model_hand26.htfx"), "chain3": os.path.join(GOLDEN, "model_chain3.htfx")}
# family -> (model, scale, pairs taken off the ignore lists, kind)
FAMILIES = {"a": ("hand17", 1.0, (), "pair"), "b": ("hand17", 1.0, (), "pair"), "c": ("hand17", 10.0, (), "pair"), "f": ("chain3", 10.0, ((0, 1),), "pair"),
            "d17": ("hand17", 1.0, (), "whole"), "d26": ("hand26", 1.0, (), "whole"), "e17": ("hand17", 1.0, (), "whole"), "e26": ("hand26", 1.0, (), "whole")}
SEEDS = {"a": 0xA11CE, "b": 0xB15EC7, "c": 0xC04B, "d17": 0xD17, "d26": 0xD26, "e17": 0xE17, "e26": 0xE26, "f": 0xF00D}
GAPS_MM = (-2.0, -0.5, 0.0, 0.5, 2.0, 3.5, 4.0)
CANDIDATES = {"d17": (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 91), "d26": (32, 33, 64, 65, 127, 128, 129, 244)}
SIGMAS_MM = {"e17": (10.0,) * 16 + (30.0,) * 16 + (60.0,) * 16, "e26": (10.0,) * 8 + (5.0,) * 8}
N_CUTOFF = 120
CENTRE = (0.0, 0.0, 0.4)
TAN_2P5_DEG = 0.04366094290851206      # tan(2.5 degrees): the half-angle tangent of a 5 degree tilt
_M64 = (1 << 64) - 1


def splitmix64_at(seed, i):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class Rand:
    """counter-based draws from splitmix64; nothing but exact double arithmetic and sqrt"""

    def __init__(self, seed):
        self.seed, self.i = seed, 0

    def u(self):
        v = (splitmix64_at(self.seed, self.i) >> 11) * (1.0 / 9007199254740992.0)
        self.i += 1
        return v

    def below(self, n):
        return min(int(self.u() * n), n - 1)

    def normal(self):
        """Irwin-Hall: twelve uniforms, variance 1 (no log, no cos: the same bits everywhere)"""
        return sum(self.u() for _ in range(12)) - 6.0

    def quat(self):
        while True:
            q = [self.u() - 0.5 for _ in range(4)]
            n = _norm(q)
            if n > 1e-3:
                return tuple(x / n for x in q)

    def unit(self):
        while True:
            d = [self.u() - 0.5 for _ in range(3)]
            n = _norm(d)
            if 1e-3 < n <= 0.5:
                return tuple(x / n for x in d)


# ---- a few lines of vector algebra on tuples of Python floats -------------------------------------------------------------------------
def _norm(v):
    s = 0.0
    for x in v:
        s += x * x
    return math.sqrt(s)


def _unit(v):
    n = _norm(v)
    return tuple(x / n for x in v)


def _add(a, b): return tuple(x + y for x, y in zip(a, b))
def _sub(a, b): return tuple(x - y for x, y in zip(a, b))
def _mul(a, s): return tuple(x * s for x in a)
def _dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _qmul(a, b):
    return (a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
            a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2])


def _qrot(q, v):
    t = _mul(_cross(q[:3], v), 2.0)
    return _add(_add(v, _mul(t, q[3])), _cross(q[:3], t))


def _orth(v):
    a = (1.0, 0.0, 0.0) if abs(v[0]) < 0.6 else (0.0, 1.0, 0.0)
    return _unit(_cross(v, a))


def _from_to(u, v):
    """the rotation that takes unit vector u to unit vector v"""
    c = _dot(u, v)
    if c < -0.999999:
        return _orth(u) + (0.0,)
    return _unit(_cross(u, v) + (1.0 + c,))


def _about(axis, x, y):
    """rotation about a unit axis by the angle whose half has sine : cosine = x : y"""
    return _unit(_mul(axis, x) + (y,))


# ---- models -----------------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, name, scale=1.0, clear=()):
        m = htfx.load(MODELS[name])
        self.name, self.scale, self.nb = name, float(scale), int(m["nb"][0])
        s = np.float32(scale)
        self.verts = [m["b%d/verts" % b][:m["nverts"][b]] * s for b in range(self.nb)]      # Shape scaling multiplies in float32 (physmodel.h:196-202)
        self.tris = [m["b%d/tris" % b] for b in range(self.nb)]
        self.radius = (m["body_f"][:, 2] * s).astype(np.float32)
        self.collide = m["body_collide"].copy()
        self.ignore = m["ignore"].copy()
        for i, j in clear:
            self.ignore[i, j] = self.ignore[j, i] = 0
        self.pairs = [(i, j) for i in range(self.nb) for j in range(i + 1, self.nb) if not self.ignore[i, j] and (self.collide[i] & self.collide[j] & 2)]
        self._feat = {}

    def features(self, b):
        """(centroid, faces [(outward unit normal, centre)], edges [(outward unit direction, midpoint)], vertices [(outward unit direction, vertex)]) in the body's frame"""
        if b in self._feat:
            return self._feat[b]
        V = [tuple(float(x) for x in v) for v in self.verts[b]]
        c = _mul(tuple(sum(v[k] for v in V) for k in range(3)), 1.0 / len(V))
        faces, edges, seen = [], [], set()
        for t in self.tris[b]:
            p = [V[int(k)] for k in t]
            n = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
            if _norm(n) < 1e-12:
                continue
            n = _unit(n)
            mid = _mul(_add(_add(p[0], p[1]), p[2]), 1.0 / 3.0)
            if _dot(n, _sub(mid, c)) < 0:
                n = _mul(n, -1.0)
            faces.append((n, mid))
            for k in range(3):
                e = (min(int(t[k]), int(t[(k + 1) % 3])), max(int(t[k]), int(t[(k + 1) % 3])))
                if e not in seen and e[0] != e[1]:
                    seen.add(e)
                    em = _mul(_add(V[e[0]], V[e[1]]), 0.5)
                    if _norm(_sub(em, c)) > 1e-9:
                        edges.append((_unit(_sub(em, c)), em))
        used = sorted({int(k) for t in self.tris[b] for k in t})
        verts = [(_unit(_sub(V[k], c)), V[k]) for k in used if _norm(_sub(V[k], c)) > 1e-9]
        self._feat[b] = (c, faces, edges, verts)
        return self._feat[b]


_models = {}


def model_of(family):
    name, scale, clear, _ = FAMILIES[family]
    key = (name, scale, clear)
    if key not in _models:
        _models[key] = Model(name, scale, clear)
    return _models[key]


# ---- scene pieces -------------------------------------------------------------------------------------------------------------------------
def _case(a, b, pa, qa, pb, qb):
    return np.array([a, b] + list(pa) + list(qa) + list(pb) + list(qb), np.float64).astype(np.float32)


def _opposed(r, M, a, b, kind_a, kind_b, gap, tilt_scale=1.0):
    """b posed so that one of its features (kind 0 face, 1 edge, 2 vertex) looks at a feature of a across `gap` metres, spun about the line between them and tilted"""
    qa = r.quat()
    fa = M.features(a)[1 + kind_a]; fb = M.features(b)[1 + kind_b]
    da, pa_l = fa[r.below(len(fa))]; db, pb_l = fb[r.below(len(fb))]
    da_w = _qrot(qa, da); pa_w = _add(CENTRE, _qrot(qa, pa_l))
    q = _from_to(db, _mul(da_w, -1.0))
    sx, sy = r.u() - 0.5, r.u() - 0.5
    if abs(sx) + abs(sy) < 1e-3:
        sy = 1.0
    q = _qmul(_about(da_w, sx, sy), q)
    t = _orth(da_w)
    tx, ty = r.u() - 0.5, r.u() - 0.5
    axis = _unit(_add(_mul(t, tx), _mul(_cross(da_w, t), ty))) if abs(tx) + abs(ty) > 1e-3 else t
    q = _qmul(_about(axis, r.u() * tilt_scale * TAN_2P5_DEG, 1.0), q)
    pb = _sub(_add(pa_w, _mul(da_w, gap)), _qrot(q, pb_l))
    return _case(a, b, CENTRE, qa, pb, q)


def family_a():
    """1200 pair scenes of the stock hand"""
    M, r, out = model_of("a"), Rand(SEEDS["a"]), []
    for k in range(640):
        a, b = M.pairs[r.below(len(M.pairs))]
        qa, qb, d, dist = r.quat(), r.quat(), r.unit(), r.u() * 0.04
        if k & 1:
            dist *= r.u()      # every other scene leans towards the centre: deeper overlaps
        out.append(_case(a, b, CENTRE, qa, _add(CENTRE, _mul(d, dist)), qb))
    for kinds, n in (((0, 0), 40), ((1, 1), 20), ((0, 2), 20)):      # plane on plane, edge on edge, vertex of b on plane of a
        for gap in GAPS_MM:
            for _ in range(n):
                a, b = M.pairs[r.below(len(M.pairs))]
                out.append(_opposed(r, M, a, b, kinds[0], kinds[1], gap * 1e-3))
    return np.stack(out)


def cutoff_draws():
    """family b before the distances are known: [N_CUTOFF, 16] with b at the centre of a, and the unit directions [N_CUTOFF, 3] (float32) it moves along.
    Every fifth draw turns both bodies so that their farthest vertices face each other: there the contact ends at the broad phase's sphere test."""
    M, r, cases, dirs = model_of("b"), Rand(SEEDS["b"]), [], []
    for k in range(N_CUTOFF):
        a, b = M.pairs[r.below(len(M.pairs))]
        d = r.unit()
        qa, qb = r.quat(), r.quat()
        if k % 5 == 4:
            far = []
            for body in (a, b):
                V = M.verts[body].astype(np.float64)
                far.append(_unit(tuple(V[int(np.argmax((V * V).sum(1)))])))
            qa, qb = _from_to(far[0], d), _from_to(far[1], _mul(d, -1.0))
        cases.append(_case(a, b, (0.0, 0.0, 0.0), qa, (0.0, 0.0, 0.0), qb))
        dirs.append(np.array(d, np.float64).astype(np.float32))
    return np.stack(cases), np.stack(dirs)


def cutoff_case(case, direction, dist):
    c = case.copy()
    c[9:12] = direction * np.float32(dist)      # float32 product: neighbouring distances give neighbouring positions
    return c


def bisect_cutoffs(count):
    """The fixture maker's half of family b: count(case16) -> contacts of the scene.  Returns [N_CUTOFF, 2] float32: neighbouring distances, contact at the first, none at the second
    (0, 0 where a draw has no such place below 0.3 m)."""
    cases, dirs = cutoff_draws()
    out = np.zeros((N_CUTOFF, 2), np.float32)
    for k in range(N_CUTOFF):
        lo, hi = np.float32(0.0), np.float32(0.3)
        if count(cutoff_case(cases[k], dirs[k], lo)) < 1 or count(cutoff_case(cases[k], dirs[k], hi)) > 0:
            continue
        while np.nextafter(lo, np.float32(1.0)) < hi:
            mid = np.float32((np.float64(lo) + np.float64(hi)) * 0.5)
            if count(cutoff_case(cases[k], dirs[k], mid)) >= 1:
                lo = mid
            else:
                hi = mid
        out[k] = (lo, hi)
    return out


def family_b(distances):
    """2 x N_CUTOFF pair scenes: draw k at distances[k, 0] (scene 2k) and distances[k, 1] (scene 2k + 1)"""
    cases, dirs = cutoff_draws()
    return np.stack([cutoff_case(cases[k], dirs[k], distances[k, s]) for k in range(N_CUTOFF) for s in (0, 1)])


def family_c():
    """300 deeply overlapping pairs of the stock hand scaled by 10 (bones of 20 .. 90 cm, centres at most 5 cm apart, at most 1 cm in every other scene).  About one such
    draw in a thousand grows a polytope beyond 64 triangles; the family's seed is the one of 80 tried whose 300 scenes hold two (found with the restatement's ho_epa_stats,
    asserted in tests/test_contact_scenes_ref.py)."""
    M, r, out = model_of("c"), Rand(SEEDS["c"]), []
    for k in range(300):
        a, b = M.pairs[r.below(len(M.pairs))]
        qa, qb, d, dist = r.quat(), r.quat(), r.unit(), r.u() * (0.01 if k & 1 else 0.05)
        out.append(_case(a, b, CENTRE, qa, _add(CENTRE, _mul(d, dist)), qb))
    return np.stack(out)


def family_f():
    """600 scenes of the chain's box (0) and prism (1) at scale 10, a plane of one opposed to a plane of the other; tilts lean towards zero (the square of a uniform draw)
    because a patch takes extra samples only when the tilt is below the 2 degrees the reference rolls the shape by (gjk.h:626-641)"""
    M, r, out = model_of("f"), Rand(SEEDS["f"]), []
    for k in range(600):
        out.append(_opposed(r, M, 0, 1, 0, 0, GAPS_MM[k % len(GAPS_MM)] * 1e-3, tilt_scale=r.u()))
    return np.stack(out)


def parked(nb):
    p = np.zeros((nb, 7), np.float32)
    p[:, 6] = 1.0
    p[:, 0] = 10.0 * (1 + np.arange(nb))
    return p


def _cluster(r, M, bodies, sigma):
    p = parked(M.nb)
    for b in bodies:
        p[b, :3] = np.array([CENTRE[k] + sigma * r.normal() for k in range(3)], np.float64).astype(np.float32)
        p[b, 3:7] = np.array(r.quat(), np.float64).astype(np.float32)
    return p


def candidates(M, pose):
    """the broad phase restated (physics.h:453-457): collide flags, |d| > r_i + r_j in float32 with the baked radii, ignore lists; the pairs in the reference's order"""
    out = []
    P = pose[:, :3].astype(np.float32)
    for i in range(M.nb):
        for j in range(i + 1, M.nb):
            if not (M.collide[i] & M.collide[j] & 2):
                continue
            d = P[j] - P[i]
            if np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])) > np.float32(M.radius[i] + M.radius[j]):
                continue
            if M.ignore[i, j]:
                continue
            out.append((i, j))
    return out


def _subset_with(r, M, want):
    """bodies among which exactly `want` pairs are neither ignored nor without the collide flag"""
    free = np.zeros((M.nb, M.nb), np.int64)
    for i, j in M.pairs:
        free[i, j] = 1
    if want == 0:
        return []
    for _ in range(200000):
        size = 2 + r.below(M.nb - 1)
        order = sorted(range(M.nb), key=lambda b: splitmix64_at(r.seed ^ 0x5EED, r.i * 64 + b))
        r.i += 1
        s = sorted(order[:size])
        if int(free[np.ix_(s, s)].sum()) == want:
            return s
    raise AssertionError("no subset of %s with %d candidate pairs" % (M.name, want))


def family_d(which):
    """one scene per candidate count of CANDIDATES[which]: the chosen bodies within about 1 mm of one point, the rest parked.  Returns (poses, counts)."""
    M, r, out = model_of(which), Rand(SEEDS[which]), []
    for want in CANDIDATES[which]:
        pose = _cluster(r, M, _subset_with(r, M, want), 1e-3)
        assert len(candidates(M, pose)) == want, (which, want, len(candidates(M, pose)))
        out.append(pose)
    return np.stack(out), np.array(CANDIDATES[which], np.int32)


def family_e(which):
    """every body about one point, standard deviation SIGMAS_MM[which][k] per axis.  Returns (poses, sigmas in mm)."""
    M, r = model_of(which), Rand(SEEDS[which])
    return np.stack([_cluster(r, M, range(M.nb), s * 1e-3) for s in SIGMAS_MM[which]]), np.array(SIGMAS_MM[which], np.float32)


# ---- what the tests take ---------------------------------------------------------------------------------------------------------------
def pair_states(cases, nb):
    s = np.zeros((len(cases), nb, 13), np.float32)
    s[:, :, :7] = parked(nb)
    for k, c in enumerate(cases):
        s[k, int(c[0]), :7] = c[2:9]
        s[k, int(c[1]), :7] = c[9:16]
    return s


def pose_states(poses):
    s = np.zeros(poses.shape[:2] + (13,), np.float32)
    s[:, :, :7] = poses
    return s


def fixture_path(family):
    return os.path.join(GOLDEN, "contact_fuzz_%s.htfx" % family)


def compact(family, distances=None):
    """the family's scenes in compact form: [n, 16] for a pair family, [n, nb, 7] for a whole-scene family"""
    if family == "b":
        if distances is None:
            distances = htfx.load(fixture_path("b"))["distances"]
        return family_b(distances)
    if family in ("d17", "d26"):
        return family_d(family)[0]
    if family in ("e17", "e26"):
        return family_e(family)[0]
    return {"a": family_a, "c": family_c, "f": family_f}[family]()


def states(family, scenes=None):
    """[n, nb, 13], zero momenta"""
    scenes = compact(family) if scenes is None else scenes
    return pair_states(scenes, model_of(family).nb) if FAMILIES[family][3] == "pair" else pose_states(scenes)


def digest(states_):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(states_, np.float32).tobytes()).hexdigest().encode(), np.uint8).copy()
