"""Inputs shared by tests/test_cloud_scenes_ref.py and tests/test_gpu_cloud_fuzz.py: model variants baked at test time from tests/golden/model_*.htfx, body states and
point clouds that reach the branches of csrc/ht_cloud.hip which natural frames leave dead, the point counts at the chunk edges, and phase A's
candidate rule in numpy.  Pure numpy, fixed seeds.  Test infrastructure only."""
import os

import numpy as np

import htfx

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CH, PAIR_WIN = 128, 1024      # csrc/ht_cloud.hip: points per chunk, (point, body) pairs per window of phase B
COUNTS = (0, 1, 2, 127, 128, 129, 255, 256, 257, 383, 384, 385, 513)
# the counts over the slots of two batches (B = 8 and 5), not sorted
BATCHES = ((257, 0, 513, 1, 128, 385, 2, 255), (129, 384, 127, 383, 256))
NBASE = 513

# hand17 with leading subsets of each body's face planes.  Every count the face scan treats differently: the largest (92), one under it, 64 / 49 / 48 and 17 / 16 / 15 either
# side of the sixteen-face rounds, 5 / 4 / 3 / 2 / 1 around the four lanes of a pair.  The last body: within 4 of the largest in mixed17, 5 in mixed17_short_last.
MIXED17 = (92, 48, 91, 17, 5, 64, 16, 3, 49, 15, 4, 33, 2, 90, 7, 1, 89)
MIXED17_SHORT_LAST = MIXED17[:-1] + (5,)
TWINS = ((4, 13), (12, 15))      # (original, bitwise copy): 4 | 13 sit in the two halves of phase A (hb = 9), 12 | 15 both in the upper half


def stock_path(name):
    return os.path.join(GOLDEN, "model_%s.htfx" % name)


def _cut(m, counts):
    m = dict(m)
    for b, k in enumerate(counts):
        m["b%d/planes" % b] = m["b%d/planes" % b][:k].copy()
        m["b%d/tris" % b] = m["b%d/tris" % b][:k].copy()
    m["nplanes"] = np.array(counts, np.int32)
    return m


def _twins(m):
    m = dict(m); bf = m["body_f"].copy()
    for a, c in TWINS:
        for k in ("verts", "sdverts", "planes", "tris"):
            m["b%d/%s" % (c, k)] = m["b%d/%s" % (a, k)].copy()
        bf[c, 2:4] = bf[a, 2:4]      # radius, radius_inner
        m["nverts"] = m["nverts"].copy(); m["nverts"][c] = m["nverts"][a]
    m["body_f"] = bf
    return m


def _fat_twins(m):
    """the twins with their inner spheres blown up to the outer ones: no face plane then lies nearer than the inner-sphere plane, so what the inner-sphere walk (phase A)
    picked stays the answer, and its tie rule shows in the row's body"""
    m = _twins(m); bf = m["body_f"].copy()
    for a, c in TWINS:
        bf[a, 3] = bf[c, 3] = bf[a, 2]
    m["body_f"] = bf
    return m


MIRROR_BODY = 5


def _mirror(m):
    """hand17 whose body MIRROR_BODY holds, beside each face plane and each vertex, its image under x -> -x: for a point with local x = 0 (a direction with x = 0) the two
    give the same value bit for bit, yet they are different planes (vertices), so the winner shows in the row.  Faces in blocks of [3 planes][their 3 images]: the two of a
    pair lie three faces apart, on different lanes of the four that share a (point, body) pair.  Vertices in blocks of [15][their 15 images]: fifteen apart, on neighbouring
    lanes of the sixteen that share an item, the lower index often not on the lane that ends up with the result."""
    m = dict(m); k = "b%d/" % MIRROR_BODY
    flip = np.array([-1, 1, 1, 1], F)

    def blocks(a, run, sign):
        out = []
        nblk = len(a) // (2 * run)
        for i in range(nblk):
            out += [a[i * run:(i + 1) * run], a[i * run:(i + 1) * run] * sign]
        out.append(a[nblk * run:nblk * run + len(a) - 2 * run * nblk])
        return np.ascontiguousarray(np.concatenate(out), a.dtype)
    m[k + "planes"] = blocks(m[k + "planes"], 3, flip)
    m[k + "verts"] = blocks(m[k + "verts"], 15, flip[:3])
    return m


VARIANTS = {
    "fat_twins17": ("hand17", _fat_twins), "mirror17": ("hand17", _mirror),
    "hand17": ("hand17", None), "hand26": ("hand26", None), "chain3": ("chain3", None),
    "mixed17": ("hand17", lambda m: _cut(m, MIXED17)), "mixed17_short_last": ("hand17", lambda m: _cut(m, MIXED17_SHORT_LAST)),
    "uniform61": ("chain3", lambda m: _cut(m, (61,) * 3)), "uniform16": ("chain3", lambda m: _cut(m, (16,) * 3)),
    "twins17": ("hand17", _twins),
}


def variant_path(name, tmpdir):
    """the baked file of a variant: a stock model's own file, or a copy with the edit applied, written into tmpdir (context and oracle load the same file)"""
    base, edit = VARIANTS[name]
    if edit is None:
        return stock_path(base)
    path = os.path.join(str(tmpdir), "model_%s.htfx" % name)
    if not os.path.exists(path):
        htfx.save(path, edit(htfx.load(stock_path(base))))
    return path


class Model:
    """what the scenes need of a baked file"""

    def __init__(self, path):
        m = htfx.load(path)
        self.path, self.nb = path, int(m["nb"][0])
        self.radius, self.rinner = m["body_f"][:, 2].copy(), m["body_f"][:, 3].copy()
        self.rest = m["rest_state"].astype(F)
        self.verts = [m["b%d/verts" % b] for b in range(self.nb)]
        self.tris = [m["b%d/tris" % b] for b in range(self.nb)]
        self.planes = [m["b%d/planes" % b] for b in range(self.nb)]
        self.nplanes = [len(p) for p in self.planes]
        assert m["nplanes"].tolist() == self.nplanes and m["nverts"].tolist() == [len(v) for v in self.verts]


# ---- states [nb,13]: momenta zero, unit quaternions ------------------------------------------------------------------------------------------------------------------
def _quats(rng, n):
    q = rng.standard_normal((n, 4)); return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def rest_state(model, z=0.45):
    s = np.zeros((model.nb, 13), F); s[:, :7] = model.rest[:, :7]
    s[:, 2] += F(z) - s[0, 2]
    return s


def truth_state(k, name="hand17"):
    import kpfit_inputs as ki
    P = ki.truths(name)
    return ki.states_of(P[k % len(P)][None])[0]


RING_P = np.array([0.02, -0.01, 0.45], F)


def ring_state(model, seed=11, P=RING_P):
    """body b at P + dir_b (radius_b - 2 mm), any orientation: every outer sphere covers the 2 mm ball about P, so every body is a candidate of every point in it"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((model.nb, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    s = np.zeros((model.nb, 13), F)
    s[:, :3] = (P.astype(np.float64) + d * (model.radius.astype(np.float64) - 0.002)[:, None]).astype(F)
    s[:, 3:7] = _quats(rng, model.nb)
    return s


def twins_state(state):
    """each copied body at exactly the pose of its original"""
    s = state.copy()
    for a, c in TWINS:
        s[c] = s[a]
    return s


def _qrot(q, v):
    x, y, z, w = (float(c) for c in q)
    m = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - z * w), 2 * (z * x + y * w)], [2 * (x * y + z * w), w * w - x * x + y * y - z * z, 2 * (y * z - x * w)],
                  [2 * (z * x - y * w), 2 * (y * z + x * w), w * w - x * x - y * y + z * z]])
    return np.asarray(v, np.float64) @ m.T


def body_in_camera(state, cam, body, where):
    """`state` with one body moved to the point `where` of the camera's own space (z < 0: behind the camera; x / z large: outside the image)"""
    s = state.copy()
    s[body, :3] = (cam[5:8].astype(np.float64) + _qrot(cam[8:12], where)).astype(F)
    return s


# ---- cameras and the rendered frame ------------------------------------------------------------------------------------------------------------------------------------
def camera(away=True):
    """a 64x64 tile's camera [12]; away: posed well off the origin, so that rays from it and rays from zero face different sides of the bodies"""
    cam = np.zeros(12, F); cam[0] = cam[1] = 90.0; cam[2] = cam[3] = 31.5; cam[4] = 0.001; cam[11] = 1.0
    if away:
        q = np.array([0.05, -0.32, 0.02, 0.94]); cam[8:12] = (q / np.linalg.norm(q)).astype(F); cam[5:8] = (0.33, -0.04, 0.06)
    return cam


def surface_samples(model, state):
    """points on the posed hulls: every vertex and ten points of every hull triangle"""
    w = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5], [1 / 3, 1 / 3, 1 / 3], [.6, .2, .2], [.2, .6, .2], [.2, .2, .6]])
    out = []
    for b in range(model.nb):
        v = model.verts[b].astype(np.float64); t = model.tris[b]
        t = t[(t < len(v)).all(axis=1) & (t >= 0).all(axis=1)]
        loc = np.concatenate([v, np.einsum("kc,tcd->tkd", w, v[t]).reshape(-1, 3)])
        out.append(_qrot(state[b, 3:7], loc) + state[b, :3].astype(np.float64))
    return np.concatenate(out)


def render(model, state, cam, w=64, h=64):
    """z-buffer splat of the surface samples as `cam` sees them -> (depth u16[h,w], the frame's cloud [n,3] in tracking space, raster order)"""
    p = surface_samples(model, state)
    qc = np.array([-cam[8], -cam[9], -cam[10], cam[11]], np.float64)
    c = _qrot(qc, p - cam[5:8].astype(np.float64))
    c = c[c[:, 2] > 0.05]
    x = np.floor(c[:, 0] / c[:, 2] * cam[0] + cam[2] + 0.5).astype(np.int64); y = np.floor(c[:, 1] / c[:, 2] * cam[1] + cam[3] + 0.5).astype(np.int64)
    ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    d = np.full(h * w, 65535, np.int64)
    np.minimum.at(d, (y * w + x)[ok], np.round(c[ok, 2] / cam[4]).astype(np.int64))
    d[d == 65535] = 0
    depth = d.astype(np.uint16).reshape(h, w)
    yy, xx = np.nonzero(depth)
    z = depth[yy, xx].astype(np.float64) * float(cam[4])
    pc = np.stack([(xx - float(cam[2])) / float(cam[0]) * z, (yy - float(cam[3])) / float(cam[1]) * z, z], axis=1)
    return depth, (_qrot(cam[8:12], pc) + cam[5:8].astype(np.float64)).astype(F)


# ---- clouds ------------------------------------------------------------------------------------------------------------------------------------------------------------
def ball(P, radius, n, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(P, np.float64) + d * (radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3))).astype(F)


def shell_behind(model, state, origin, n, seed):
    """points a little behind the bodies as seen from `origin`: they face away from it, and the ray to them passes through their body (a hit) or beside it (a miss)"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, model.nb, n)
    c = state[b, :3].astype(np.float64)
    away = c - np.asarray(origin, np.float64); away /= np.linalg.norm(away, axis=1, keepdims=True)
    side = rng.standard_normal((n, 3)); side -= (side * away).sum(1, keepdims=True) * away; side /= np.linalg.norm(side, axis=1, keepdims=True)
    r = model.radius[b].astype(np.float64)[:, None]
    return (c + away * r * rng.uniform(0.3, 1.6, (n, 1)) + side * r * rng.uniform(0.0, 1.3, (n, 1))).astype(F)


def inside(model, state, n, seed):
    """points well inside bodies (dmin < 0)"""
    rng = np.random.default_rng(seed)
    b = np.arange(n) % model.nb
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (state[b, :3].astype(np.float64) + d * (0.4 * model.rinner[b].astype(np.float64) * rng.uniform(0.05, 1, n))[:, None]).astype(F)


def body_probes(model, state, per_body, seed):
    """around every body in turn: points just outside its own faces (1 mm to 6 mm above a face, over the face's own triangle)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(per_body):
        for b in range(model.nb):
            f = int(rng.integers(0, model.nplanes[b]))
            t = model.tris[b][f]; v = model.verts[b].astype(np.float64)
            w = rng.dirichlet((2, 2, 2))
            loc = w @ v[t] + model.planes[b][f, :3].astype(np.float64) * rng.uniform(0.001, 0.006)
            out.append(_qrot(state[b, 3:7], loc) + state[b, :3].astype(np.float64))
    return np.array(out).astype(F)


def mirror_plane_points(model, state, n, seed):
    """points with exactly the x of body MIRROR_BODY's position (its orientation is the identity: local x = 0), around it in y and z"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, n); r = model.radius[MIRROR_BODY] * rng.uniform(0.2, 1.4, n)
    p = np.tile(state[MIRROR_BODY, :3], (n, 1)).astype(F)
    p[:, 1] += (r * np.cos(a)).astype(F); p[:, 2] += (r * np.sin(a)).astype(F)
    return p


FAR_POINT = np.array([3.0, -4.0, 8.6602540], F)      # 10 m away


def natural_cloud(model, state, cam, seed=3, n=NBASE):
    """the frame's own cloud first, then the away-facing shell, points inside bodies, a point exactly at a body's position and one 10 m away, interleaved so that every
    cut of the cloud holds some of each; n points"""
    depth, pts = render(model, state, cam)
    parts = [pts, shell_behind(model, state, (0, 0, 0), n // 3, seed), shell_behind(model, state, cam[5:8], n // 3, seed + 1), inside(model, state, n // 8, seed + 2),
             body_probes(model, state, 4, seed + 3)]
    mixed = []
    it = [iter(p) for p in parts]
    while len(mixed) < n + 8:
        got = False
        for j, i in enumerate(it):
            for _ in range(3 if j == 0 else 1):
                v = next(i, None)
                if v is not None:
                    mixed.append(v); got = True
        assert got, "the parts hold fewer than %d points" % n
    mixed = np.array(mixed[:n], F)
    mixed[0] = state[model.nb // 2, :3]; mixed[1] = FAR_POINT; mixed[CH - 1] = state[0, :3]; mixed[CH] = state[model.nb - 1, :3]
    return depth, np.ascontiguousarray(mixed)


def plane_clouds(cloud, seed=5):
    """for the boundary planes' strict `> 0`: every point twice in a row; and runs of points on one ray through the origin (exact multiples by powers of two)"""
    dup = np.repeat(cloud[:(NBASE + 1) // 2], 2, axis=0)[:NBASE]
    k = np.array([1.0, 2.0, 0.5, 1.0], F)
    col = (cloud[:(NBASE + 3) // 4, None, :] * k[None, :, None]).reshape(-1, 3)[:NBASE]
    return np.ascontiguousarray(dup), np.ascontiguousarray(col)


def cuts(cloud, batch):
    return [np.ascontiguousarray(cloud[:n]) for n in batch]


# ---- phase A's candidate rule -------------------------------------------------------------------------------------------------------------------------------------------
def candidates(model, state, pts):
    """bool [n,nb]: body b is a candidate of point v when !(|v - pos_b| - radius_b > min_b(|v - pos_b| - rinner_b)) (closest_chunk, phase A; float32, the device's bound is
    the same quantity through the inner-sphere plane, so a pair on the very edge may differ by a rounding)"""
    pts = np.asarray(pts, F).reshape(-1, 3)
    d = np.sqrt(((pts[:, None, :] - state[None, :, :3]) ** 2).sum(-1, dtype=F)).astype(F)
    bound = (d - model.rinner[None, :]).min(axis=1)
    return ~((d - model.radius[None, :]) > bound[:, None])


def pairs_per_chunk(model, state, pts, stride=1):
    """the candidate pairs of every chunk of CH (sub-sampled) points"""
    c = candidates(model, state, np.asarray(pts)[::stride]).sum(axis=1)
    return [int(c[i:i + CH].sum()) for i in range(0, len(c), CH)]


def where(model, state, pts, i, stride=1):
    """(chunk, first window, last window) of the sub-sampled point i: the chunk of CH points it falls in and the windows of PAIR_WIN pairs that hold its candidate pairs"""
    sub = np.asarray(pts)[::stride]
    c0 = (i // CH) * CH
    c = candidates(model, state, sub[c0:i + 1]).sum(axis=1)
    before, own = int(c[:-1].sum()), int(c[-1])
    return i // CH, before // PAIR_WIN, (before + max(own, 1) - 1) // PAIR_WIN


# ---- the scenes: a model variant, one state, one cloud of NBASE points (cut to the counts per slot), a camera and the frame it sees ------------------------------------
def _natural(model, state, cam):
    depth, cloud = natural_cloud(model, state, cam)
    return state, cloud, depth


def _ring(model, cam):
    state = ring_state(model)
    return state, ball(RING_P, 0.004, NBASE, 7), render(model, state, cam)[0]


SCENES = {
    # name: (variant, what it is for)
    "nat17": ("hand17", "a tracked pose and its frame: fewer than PAIR_WIN pairs a chunk"),
    "nat26": ("hand26", "the same on 26 bodies"),
    "ring17": ("hand17", "every body a candidate of every point: more than PAIR_WIN pairs a chunk"),
    "ring26": ("hand26", "more than 2 PAIR_WIN pairs a chunk"),
    "mixed17": ("mixed17", "face counts from 1 to 92 in one wave: the range-tested scan"),
    "short_last": ("mixed17_short_last", "a last body of 5 faces: the scan's read-ahead behind the plane copy"),
    "uniform61": ("uniform61", "the fast scan at a largest count of 61"),
    "uniform16": ("uniform16", "the fast scan at a largest count of 16: no fast round at all"),
    "chain3": ("chain3", "three bodies of 98, 74 and 322 vertices"),
    "twins17": ("twins17", "two pairs of bitwise equal bodies at equal poses: exact ties between face planes of two bodies"),
    "fat_twins17": ("fat_twins17", "the same with inner spheres as large as the outer ones: the ties of the inner-sphere walk decide"),
    "mirror17": ("mirror17", "a body whose faces and vertices come in mirror pairs, points in its mirror plane: exact ties between two faces, two vertices"),
    "behind17": ("hand17", "nat17 with a body behind the camera"),
    "outside17": ("hand17", "nat17 with a body that projects outside the image"),
    "inside17": ("hand17", "every point inside a body: FitError from the bone term alone"),
}
DENSE = ("ring17", "ring26")


def scene(name, tmpdir):
    """dict(name, variant, path, model, state [nb,13], cloud [NBASE,3], cam [12], depth u16[64,64])"""
    variant = SCENES[name][0]
    path = variant_path(variant, tmpdir); model = Model(path); cam = camera()
    if name in DENSE:
        state, cloud, depth = _ring(model, cam)
    elif name == "nat26":
        state, cloud, depth = _natural(model, truth_state(2, "hand26"), cam)
    elif name in ("twins17", "fat_twins17"):
        state, cloud, depth = _natural(model, twins_state(truth_state(9)), cam)
    elif name == "mirror17":
        state = rest_state(model); state[MIRROR_BODY, 3:7] = (0, 0, 0, 1)
        state, cloud, depth = _natural(model, state, cam)
        cloud[2::2] = mirror_plane_points(model, state, NBASE, 21)[2::2]
    elif name in ("nat17", "behind17", "outside17", "inside17"):
        state, cloud, depth = _natural(model, truth_state(5), cam)
        if name == "behind17":
            state = body_in_camera(state, cam, 16, (0.01, 0.02, -0.3))
        if name == "outside17":
            state = body_in_camera(state, cam, 7, (0.6, -0.1, 0.4))
        if name == "inside17":
            cloud = inside(model, state, NBASE, 9)
    else:
        state, cloud, depth = _natural(model, rest_state(model), cam)
    # FitError's bone term compares a bone's depth with the frame's at its pixel and counts what lies between 0 and 1 cm: the frame handed to it is the rendered one pushed
    # back by 0 to 29 mm pixel by pixel, so that bones fall below, inside and above that range
    depth = np.where(depth > 0, depth + np.random.default_rng(13).integers(0, 30, depth.shape), 0).astype(np.uint16)
    assert cloud.shape == (NBASE, 3) and cloud.dtype == F and state.shape == (model.nb, 13) and depth.shape == (64, 64)
    return dict(name=name, variant=variant, path=path, model=model, state=state, cloud=cloud, cam=cam, depth=depth)
