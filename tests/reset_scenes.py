"""Seeded scenes for the full-reset branch (k_reset, csrc/ht_cloud.hip: PoseFromScratch, then rounds of UnibodyFit), shared by tests/test_reset_ref.py and
tests/test_gpu_reset_fuzz.py.  A scene is a cloud of n points, a decoded analysis (landmark rays, a unit palmq, clench angles), a posed camera, a start pose and the
unibody_force it runs under.  Pure numpy, fixed seeds.  Test infrastructure only.

The cloud decides the path of the single-body solve: nr = (n + 3) / 4 rows; up to UB16_ROWS sixteen rows at a time, up to UB_LDS_ROWS row by row from LDS, beyond from HBM.
Clouds are points on and near the hulls of the model where PoseFromScratch puts it for the scene's analysis (tests/cloud_scenes.py: surface_samples), up to the default point
capacity; a family's scenes are cuts of such a cloud, so two scenes either side of a seam differ by the points between the cuts alone.

Families: edges (row counts at every seam of the kernel and point counts at the seams of PoseFromScratch's 256-point passes and their eight-term tail), natural17 / natural26
(random counts in each band), far (the cloud turned and moved away from the model: UnibodyFit does real work), limits (unibody_force 0.01: every limit binds; 1.0: none
does), thin (all points equal; points on the palm ray, weights at their 1e6 ceiling; 1 to 5 points), behind (the camera beyond the hand: rays from it face the other side
of every body), ubcom (a model variant whose proxy cube has a centre of mass off its origin -- the stock models' is zero, and the `+ com` of handtrack.h:455 would go
unchecked)."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

import cloud_scenes as cs
import htfx
import reset_ref

F = np.float32
UB16_ROWS, UB_LDS_ROWS, CAPACITY = 448, 896, 4096      # csrc/ht_cloud.hip; include/ht_mi355x.h: HT_MAX_POINTS
PATHS = ("blocked16", "lds", "hbm")
EDGE_ROWS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 447, 448, 449, 450, 895, 896, 897, 1024)
EDGE_POINTS = (255, 256, 257, 511, 512, 513, 263, 264, 265, 1287, 1288, 1289, 3591, 3592, 3593)      # 256 k + {7, 8, 9} for k = 1, 5, 14
CLENCH = (0.0, -0.3, 0.4, 1.1, 1.9, 2.4, -0.05, 0.8)      # 0, negative values, values above pi / 2
UBCOM = (0.004, -0.006, 0.005)
CENTRE = np.array([0.02, -0.01, 0.45])


def rows_of(n):
    return (n + 3) // 4


def path_of(n):
    nr = rows_of(n)
    return PATHS[0] if nr <= UB16_ROWS else PATHS[1] if nr <= UB_LDS_ROWS else PATHS[2]


_tmp = None


def model_path(name):
    """hand17 / hand26: the stock files; ubcom17: hand17 with the proxy cube's com moved off zero, baked into a temporary directory once per process"""
    global _tmp
    if name != "ubcom17":
        return cs.stock_path(name)
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="reset_scenes_")
        atexit.register(shutil.rmtree, _tmp, True)
    path = os.path.join(_tmp, "model_ubcom17.htfx")
    if not os.path.exists(path):
        m = dict(htfx.load(cs.stock_path("hand17")))
        u = m["unibody/f"].copy(); u[6:9] = UBCOM; m["unibody/f"] = u
        htfx.save(path, m)
    return path


@functools.lru_cache(None)
def model(name):
    return reset_ref.Model(model_path(name)), cs.Model(model_path(name))


def _unit(v):
    return v / np.linalg.norm(v)


def _axis_angle(axis, deg):
    t = np.deg2rad(deg) / 2.0
    return np.concatenate([_unit(np.asarray(axis, np.float64)) * np.sin(t), [np.cos(t)]])


def analysis(rng, centre, clench0):
    """[84]: rays 0:32 (the first three about the direction of `centre`), confidences 1, palmq 75:79 a unit quaternion, clench angles 79:84 from CLENCH"""
    an = np.zeros(84, F)
    for i in range(8):
        d = _unit(_unit(centre) + rng.normal(0, 0.02 if i < 3 else 0.3, 3))
        an[4 * i:4 * i + 3] = d; an[4 * i + 3] = 1.0
    an[48:56] = 1.0
    an[75:79] = _unit(rng.standard_normal(4)).astype(F)
    an[79:84] = [CLENCH[(clench0 + 3 * i) % len(CLENCH)] for i in range(5)]
    return an


def camera(rng, centre, behind=False):
    """a tile's camera [12] posed well off the origin; behind: beyond the hand as the origin sees it"""
    cam = cs.camera(away=False)
    side = rng.normal(0, 0.08, 3)
    cam[5:8] = (centre * 1.7 + side) if behind else (np.array([0.33, -0.04, 0.06]) + side)
    cam[8:12] = _axis_angle(rng.standard_normal(3), rng.uniform(10, 40) * (4 if behind else 1)).astype(F)
    return cam


@functools.lru_cache(None)
def base(name, seed, behind=False):
    """(analysis, camera, cloud [CAPACITY,3]) of one seed: the cloud lies on and near the hulls of the model as PoseFromScratch poses it with its palm at the centre"""
    rng = np.random.default_rng(1000 + seed)
    centre = CENTRE + rng.normal(0, 0.02, 3)
    an, cam = analysis(rng, centre, seed), camera(rng, centre, behind)
    ref, shapes = model(name)
    state = reset_ref.pose_from_scratch(ref, None, an, cam, pcom=centre).astype(F)
    p = cs.surface_samples(shapes, state)
    p = p[rng.permutation(len(p))[:CAPACITY]]
    p[::3] += rng.normal(0, 0.002, p[::3].shape)      # every third point up to a few millimetres off the surface
    return an, cam, np.ascontiguousarray(p, F)


def _scene(family, name, n, seed, cloud=None, force=0.1, behind=False, tag=""):
    an, cam, pts = base(name, seed, behind)
    cloud = pts[:n] if cloud is None else cloud
    assert len(cloud) == n <= CAPACITY
    start = cs.rest_state(model(name)[1])[:, :7].copy()
    return dict(name="%s/%s%s n=%d" % (family, name, tag, n), family=family, model=name, n=n, nr=rows_of(n), path=path_of(n), cloud=np.ascontiguousarray(cloud, F), analysis=an, cam=cam,
                start=start, unibody_force=float(F(force)))


def _far(name, seed, rng):
    an, cam, pts = base(name, seed)
    c = pts.astype(np.float64).mean(0)
    R = cs._qrot(_axis_angle(rng.standard_normal(3), rng.uniform(15, 50)), np.eye(3)).T
    d = _unit(rng.standard_normal(3)) * rng.uniform(0.05, 0.15)
    return ((pts.astype(np.float64) - c) @ R.T + c + d).astype(F)


@functools.lru_cache(None)
def scenes():
    out = []
    # edges: cuts of one hand17 cloud (the seams of the solve), of one hand26 cloud (the seams of PoseFromScratch's passes)
    for i, nr in enumerate(EDGE_ROWS):
        out.append(_scene("edges", "hand17", max(0, 4 * nr - (i % 4)), 1))      # every residue of n mod 4
    for n in EDGE_POINTS:
        out.append(_scene("edges", "hand26", n, 2))
    rng = np.random.default_rng(77)
    bands = ((40, 4 * UB16_ROWS), (4 * UB16_ROWS + 1, 4 * UB_LDS_ROWS), (4 * UB_LDS_ROWS + 1, CAPACITY))
    for fam, name in (("natural17", "hand17"), ("natural26", "hand26")):
        for lo, hi in bands:
            for k in range(4):
                out.append(_scene(fam, name, int(rng.integers(lo, hi + 1)), 10 + len(out)))
    for k in range(9):
        name = ("hand17", "hand26")[k % 2]; lo, hi = bands[k % 3]; n = int(rng.integers(lo, hi + 1)); seed = 40 + k
        out.append(_scene("far", name, n, seed, cloud=_far(name, seed, rng)[:n]))
    for k, force in enumerate((0.01, 1.0)):
        for j, (lo, hi) in enumerate(bands):
            for name in ("hand17", "hand26"):
                out.append(_scene("limits", name, int(rng.integers(lo, hi + 1)), 60 + 2 * j + k, force=force, tag=" force %g" % force))
    an, cam, pts = base("hand17", 70)
    ray = reset_ref.palm_ray(an)
    out.append(_scene("thin", "hand17", 64, 70, cloud=np.tile(pts[7], (64, 1)), tag=" equal"))
    out.append(_scene("thin", "hand17", 200, 70, cloud=(np.linspace(0.3, 0.6, 200)[:, None] * ray[None]).astype(F), tag=" on the palm ray"))
    for n in range(1, 6):
        out.append(_scene("thin", ("hand17", "hand26")[n % 2], n, 71))
    out.append(_scene("thin", "hand26", 1800, 72, cloud=np.tile(base("hand26", 72)[2][11], (1800, 1)), tag=" equal"))
    for k in range(8):
        name = ("hand17", "hand26")[k % 2]; lo, hi = bands[k % 3]
        out.append(_scene("behind", name, int(rng.integers(lo, hi + 1)), 80 + k, behind=True))
    for k, n in enumerate((37, 64, 301, 1000, 1789, 1793, 2600, 3700)):
        out.append(_scene("ubcom", "ubcom17", n, 90 + k))
    names = [s["name"] for s in out]
    assert len(set(names)) == len(names)
    return tuple(out)


FAMILIES = ("edges", "natural17", "natural26", "far", "limits", "thin", "behind", "ubcom")


def family(name):
    return [s for s in scenes() if s["family"] == name]


def path_counts():
    """{family: {path: scenes}}"""
    return {f: {p: sum(1 for s in family(f) if s["path"] == p) for p in PATHS} for f in FAMILIES}
