"""CPU only: the conditions under which tests/test_gpu_cloud_fuzz.py means something, asserted on the oracle alone (tests/cloud_scenes.py makes the scenes).
The dense scenes really turn the pair window of closest_chunk's phase B over, the natural ones do not; the away-facing shell gives ConvexHitCheck both outcomes; the twin
bodies really tie, bit for bit, and the lower one wins; every body of the mixed-count model is somebody's closest; every point count at a chunk edge occurs.  Prints, per
scene, the pairs per chunk, the hit and miss counts and the tie counts (run with -s; profiles/cloud_scenes_ref.txt keeps one such print).
No model variant was refused by either loader: both take a body's face count from its plane array (oracle/ho_track.c, csrc/ht_model_host.hip)."""
import ctypes as C

import numpy as np
import pytest

import cloud_scenes as cs
import oracle_lib as ol
import views_ref as vr

ZERO = np.zeros(3, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cloud_models"); made = {}

    def get(name):
        if name not in made:
            sc = cs.scene(name, tmp); sc["orc"] = ol.Oracle(None, model=sc["path"])
            made[name] = sc
        return made[name]
    yield get
    for sc in made.values():
        sc["orc"].close()


def _rows(sc, origin):
    pts4 = np.concatenate([sc["cloud"], np.zeros((len(sc["cloud"]), 1), np.float32)], axis=1)
    return vr.rows(ol, sc["orc"], 0, sc["state"], pts4, [origin], 1.0, 1.0)


def _hit_miss(sc, origin):
    """(rows whose normal is the ray: ConvexHitCheck hit; away-facing rows that keep the plane's normal: it missed)"""
    r = _rows(sc, origin)
    d = sc["cloud"] - origin
    away = (d * r[:, 8:11]).sum(1) > 0
    with np.errstate(all="ignore"):
        ray = d / np.linalg.norm(d, axis=1, keepdims=True)
    hit = np.abs(r[:, 8:11] - ray).max(1) < 1e-6
    return int(hit.sum()), int((away & ~hit).sum()), r


def test_counts_cover_the_chunk_edges():
    flat = [n for b in cs.BATCHES for n in b]
    assert sorted(flat) == list(cs.COUNTS) and all(len(b) <= 8 for b in cs.BATCHES)
    assert all(list(b) != sorted(b) for b in cs.BATCHES)
    for edge in (cs.CH, 256, 384):      # the rows' chunk, the plane scan's chunk, a third chunk: the second block's second pass
        assert {edge - 1, edge, edge + 1} <= set(flat)
    assert max(flat) == cs.NBASE


@pytest.mark.parametrize("name", sorted(cs.SCENES))
def test_pairs_per_chunk(scenes, name):
    sc = scenes(name)
    per = {s: cs.pairs_per_chunk(sc["model"], sc["state"], sc["cloud"], s) for s in (1, 4, 7)}
    print("%-10s (%s) pairs per chunk: stride 1 %s, stride 4 %s, stride 7 %s" % (name, sc["variant"], per[1], per[4], per[7]))
    full = per[1][:cs.NBASE // cs.CH]
    if name in cs.DENSE:
        assert min(full) > (2 if name == "ring26" else 1) * cs.PAIR_WIN
        assert any(p % cs.PAIR_WIN for p in full)      # a chunk ends in a partial window
        assert max(per[4]) > cs.PAIR_WIN and max(per[7]) > cs.PAIR_WIN      # sub-sampled too: the window turns over inside a ragged chunk (74 points at stride 7)
    else:
        assert max(per[1]) < cs.PAIR_WIN
    c = cs.candidates(sc["model"], sc["state"], sc["cloud"])
    assert c.any(axis=1).all()
    # the candidate rule keeps the body the oracle picks
    rb = _rows(sc, ZERO)[:, 1].astype(int)
    assert c[np.arange(len(rb)), rb].mean() > 0.99


@pytest.mark.parametrize("name", ["nat17", "nat26", "mixed17", "uniform16", "twins17"])
def test_away_facing_points_hit_and_miss(scenes, name):
    sc = scenes(name)
    h0, m0, r0 = _hit_miss(sc, ZERO); h1, m1, r1 = _hit_miss(sc, sc["cam"][5:8])
    print("%-10s ConvexHitCheck from zero: %d hit, %d miss; from the camera: %d hit, %d miss; rows that differ between the origins: %d" % (name, h0, m0, h1, m1, int((_bits(r0) != _bits(r1)).any(1).sum())))
    assert min(h0, m0, h1, m1) >= 10
    assert (_bits(r0) != _bits(r1)).any()


def test_dense_ball_hits(scenes):
    for name in cs.DENSE:
        h, m, _ = _hit_miss(scenes(name), ZERO)
        print("%-10s ConvexHitCheck from zero: %d hit, %d miss of %d" % (name, h, m, cs.NBASE))
        assert h >= 10


@pytest.mark.parametrize("name", ["twins17", "fat_twins17"])
def test_twins_tie_bit_for_bit_and_the_lower_body_wins(scenes, name):
    sc = scenes(name); orc = sc["orc"]; m = orc.model(0)
    for a, c in cs.TWINS:
        assert np.array_equal(_bits(sc["state"][a]), _bits(sc["state"][c]))
    orc.set_state(0, sc["state"])
    first = []
    for v in sc["cloud"]:
        p = ol.F4(); first.append((orc.L.ho_closest(m, ol.v3(v), C.byref(p)), (p.x, p.y, p.z, p.w)))
    got = np.array([f[0] for f in first])
    assert not np.isin(got, [c for _, c in cs.TWINS]).any()      # never the copy: the first strict minimum in body order
    for a, c in cs.TWINS:
        away = sc["state"].copy(); away[a, 2] += 10.0      # without the original the copy takes its place, at the very same plane
        orc.set_state(0, away)
        ties = 0
        for i in np.flatnonzero(got == a):
            p = ol.F4(); rb = orc.L.ho_closest(m, ol.v3(sc["cloud"][i]), C.byref(p))
            ties += int(rb == c and np.array_equal(_bits(np.array((p.x, p.y, p.z, p.w))), _bits(np.array(first[i][1]))))
        print("%-10s bodies %d | %d: %d points closest to %d, %d of them tie with %d bit for bit" % (name, a, c, int((got == a).sum()), a, ties, c))
        assert ties >= 10
        if name == "fat_twins17":      # ... and the winning plane is the inner-sphere plane of the first walk, whose tie rule (`du < dmin` across the halves) then decides the body
            inner = 0
            for i in np.flatnonzero(got == a):
                d = (sc["cloud"][i] - sc["state"][a, :3]).astype(np.float64); n = np.linalg.norm(d)
                inner += int(n > 0 and np.abs(np.array(first[i][1][:3]) - d / n).max() < 1e-5)
            print("%-10s bodies %d | %d: %d of them keep the inner-sphere plane" % (name, a, c, inner))
            assert inner >= 10
    orc.set_state(0, sc["state"])


def test_mirror_body_ties_two_faces_and_two_vertices(scenes):
    """points in the mirror plane of body MIRROR_BODY: its most-above face ties with the face's image, three faces on, bit for bit (float32, the kernel's order of the
    sum); the lower index must win, and it sits on every one of the four lanes.  Boundary plane 2's normal has x = 0 by construction of the scan (tangent (1, 0, 0)), so the
    body's support vertex ties with its image fifteen vertices on."""
    sc = scenes("mirror17"); m = sc["model"]; b = cs.MIRROR_BODY; st = sc["state"]
    assert st[b, 3:7].tolist() == [0, 0, 0, 1]
    rows = _rows(sc, ZERO)
    sel = np.flatnonzero((rows[:, 1] == b) & (sc["cloud"][:, 0] == st[b, 0]))
    P = m.planes[b]; loc = sc["cloud"][sel] - st[b, :3]
    assert not loc[:, 0].any()
    vals = ((P[None, :, 0] * loc[:, None, 0] + P[None, :, 1] * loc[:, None, 1]) + P[None, :, 2] * loc[:, None, 2]) + P[None, :, 3]
    first = vals.argmax(axis=1)
    tied = (vals == vals.max(axis=1, keepdims=True)).sum(axis=1) > 1
    lanes = np.bincount(first[tied] % 4, minlength=4)
    print("mirror17   %d points closest to body %d in its mirror plane, %d with two equal most-above faces; lane of the lower face %s" % (len(sel), b, int(tied.sum()), lanes.tolist()))
    assert tied.sum() >= 10 and (lanes > 0).all()
    want_n = P[first, :3]      # the identity orientation: the row's normal is the plane's own where ConvexHitCheck did not replace it
    kept = (_bits(rows[sel, 8:11]) == _bits(want_n)).all(axis=1)
    assert (kept & tied).sum() >= 10
    orc = sc["orc"]; orc.set_state(0, st)
    lin = (ol.Linear * (5 * m.nb))()
    assert orc.L.ho_cloud_chamber(orc.model(0), ol.f3ptr(sc["cloud"]), cs.NBASE, lin, 10.0) == 5 * m.nb
    r = ol.linears_to_array(lin, 5 * m.nb)[2 * m.nb + b]
    assert r[8] == 0 and r[1] == b
    V = m.verts[b]; d = (V[:, 0] * np.float32(0) + V[:, 1] * -r[9]) + V[:, 2] * -r[10]
    k = int(np.flatnonzero(d == d.max())[0]); ties = int((d == d.max()).sum())
    print("mirror17   boundary plane 2: support vertex %d of body %d, %d vertices with that value" % (k, b, ties))
    assert ties >= 2 and np.array_equal(_bits(r[5:8]), _bits(V[k]))


@pytest.mark.parametrize("name", ["mixed17", "short_last"])
def test_every_body_of_the_mixed_model_is_closest_somewhere(scenes, name):
    sc = scenes(name)
    assert sc["model"].nplanes == list(cs.MIXED17 if name == "mixed17" else cs.MIXED17_SHORT_LAST)
    assert {92, 91, 64, 49, 48, 17, 16, 15, 5, 4, 3, 2, 1} <= set(sc["model"].nplanes)
    assert max(sc["model"].nplanes) - sc["model"].nplanes[-1] == (3 if name == "mixed17" else 87)
    n = np.bincount(_rows(sc, ZERO)[:, 1].astype(int), minlength=sc["model"].nb)
    print("%-10s points per closest body: %s" % (name, n.tolist()))
    assert (n > 0).all()
    for cut in (127, 255):      # and in the smaller cuts most of them
        assert (np.bincount(_rows(sc, ZERO)[:cut, 1].astype(int), minlength=sc["model"].nb) > 0).sum() >= sc["model"].nb - 2


def test_uniform_models(scenes):
    for name, k in (("uniform61", 61), ("uniform16", 16), ("chain3", 92)):
        assert scenes(name)["model"].nplanes == [k] * 3


def test_cloud_constraint_rows_are_views_ref_rows(scenes):
    """one restatement of the rows serves the cloud tests and the views tests: views_ref.rows is ho_cloud_constraint in ht_stage_cloud_rows' layout, unit limits at
    microforce 1 and weak force 1, FitPointCloud's otherwise"""
    sc = scenes("nat17"); orc = sc["orc"]; org = sc["cam"][5:8]
    pts4 = np.concatenate([sc["cloud"], np.zeros((cs.NBASE, 1), np.float32)], axis=1)
    got = vr.rows(ol, orc, 0, sc["state"], pts4, [org], 1.0, 1.0)
    orc.set_state(0, sc["state"])
    lin = (ol.Linear * cs.NBASE)()
    for i, v in enumerate(sc["cloud"]):
        lin[i] = orc.L.ho_cloud_constraint(orc.model(0), ol.v3(v), ol.v3(org))
    want = ol.linears_to_array(lin, cs.NBASE)
    assert np.array_equal(_bits(got), _bits(want))
    assert (want[:, 0] == -1).all() and np.array_equal(_bits(want[:, 2:5]), _bits(sc["cloud"])) and (want[:, 13] == -1).all() and (want[:, 14] == 1).all() and not want[:, [12, 15]].any()
    fit = vr.rows(ol, orc, 0, sc["state"], pts4, [org], 3.0, 0.4)
    assert np.array_equal(_bits(fit[:, :13]), _bits(want[:, :13]))
    k = np.where(want[:, 1] <= 2, np.float32(0.4), np.float32(1.0)) * np.float32(3.0)
    assert np.array_equal(fit[:, 14], k) and np.array_equal(fit[:, 13], -k)


def test_special_points_and_states(scenes):
    sc = scenes("nat17"); st, cl = sc["state"], sc["cloud"]
    assert np.array_equal(cl[0], st[8, :3]) and np.array_equal(cl[cs.CH - 1], st[0, :3]) and np.array_equal(cl[cs.CH], st[16, :3])      # points exactly at a body's position
    assert abs(np.linalg.norm(cl[1]) - 10.0) < 1e-3
    r = _rows(sc, ZERO)
    assert np.isfinite(r).all()
    cam = ol.camera(sc["cam"])
    for name, body in (("behind17", 16), ("outside17", 7)):
        s = scenes(name); orc = s["orc"]
        p = cs._qrot(np.array([-s["cam"][8], -s["cam"][9], -s["cam"][10], s["cam"][11]]), s["state"][body, :3].astype(np.float64) - s["cam"][5:8])
        px = p[0] / p[2] * 90.0 + 31.5
        assert (p[2] < -0.1) if name == "behind17" else (p[2] > 0.1 and px > 64)
        orc.set_state(0, s["state"])
        e = orc.L.ho_fit_error(orc.h, orc.model(0), ol.f3ptr(s["cloud"]), cs.NBASE, ol.u16ptr(np.ascontiguousarray(s["depth"].reshape(-1))), C.byref(cam))
        print("%-10s FitError %.6f" % (name, e))
        assert np.isfinite(e)
    s = scenes("inside17"); orc = s["orc"]; orc.set_state(0, s["state"])
    d = np.ascontiguousarray(s["depth"].reshape(-1))
    e = orc.L.ho_fit_error(orc.h, orc.model(0), ol.f3ptr(s["cloud"]), cs.NBASE, ol.u16ptr(d), C.byref(cam))
    e0 = orc.L.ho_fit_error(orc.h, orc.model(0), ol.f3ptr(s["cloud"]), 0, ol.u16ptr(d), C.byref(cam))
    print("inside17   FitError %.6f, without a point %.6f" % (e, e0))
    assert e == e0 and e > 0      # the bone term alone, and not nothing


def test_plane_clouds_meet_zeros(scenes):
    """the containing-plane scan's strict `> 0` sees exact zeros on the duplicated and the collinear cloud"""
    sc = scenes("nat17")
    for what, cloud in zip(("duplicated", "collinear"), cs.plane_clouds(sc["cloud"])):
        assert cloud.shape == (cs.NBASE, 3)
        zeros = 0
        for od in ((-1, -0.25, 0), (-1, -1, 0), (0, -1, 0), (1, -1, 0), (1, -0.25, 0)):
            od = np.array(od, np.float32); best = np.array([0, 0, 1], np.float32) - od; tangent = np.cross(best, od)
            for p in cloud:
                d = np.dot(np.cross(best, p), tangent)
                zeros += int(d == 0)
                if d > 0:
                    best = p
        print("nat17      %s cloud: %d exact zeros in the five plane scans" % (what, zeros))
        assert zeros >= 10
