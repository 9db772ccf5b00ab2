"""CPU: tests/kpfit_ref.py, the numpy restatement of the keypoint fit, pinned on the reference-pinned C restatement of the solver: one nail and the
eight landmark rays equal ho_slowfit bit for bit; presence, order and compaction of the rows; the convergence figures of DESIGN section 33; every wrong= variant is
noticed.  tests/test_gpu_kpfit.py holds the kernel to this restatement bit for bit."""
import numpy as np
import pytest

import joints_inputs as ji
import kpfit_inputs as ki
import kpfit_ref as kr
import oracle_lib as ol
import quality_ref as Q


@pytest.fixture(scope="module")
def oracles():
    made = {}

    def get(name):
        if name not in made:
            made[name] = ol.Oracle(None, ji.model_path(name))
        return made[name]
    yield get
    for o in made.values():
        o.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- (a) the two pins on ho_slowfit ----------------------------------------------------------------------------------------------------------------------------
def _nail(orc, wrong=None):
    """K = 1, unbounded force, momenta kept, 6 steps against slowfit's nailed bone (handtrack.h:809-810) without points: (restatement, ho_slowfit) states"""
    m = ji.model("hand17")
    st = ki.states_of(ki.truths("hand17")[1:2])
    tab = (np.array([7], np.int32), np.array([[0.001, 0.002, -0.01]], np.float32), np.array([1], np.int32))
    spoint = np.array([[[0.02, -0.03, 0.45]]], np.float32)
    tr, _ = kr.fit_loop(ol, orc, m, st, tab, steps=6, flags=kr.KEEP_MOMENTA, xyz=spoint, wrong=wrong)
    orc.set_state(0, st[0])
    orc.L.ho_slowfit(orc.h, None, 0, 0, None, 6, 7, ol.v3(spoint[0, 0]), ol.v3(tab[1][0]), None, 0)
    return tr[-1][0], orc.get_state(0), st[0]


def _rays8(orc, wrong=None):
    """the FEATURE8 points as pixel targets through an identity camera (radius 0.01, +-100000, 5 steps, momenta kept) against slowfit's crays = the restatement's own rays"""
    m, t8 = ji.model("hand17"), Q.feature8()
    sc = ki.scene("hand17", 1, t8)
    tr, _ = kr.fit_loop(ol, orc, m, sc["state"], t8, steps=5, flags=kr.KEEP_MOMENTA, kind=np.ones(8, np.int32), pix=sc["pix"], cams=sc["cams"], wrong=wrong)
    crays = np.ones((8, 4), np.float32); crays[:, :3] = kr.rays(sc["pix"], sc["cams"])[0]
    orc.set_state(0, sc["state"][0])
    orc.L.ho_slowfit(orc.h, None, 0, 0, None, 5, -1, ol.F3(0, 0, 0), ol.F3(0, 0, 0), ol.fptr(np.ascontiguousarray(crays.reshape(-1))), 8)
    return tr[-1][0], orc.get_state(0), sc["state"][0]


def test_one_nail_is_slowfits_nailed_bone(oracles):
    got, ref, start = _nail(oracles("hand17"))
    assert np.abs(ref[:, :7] - start[:, :7]).max() > 1e-3      # the nail moves the hand
    assert np.array_equal(_bits(got), _bits(ref))                # all 13 floats of every body


def test_feature8_rays_are_slowfits_crays(oracles):
    got, ref, start = _rays8(oracles("hand17"))
    assert np.abs(ref[:, :7] - start[:, :7]).max() > 1e-3
    assert np.array_equal(_bits(got), _bits(ref))


# ---- (b) presence ----------------------------------------------------------------------------------------------------------------------------------------------
def test_presence(oracles):
    m = ji.model("hand17"); tab = Q.skeleton(m); K = len(tab[0])
    sc = ki.scene("hand17", 3, tab)
    kind = ki.mixed_kind(K)
    xyz, pix, w = sc["xyz"].copy(), sc["pix"].copy(), np.ones((3, K), np.float32)
    w[0, 0] = 0; w[0, 1] = 0                      # a point and a pixel by weight
    xyz[0, 2, 1] = np.nan; pix[0, 4, 0] = np.nan    # one of each by a NaN component
    xyz[0, 1] = np.nan; pix[0, 3] = np.inf          # components the keypoint's kind does not read: still present
    w[2] = 0                                        # a frame with no keypoint at all
    full = 3 * int((kind == 0).sum()) + 4 * int((kind == 1).sum())
    rws = kr.rows(m, sc["state"], tab, kind=kind, xyz=xyz, pix=pix, weights=w, cams=sc["cams"])
    assert [len(r) for r in rws] == [full - 3 - 4 - 3 - 4, full, 0]
    res = kr.residuals(m, sc["state"], tab, kind=kind, xyz=xyz, pix=pix, weights=w, cams=sc["cams"])
    assert list(np.nonzero(res[0] < 0)[0]) == [0, 1, 2, 4] and (res[1] >= 0).all() and (res[2] == -1).all()
    assert all(np.isfinite(r).all() for r in rws)
    # the frame without rows: the step is plain FitPointCloud({}) with the joint ranges brought up to date
    tr, _ = kr.fit_loop(ol, oracles("hand17"), m, sc["state"], tab, steps=1, kind=kind, xyz=xyz, pix=pix, weights=w, cams=sc["cams"])
    orc = oracles("hand17")
    plain = kr.oracle_step(ol, orc, 0, sc["state"][2], np.zeros((0, 16), np.float32)); plain[:, 7:13] = 0
    assert np.array_equal(_bits(tr[1][2]), _bits(plain))
    # the force limits carry the weight: one multiplication
    w2 = np.full((3, K), 0.5, np.float32)
    r2 = kr.rows(m, sc["state"], tab, kind=kind, xyz=sc["xyz"], pix=sc["pix"], weights=w2, cams=sc["cams"], max_force=1000.0, ray_force=100000.0)[0]
    assert set(np.unique(np.abs(r2[:, 13:15]))) == {0.0, 500.0, 50000.0}


# ---- (c) order and compaction of mixed kinds -------------------------------------------------------------------------------------------------------------------
def test_order_and_compaction():
    m = ji.model("hand17"); tab = Q.skeleton(m); K = len(tab[0])
    sc = ki.scene("hand17", 4, tab, away=True)
    kind = ki.mixed_kind(K); w = ki.ragged_weights(4, K)
    rws = kr.rows(m, sc["state"], tab, kind=kind, xyz=sc["xyz"], pix=sc["pix"], weights=w, cams=sc["cams"], max_force=1e5)
    assert len(set(len(r) for r in rws)) == 4 and len(rws[3]) == 0      # every frame another row count, one without
    for f in range(4):
        at = 0
        for k in range(K):
            if w[f, k] <= 0:
                continue
            n = 4 if kind[k] else 3
            r = rws[f][at:at + n]; at += n
            assert (r[:, 0] == -1).all() and (r[:, 1] == tab[0][k]).all() and (r[:, 12] == 0).all() and (r[:, 15] == 0).all()
            off = tab[1][k] - m.com[tab[0][k]]      # skeleton offsets are user-frame offsets (rel = 0)
            assert np.array_equal(r[:, 5:8], np.broadcast_to(off, (n, 3)))
            if kind[k]:
                assert np.array_equal(r[:, 2:5], np.broadcast_to(sc["cams"][f, 5:8], (4, 3)))      # position0 = the camera's position
                assert np.array_equal(r[0, 8:11], r[1, 8:11]) and np.array_equal(r[2, 8:11], r[3, 8:11])
                assert abs(float(np.dot(r[0, 8:11], r[2, 8:11]))) < 1e-6 and abs(float(np.linalg.norm(r[0, 8:11])) - 1) < 1e-6
                f5 = np.float32(100000.0) * w[f, k]
                assert np.array_equal(r[:, 13:15], np.array([[0, f5], [-f5, 0], [0, f5], [-f5, 0]], np.float32))
                assert r[0, 11] - r[1, 11] == pytest.approx(0.02, abs=1e-6)
            else:
                assert np.array_equal(r[:, 2:5], np.broadcast_to(sc["xyz"][f, k], (3, 3)))
                assert np.array_equal(r[:, 8:11], np.eye(3, dtype=np.float32))
                f3 = np.float32(1e5) * w[f, k]
                assert np.array_equal(r[:, 13:15], np.broadcast_to(np.array([-f3, f3], np.float32), (3, 2)))
        assert at == len(rws[f])
    # float32 against the float64 yardstick: rounding level
    r64 = kr.rows(m, sc["state"], tab, kind=kind, xyz=sc["xyz"], pix=sc["pix"], weights=w, cams=sc["cams"], max_force=1e5, dtype=np.float64)
    for a, b in zip(rws, r64):
        assert a.shape == b.shape and (len(a) == 0 or np.abs(a[:, 2:13] - b[:, 2:13]).max() < 2e-6)


# ---- (d) convergence: the figures of DESIGN section 33 ------------------------------------------------------------------------------------------------------------
def _falls(res):
    a, b = kr.mean_residual(res[:, 0]), kr.mean_residual(res[:, 1])
    return bool((b < a).all())


@pytest.mark.parametrize("name", ["hand17", "hand26"])
def test_convergence(oracles, name):
    m = ji.model(name); tab = Q.skeleton(m); K = len(tab[0])
    orc = oracles(name)
    sc = ki.scene(name, 8, tab)
    tr, res = kr.fit_loop(ol, orc, m, sc["state"], tab, steps=10, xyz=sc["xyz"], max_force=1e5)
    print("%s: %d keypoints, %d rows; 3-D targets: mean %.2f mm -> %.3f mm after 10 steps, worst keypoint %.2f mm" % (name, K, 3 * K, 1e3 * res[:, 0].mean(), 1e3 * res[:, 1].mean(), 1e3 * res[:, 1].max()))
    assert np.isfinite(tr).all() and _falls(res)
    far = ki.scene(name, 8, tab, lag=32)
    tr, res = kr.fit_loop(ol, orc, m, far["state"], tab, steps=12, xyz=far["xyz"], max_force=1e5)
    print("%s: unrelated start: mean %.1f mm -> %.2f mm after 12 steps" % (name, 1e3 * res[:, 0].mean(), 1e3 * res[:, 1].mean()))
    assert np.isfinite(tr).all() and _falls(res)
    kind = np.ones(K, np.int32)
    for radius in (0.01, 0.0):
        tr, res = kr.fit_loop(ol, orc, m, sc["state"], tab, steps=10, kind=kind, pix=sc["pix"], cams=sc["cams"], ray_radius=radius)
        d3 = np.linalg.norm(Q.keypoints(m, tr[-1][:, :, :7], tab, np.float32, com_poses=True)["xyz"] - sc["xyz"], axis=-1)
        print("%s: ray targets, %d rows, radius %g: mean distance to the rays %.2f mm -> %.2f mm; 3-D error %.1f mm" % (name, 4 * K, radius, 1e3 * res[:, 0].mean(), 1e3 * res[:, 1].mean(), 1e3 * d3.mean()))
        # inside the dead zone nothing pulls: a frame that starts within a centimetre of its rays need not come closer, so only radius 0 must fall on every frame
        assert np.isfinite(tr).all() and (radius > 0 or _falls(res))
    assert 4 * K <= 5 * m.nb + 128


# ---- (e) every wrong= variant is noticed ---------------------------------------------------------------------------------------------------------------------------
def test_wrong_variants_are_noticed(oracles):
    assert kr.WRONG == ("rel", "origin", "limits")
    m = ji.model("hand17"); tab = Q.skeleton(m); K = len(tab[0])
    # at the target pose itself nothing pulls: every targetdist of a point is rounding, every ray passes through its keypoint -- for a camera away from the origin too
    sc = ki.scene("hand17", 2, tab, lag=0, away=True)
    kind = ki.mixed_kind(K)
    at_rest = lambda wrong: kr.residuals(m, sc["state"], tab, kind=kind, xyz=sc["xyz"], pix=sc["pix"], cams=sc["cams"], wrong=wrong)
    ok = at_rest(None)
    assert ok[:, kind == 0].max() < 1e-6 and ok[:, kind == 1].max() < 1e-5
    assert at_rest("rel")[:, kind == 0].max() > 1e-3        # user-frame offsets taken for centre-of-mass ones
    assert at_rest("origin")[:, kind == 1].max() > 1e-3     # the rays of a camera that is not at the origin
    assert np.array_equal(at_rest("limits"), ok)            # (the residuals cannot see the limits: the pin does)
    orc = oracles("hand17")
    got, ref, _ = _rays8(orc, wrong="limits")
    assert not np.array_equal(_bits(got), _bits(ref))       # a pair that pushes away from the ray
    # and the rows of each variant differ from the right ones
    right = kr.rows(m, sc["state"], tab, kind=kind, xyz=sc["xyz"], pix=sc["pix"], cams=sc["cams"])
    for wrong in kr.WRONG:
        bad = kr.rows(m, sc["state"], tab, kind=kind, xyz=sc["xyz"], pix=sc["pix"], cams=sc["cams"], wrong=wrong)
        assert any(not np.array_equal(a, b) for a, b in zip(right, bad)), wrong
