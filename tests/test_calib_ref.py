"""CPU: the restatement of ht_calibrate_view alone (tests/calib_ref.py; include/ht_mi355x.h "a view's extrinsics").  Scenes: hand17, three bench frames,
80x60, a second camera at 90 and at 180 degrees about the palm, the models at the ground truth.  RIG mode takes calib_ref.rig_scene (views_ref.two_view_scene's second camera
of the first frame, FIXED for the batch: the rig is fixed and the hand moves); PER_SLOT mode takes views_ref.two_view_scene as it is (a camera of its own a slot).
The guess: the true pose turned about (1,1,0)/sqrt 2 through the camera's own position and shifted.  RIG mode: 5 degrees and 20 mm, the first perturbation tried, met
the condition.  PER_SLOT mode (one frame a transform): at 5 degrees and 20 mm two of the three slots at 90 degrees end in another minimum (7.58e-3 and 2.68e-3 m^2 against
1.21e-3 at the truth; 30 iterations change nothing); halved once, 2.5 degrees and 10 mm, every slot at both angles meets it, and that is what the test uses.
Measured here (fraction 1, the defaults otherwise: 10 iterations, max_dist 0.03, damping 1e-3), RIG: truncated cost at the truth 3.190e-3 / 5.536e-3 m^2 (90 / 180
degrees), after 10 steps 1.255e-3 / 2.240e-3; rigid error of the recovered T 2.91 / 2.48 mm (the frames are rendered from the subdivision surface, the model closest()
knows is the convex bones: the truth is not the minimum)."""
import functools

import numpy as np
import pytest

import calib_ref as cr
import joints_inputs as ji
import oracle_lib as ol
import views_ref as vr

NAME, FRAMES, W, H = "hand17", (0, 3, 6), 80, 60
PERTURB = {True: (5.0, 0.02), False: (2.5, 0.01)}      # degrees, metres: RIG mode, PER_SLOT mode (halved once, see above)
RIGID_MEASURED = {90.0: 2.91e-3, 180.0: 2.48e-3}      # metres, RIG mode, measured on the restatement; the tests assert twice these (numpy and libm versions only)


@pytest.fixture(scope="module")
def orc():
    o = ol.Oracle(None, ji.model_path(NAME))
    yield o
    o.close()


@functools.lru_cache(None)
def scene(degrees, rig):
    sc = cr.rig_scene(NAME, FRAMES, W, H, degrees) if rig else vr.two_view_scene(NAME, FRAMES, W, H, degrees)
    depth, cams = np.ascontiguousarray(sc["depth"][:, 1]), np.ascontiguousarray(sc["cams"][:, 1])
    guess = np.stack([cr.perturbed(c, *PERTURB[rig]) for c in cams])
    return depth, cams, guess, sc["truth"]


@functools.lru_cache(None)
def _runs(degrees, rig):
    """(at the truth with iterations = 0, from the guess with the default iterations), computed once"""
    o = ol.Oracle(None, ji.model_path(NAME))
    try:
        depth, cams, guess, truth = scene(degrees, rig)
        mode = cr.RIG if rig else cr.PER_SLOT
        return cr.calibrate(o, depth, cams, truth, cr.options(fraction=1, iterations=0, mode=mode)), cr.calibrate(o, depth, guess, truth, cr.options(fraction=1, mode=mode))
    finally:
        o.close()


def _independent_cost(orc, depth, cams, truth, T, o):
    """sum over the points of min(r^2, max_dist^2) in plain float64 (the points placed by a float64 rotation matrix, one np.sum): no tree, no float32 term"""
    total = 0.0
    for b in range(len(depth)):
        orc.L.ho_set_pose(orc.h, 0, ol.fptr(np.ascontiguousarray(truth[b], np.float32)))
        p = cr.cloud(depth[b], cams[b], o).astype(np.float64)
        x = np.array([T[:3] + vr.qrot64(T[3:7], v) for v in p]).reshape(-1, 3)
        pl = cr.planes_of(orc, x.astype(np.float32)).astype(np.float64)
        r = (pl[:, :3] * x).sum(1) + pl[:, 3]
        total += float(np.minimum(r * r, float(np.float32(o["max_dist"])) ** 2).sum())
    return total


@pytest.mark.parametrize("degrees", [90.0, 180.0])
def test_one_step_at_the_truth_moves_less_and_row_0_is_the_cost(orc, degrees):
    depth, cams, guess, truth = scene(degrees, True)
    o = cr.options(fraction=1, iterations=1)
    _, at_truth = cr.calibrate(orc, depth, cams, truth, o)
    _, at_guess = cr.calibrate(orc, depth, guess, truth, o)
    print("%g degrees: one step from the truth |dt| %.3g |dw| %.3g, from the guess |dt| %.3g |dw| %.3g" % (degrees, at_truth[0, 0, 3], at_truth[0, 0, 4], at_guess[0, 0, 3], at_guess[0, 0, 4]))
    assert at_truth[0, 0, 3] < at_guess[0, 0, 3] and at_truth[0, 0, 4] < at_guess[0, 0, 4]
    assert at_truth[0, 0, 5] == 0 and at_truth[0, 0, 0] > 1000 and at_truth[0, 0, 1] == sum(len(cr.cloud(depth[b], cams[b], o)) for b in range(3))
    # float32 places a point to 3e-8 m and residuals are of the order of a millimetre: a term moves by 1e-4 of itself at most, far inside 1e-3 of the sum
    for c, st in ((cams, at_truth), (guess, at_guess)):
        want = _independent_cost(orc, depth, c, truth, c[0, 5:12].astype(np.float64), o)
        assert st[0, 0, 2] == pytest.approx(want, rel=1e-3)
    score = _runs(degrees, True)[0][1][0]      # iterations = 0 scores the same state: the same sums, no step
    assert np.array_equal(at_truth[0][:, [0, 1, 2] + list(range(5, cr.STATS))], score[:, [0, 1, 2] + list(range(5, cr.STATS))]) and not score[:, 3:5].any()


@pytest.mark.parametrize("degrees", [90.0, 180.0])
def test_rig_mode_ends_at_or_below_the_cost_of_the_truth(degrees):
    depth, cams, guess, truth = scene(degrees, True)
    (_, s_truth), (T, s) = _runs(degrees, True)
    pts = np.concatenate([cr.cloud(depth[b], cams[b], cr.options(fraction=1)) for b in range(3)])
    err0 = cr.rigid_error(guess[0, 5:12].astype(np.float64), cams[0, 5:12].astype(np.float64), pts)
    err = cr.rigid_error(T[0].astype(np.float64), cams[0, 5:12].astype(np.float64), pts)
    print("%g degrees, guess off by %g degrees and %g m (rigid error %.5f m): cost at the truth %.6g, at the guess %.6g, after %d steps %.6g; rigid error %.5f m"
          % (degrees, PERTURB[True][0], PERTURB[True][1], err0, s_truth[0, 0, 2], s[0, 0, 2], len(s) - 1, s[-1, 0, 2], err))
    assert T.shape == (1, 7) and s.shape == (11, 1, cr.STATS) and not s[:, 0, 5].any()
    assert s[-1, 0, 2] <= s_truth[0, 0, 2] < s[0, 0, 2]                     # a minimiser that found the basin cannot do worse than one particular point of it
    assert s[-1, 0, 3] == 0 and s[-1, 0, 4] == 0 and (s[:-1, 0, 3] > 0).all()      # the last row takes no step
    assert err <= 2 * RIGID_MEASURED[degrees] and err < err0 / 3
    assert abs(np.linalg.norm(T[0, 3:7].astype(np.float64)) - 1) < 1e-6


@pytest.mark.parametrize("degrees", [90.0, 180.0])
def test_per_slot_mode_meets_the_condition_in_every_slot(degrees):
    (_, s_truth), (T, s) = _runs(degrees, False)
    print("%g degrees per slot: cost at the truth %s, after 10 steps %s" % (degrees, s_truth[0, :, 2], s[-1, :, 2]))
    assert T.shape == (3, 7) and s.shape == (11, 3, cr.STATS) and not s[:, :, 5].any()
    assert (s[-1, :, 2] <= s_truth[0, :, 2]).all() and (s_truth[0, :, 2] < s[0, :, 2]).all()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_degenerate_inputs_leave_T_alone_and_set_the_flag(orc):
    depth, cams, guess, truth = scene(180.0, False)
    # a slot whose view sees nothing, beside slots that move
    blind = depth.copy(); blind[1] = 0
    T, s = cr.calibrate(orc, blind, guess, truth, cr.options(fraction=1, iterations=2, mode=cr.PER_SLOT))
    assert np.array_equal(_bits(T[1]), _bits(guess[1, 5:12])) and (s[:, 1, 5] == cr.FEW_INLIERS).all() and (s[:, 1, :5] == 0).all() and not s[:, 1, 6:].any()
    assert not np.array_equal(_bits(T[0]), _bits(guess[0, 5:12])) and not s[:, [0, 2], 5].any()
    # a batch below min_points
    n = int(_runs(180.0, False)[0][1][0, :, 1].sum())
    T, s = cr.calibrate(orc, depth, guess, truth, cr.options(fraction=1, iterations=2, min_points=n + 1))
    assert np.array_equal(_bits(T[0]), _bits(guess[0, 5:12])) and (s[:, 0, 5] == cr.FEW_INLIERS).all() and s[0, 0, 1] == n and s[0, 0, 0] <= n and not s[:, 0, 3:5].any()
    # every point beyond max_dist: with min_points it is "few inliers", without it the first pivot is zero
    far = guess.copy(); far[:, 5] += 0.5
    for min_points, flag in ((12, cr.FEW_INLIERS), (0, cr.BAD_PIVOT)):
        T, s = cr.calibrate(orc, depth, far, truth, cr.options(fraction=1, iterations=2, max_dist=0.01, min_points=min_points))
        assert np.array_equal(_bits(T[0]), _bits(far[0, 5:12])) and (s[:2, 0, 5] == flag).all() and s[2, 0, 5] == (flag & cr.FEW_INLIERS) and not s[:, 0, 0].any()
        assert s[0, 0, 2] == pytest.approx(s[0, 0, 1] * float(np.float32(0.01)) ** 2, rel=1e-12) and np.isfinite(s).all() and np.isfinite(T).all()
