"""The restatement of the model split (tests/split_model_ref.py) on hand-made cases with every answer written out, and the conditions of the
rendered scenes the GPU tests track, built on the host: the separable scenes split into their solo frames (also with the priors swapped: crossed hands), and the
touching scene -- the first 5 mm step at which the blob split sees one component -- is split with at most 2 % of its foreground cells mislabelled."""
import os

import numpy as np
import pytest

import htfx
import mirror_ref
import split_model_ref as R
import split_model_scene as SC
import split_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
FAR, HI, N = 4000, 650, 0xFFFF
F = np.float32
ABSENT = [0, N, 0, 0, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def closest():
    c = R.Closest()
    yield c
    c.close()


_priors, _frame, CAM, FOUR = SC.hand_made_priors, SC.small_frame, SC.SMALL_CAM, SC.FOUR


def _split(closest, frame, poses=None, cam=CAM, **kw):
    kw.setdefault("mode", R.ALWAYS)
    return R.split(frame[None], cam[None], (_priors() if poses is None else poses)[None], 0, HI, FAR, closest, **kw)


def test_two_by_two(closest):
    out = _split(closest, _frame(FOUR))
    assert out["labels"][0].tolist() == [[1, 0], [1, 0]] and out["source"].tolist() == [1] and out["n_components"].tolist() == [2]
    assert out["info"][0].tolist() == [[2, 0, 2, 1, 1, 0, 1, 1], [2, 1, 0, 1, 0, 0, 0, 1]]
    want = np.full((2, 8, 8), FAR, np.uint16)
    want[0, 2, 6], want[0, 6, 6], want[1, 1, 1], want[1, 5, 2] = 431, 433, 430, 432
    assert out["frames"][0].tolist() == want.tolist()
    d = out["dist"][0]
    assert np.isfinite(d).all() and (d[:, 1, 0] < d[:, 1, 1]).all() and (d[:, 0, 1] < d[:, 0, 0]).all() and (np.abs(d.min(axis=2)) < 0.03).all()
    # the left frame mirrored, its camera the mirrored camera
    m = _split(closest, _frame(FOUR), flags=R.MIRROR_LEFT)
    assert m["frames"][0, 1].tolist() == want[1][:, ::-1].tolist() and m["frames"][0, 0].tolist() == want[0].tolist()
    assert m["cams"][0, 1, 2] == F(7) - F(3.5) and m["cams"][0, 0].tolist() == CAM.tolist() and m["labels"].tolist() == out["labels"].tolist()


def test_the_first_minimal_pixel_in_raster_order_is_the_cells_point(closest):
    frame = _frame({(2, 1): 430, (1, 2): 430, (3, 3): 431, (6, 2): 431})      # cell (0, 0)'s minimum 430 occurs twice: (2, 1) comes first in raster order
    Q, xs, ys = R.first_min(frame)
    assert Q.tolist() == [[430, 431], [FAR, FAR]] and (xs[0, 0], ys[0, 0]) == (2, 1) and (xs[0, 1], ys[0, 1]) == (6, 2)
    out = _split(closest, frame)
    closest.set(R.prior_poses(_priors(), closest.com, 0))
    first, second = R.cell_point(2, 1, 430, CAM), R.cell_point(1, 2, 430, CAM)
    assert first.tolist() == [F(F(F(2) - F(3.5)) / F(20)) * F(F(430) * F(0.001)), F(F(F(1) - F(3.5)) / F(20)) * F(F(430) * F(0.001)), F(F(430) * F(0.001))]
    assert out["dist"][0, 0, 0, 0] == closest.dist(0, first) and out["dist"][0, 0, 0, 0] != closest.dist(0, second)
    assert out["dist"][0, 0, 0, 1] == closest.dist(1, first * np.array([-1, 1, 1], F))


def test_a_tie_goes_to_the_right_hand(closest):
    """left prior = mirror of the right prior, principal x = 4 and the cells' minimal pixels in column 4: v.x = 0, so both models see the same bodies and the same point
    up to the sign of a zero: d_R == d_L bit for bit"""
    cam = CAM.copy(); cam[2] = 4
    out = _split(closest, _frame({(4, 1): 430, (4, 6): 455, (1, 1): 430}), cam=cam)
    d = out["dist"][0]
    assert d[0, 1, 0] == d[0, 1, 1] and d[1, 1, 0] == d[1, 1, 1] and np.isfinite(d[:, 1]).all()
    assert out["labels"][0].tolist() == [[1, 0], [N, 0]]
    assert out["info"][0].tolist() == [[2, 0, 2, 1, 1, 0, 1, 1], [1, 1, 0, 0, 0, 0, 0, 0]]


def test_max_dist_keeps_a_cell_at_exactly_its_distance_and_drops_it_one_ulp_below(closest):
    frame = _frame({(1, 1): 380, (6, 2): 431})      # the left cell 5 cm in front of the hand: a positive distance
    free = _split(closest, frame)
    D = free["dist"][0, 0, 0].min()
    assert D == free["dist"][0, 0, 0, 1] and 0.01 < D < 0.08 and free["labels"][0].tolist() == [[1, 0], [N, N]]
    at = _split(closest, frame, max_dist=D)
    assert at["labels"].tolist() == free["labels"].tolist() and at["info"].tolist() == free["info"].tolist()
    below = _split(closest, frame, max_dist=np.nextafter(D, F(0)))
    assert below["labels"][0].tolist() == [[N, 0], [N, N]] and below["info"][0].tolist() == [[1, 0, 1, 0, 1, 0, 1, 0], ABSENT] and below["n_components"].tolist() == [1]
    assert below["dist"].tobytes() == free["dist"].tobytes()      # a dropped cell keeps its distances
    assert (below["frames"][0, 1] == FAR).all()
    for off in (np.inf, np.finfo(F).max):
        assert _split(closest, frame, max_dist=off)["labels"].tolist() == free["labels"].tolist()


def test_min_pixels_boundary(closest):
    two = _split(closest, _frame(FOUR), min_pixels=2)
    assert two["info"][0, :, 0].tolist() == [2, 2] and two["n_components"].tolist() == [2]
    three = _split(closest, _frame(FOUR), min_pixels=3)
    assert three["info"][0].tolist() == [ABSENT, ABSENT] and three["n_components"].tolist() == [0] and three["source"].tolist() == [1]
    assert three["labels"].tolist() == two["labels"].tolist() and (three["frames"] == FAR).all()      # the cells keep their labels, the frame writer matches none
    one_left = _frame({(1, 1): 430, (6, 2): 431, (6, 6): 433})
    out = _split(closest, one_left, min_pixels=2)
    assert out["info"][0].tolist() == [[2, 0, 2, 1, 1, 0, 1, 1], ABSENT] and out["n_components"].tolist() == [1]


def test_merged_takes_the_model_only_for_one_blob_that_holds_both_hands(closest):
    full = np.full((8, 8), 430, np.uint16)      # one blob of four cells, the minimal pixel of each its first
    blob = S.split(full[None], 0, HI, FAR, min_pixels=2, cams=CAM[None])
    assert blob["n_components"].tolist() == [1]
    out = _split(closest, full, mode=R.MERGED, min_pixels=2)
    assert out["source"].tolist() == [1] and out["n_components"].tolist() == [1] and out["labels"][0].tolist() == [[1, 0], [1, 0]] and out["info"][0, :, :2].tolist() == [[2, 0], [2, 1]]
    # the second hand would be absent: the blob split stands, byte for byte
    out = _split(closest, full, mode=R.MERGED, min_pixels=3)
    assert out["source"].tolist() == [0] and all(out[k].tobytes() == blob[k].tobytes() for k in ("frames", "info", "n_components", "labels", "cams"))
    assert np.isfinite(out["dist"]).all()      # (it was evaluated)
    right_only = _frame({(6, 2): 431, (6, 6): 433})
    blob = S.split(right_only[None], 0, HI, FAR, cams=CAM[None])
    out = _split(closest, right_only, mode=R.MERGED)
    assert blob["n_components"].tolist() == [1] and out["source"].tolist() == [0] and all(out[k].tobytes() == blob[k].tobytes() for k in ("frames", "info", "n_components", "labels"))
    # two blobs: nothing is evaluated
    diagonal = _frame({(1, 1): 430, (6, 6): 433})
    out = _split(closest, diagonal, mode=R.MERGED)
    blob = S.split(diagonal[None], 0, HI, FAR, cams=CAM[None])
    assert blob["n_components"].tolist() == [2] and out["source"].tolist() == [0] and np.isinf(out["dist"]).all() and out["info"].tobytes() == blob["info"].tobytes()


def test_swapping_the_priors_swaps_the_frames(closest):
    a = _split(closest, _frame(FOUR))
    b = _split(closest, _frame(FOUR), poses=_priors()[::-1])
    assert b["frames"][0, ::-1].tobytes() == a["frames"][0].tobytes() and b["labels"][0].tolist() == [[0, 1], [0, 1]]
    assert b["info"][0, ::-1, 2:].tolist() == a["info"][0, :, 2:].tolist() and b["info"][0, :, :2].tolist() == [[2, 0], [2, 1]]


def test_user_poses_are_brought_to_the_centre_of_mass_in_canonical_space(closest):
    """an update's poses_out fed back: user pose = pose * (-com) (physics.h:142); the left one is the mirror image of a canonical user pose"""
    P = _priors()
    canon = R.prior_poses(P, closest.com, 0)
    user = canon.copy()
    for k in range(2):
        for b in range(closest.nb):
            user[k, b, :3] = canon[k, b, :3] - R._qrot(canon[k, b, 3:], closest.com[b])
    user[1] = mirror_ref.poses(user[1][None])[0]      # real space
    back = R.prior_poses(user, closest.com, R.USER_POSES)
    assert np.abs(back - canon).max() < 1e-6
    out = _split(closest, _frame(FOUR), poses=user, flags=R.USER_POSES)
    ref = _split(closest, _frame(FOUR))
    assert out["labels"].tolist() == ref["labels"].tolist() and np.abs(out["dist"] - ref["dist"]).max() < 1e-5
    assert np.abs(_split(closest, _frame(FOUR), poses=user)["dist"] - ref["dist"]).max() > 1e-4      # without the flag they are other poses


def test_arguments_the_calls_refuse_are_refused_here_too(closest):
    for kw in (dict(max_dist=np.nan), dict(max_dist=-1.0), dict(mode=2), dict(flags=8), dict(flags=R.RIGHT_IS_LOW_X)):
        with pytest.raises(AssertionError):
            _split(closest, _frame(FOUR), **kw)
    _split(closest, _frame(FOUR), mode=R.MERGED, flags=R.RIGHT_IS_LOW_X)


# ---- the rendered scenes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from hand_tracking_samples_amd import native
    m = native.Model(R.MODEL17)
    yield m
    m.close()


def test_separable_scenes_split_into_their_solo_frames_also_with_crossed_priors(closest, model):
    """(a) section 27's scenes, the scenes' own poses as priors: the model split's frames are the solo frames byte for byte; with the priors swapped they are the swapped
    solo frames, which the position rule cannot express"""
    k = S.SCENES[0]
    P = S.scene_poses(k)
    solo = np.stack([model.render_mesh(P[0], S.SCENE_CAM, S.SCENE_W, S.SCENE_H, far=4.0)[0],
                     model.render_mesh(mirror_ref.poses(P[1][None])[0], mirror_ref.cams(S.SCENE_CAM[None], S.SCENE_W)[0], S.SCENE_W, S.SCENE_H, far=4.0)[0][:, ::-1]])
    assert S.separable(*solo)
    scene = np.minimum(*solo)
    kw = dict(min_pixels=S.SCENE_MIN_PIXELS)
    for mode in (R.ALWAYS, R.MERGED):
        out = R.split(scene[None], S.SCENE_CAM[None], P[None], 0, S.SCENE_HI, S.SCENE_FAR, closest, mode=mode, **kw)
        assert out["frames"][0].tobytes() == solo.tobytes() and out["source"].tolist() == [1 - mode] and out["n_components"].tolist() == [2]
    out = R.split(scene[None], S.SCENE_CAM[None], P[None, ::-1], 0, S.SCENE_HI, S.SCENE_FAR, closest, **kw)
    assert out["frames"][0].tobytes() == solo[::-1].tobytes() and (out["info"][0, :, 0] > 300).all()


@pytest.fixture(scope="module")
def touching(model):
    """(b) scene 300 with the lateral offset reduced in 5 mm steps until the composed hull frames' blob split first reports one component"""
    k = S.SCENES[1]
    shift = S.SCENE_SHIFT
    for _ in range(18):
        P = R.scene_poses_at(k, shift)
        solo = SC.solo_frames(model, P)
        both, truth = R.compose(*solo)
        n = S.split(both[None], 0, S.SCENE_HI, S.SCENE_FAR, min_pixels=S.SCENE_MIN_PIXELS)["n_components"][0]
        if n < 2:
            return dict(shift=shift, poses=P, solo=solo, frame=both, truth=truth, n=n)
        shift -= SC.STEP
    raise AssertionError("the hands never merged")


def test_the_touching_scene_is_split_with_at_most_two_percent_of_its_cells_mislabelled(closest, touching):
    t = touching
    assert t["n"] == 1 and abs(t["shift"] - SC.TOUCH_SHIFT) < 1e-9      # the premise, and the offset the GPU test renders at
    blob = S.split(t["frame"][None], 0, S.SCENE_HI, S.SCENE_FAR, min_pixels=S.SCENE_MIN_PIXELS)
    assert (blob["info"][0, :, 0] == 0).any()      # the blob split loses a hand
    for mode in (R.ALWAYS, R.MERGED):
        out = R.split(t["frame"][None], S.SCENE_CAM[None], t["poses"][None], 0, S.SCENE_HI, S.SCENE_FAR, closest, mode=mode, min_pixels=S.SCENE_MIN_PIXELS)
        wrong, fg = R.mislabelled(out["labels"][0], t["truth"])
        print("touching scene, offset %.3f m, mode %d: %d of %d foreground cells mislabelled (%.2f %%)" % (t["shift"], mode, wrong, fg, 100.0 * wrong / fg))
        assert out["source"].tolist() == [1] and (out["info"][0, :, 0] > 300).all() and fg > 800
        assert wrong <= 0.02 * fg


def test_the_touching_scene_with_priors_one_frame_stale_is_recorded(closest, touching):
    """(c) the previous animbank row's poses as priors: the share is printed, not bounded"""
    t = touching
    k = S.SCENES[1]
    stale = R.scene_poses_at((k - 1) % 1024, t["shift"])
    out = R.split(t["frame"][None], S.SCENE_CAM[None], stale[None], 0, S.SCENE_HI, S.SCENE_FAR, closest, min_pixels=S.SCENE_MIN_PIXELS)
    wrong, fg = R.mislabelled(out["labels"][0], t["truth"])
    print("touching scene, priors one row stale: %d of %d foreground cells mislabelled (%.2f %%)" % (wrong, fg, 100.0 * wrong / fg))
    assert fg > 800 and 0 <= wrong <= fg
