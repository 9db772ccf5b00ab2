"""CPU: pins tests/quality_ref.py (the numpy restatement the accuracy kernels are compared with, tests/test_gpu_quality.py) on the host's ImageFeaturePoints
(ht_expected_cnn_full, itself pinned on the reference), on float64 anchors of the bench frames and on hand-written cases with every answer written out; shows that
three wrong restatements land far away on the same inputs."""
import ctypes as C
import os

import numpy as np
import pytest

import joints_inputs as ji
import joints_ref as jr
import mirror_ref
import pose_frame
import quality_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
IDENT = [0, 0, 0, 0, 0, 0, 1]


@pytest.fixture(scope="module")
def bench():
    return np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))


def _cam(fx, fy, cx, cy, ds=0.001, pose=IDENT):
    return np.array([[fx, fy, cx, cy, ds] + list(pose)], F)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


# ---- pinned on the oracle ------------------------------------------------------------------------------------------------------------------------------
def test_feature8_pixels_equal_the_hosts_image_feature_points_bit_for_bit(bench):
    gt, cam = bench["gtpose"][:64].astype(F), bench["cam"][:64].astype(F)
    _, ip, _ = pose_frame.host_labels(gt, cam)
    hcam = cam.copy(); hcam[:, :4] = cam[:, :4] / F(4.0)      # camsub(cam, 4): the 16x16 heat-map camera
    mine = Q.keypoints(ji.model("hand17"), gt, Q.feature8(), np.float32, com_poses=True, cams=hcam)["pix"]
    assert mine.dtype == np.float32 and np.array_equal(_bits(mine), _bits(ip))
    assert np.isfinite(mine).all() and mine.min() > -16 and mine.max() < 32


# ---- anchors -------------------------------------------------------------------------------------------------------------------------------------------------
def test_bench_anchors(bench):
    m = ji.model("hand17")
    res = {}
    for T in (np.float32, np.float64):
        a = Q.keypoints(m, bench["startpose"], Q.feature8(), T, com_poses=True)["xyz"]
        b = Q.keypoints(m, bench["gtpose"], Q.feature8(), T, com_poses=True)["xyz"]
        e = Q.errors(a, b, [0.02], T)
        res[T] = (float(e["sum_kp"].sum() / (1024 * 8)), float(e["dist"].max()), int((e["frame"][:, 1] < T(0.02)).sum()))
        print(T.__name__, "mean %.6e worst %.6e frames under 0.02: %d" % res[T])
    # the float64 figures as the issue quotes them, to the digits quoted (half a unit of the fifth); float32 within 1e-5 relative of float64
    assert abs(res[np.float64][0] - 4.1122e-3) <= 0.5e-7 and abs(res[np.float64][1] - 0.20020) <= 0.5e-5
    assert res[np.float64][2] == 1001 and res[np.float32][2] == 1001
    assert abs(res[np.float32][0] - res[np.float64][0]) <= 1e-5 * res[np.float64][0]
    assert abs(res[np.float32][1] - res[np.float64][1]) <= 1e-5 * res[np.float64][1]
    assert Q.identity_cams(bench["cam"]).all()      # item 7 must copy on this file
    p = bench["gtpose"][:8].astype(F)
    assert np.array_equal(_bits(Q.pose_to_render(m, p, bench["cam"][:8], np.float32, com_poses=True)), _bits(p))


# ---- hand-written cases ----------------------------------------------------------------------------------------------------------------------------------------
CHAIN2 = Q.Chain(com=[[0.5, 0, 0], [0, 0.25, 0]], joints=[(0, 1, [0, -0.5, 0])])
QZ90 = [0, 0, np.sqrt(0.5), np.sqrt(0.5)]      # a quarter turn about z: x -> y, y -> -x


def test_two_bone_chain_by_hand():
    b, off, rel = Q.skeleton(CHAIN2)
    assert b.tolist() == [0, 1, 1] and rel.tolist() == [0, 0, 0]      # origin, the joint's child anchor, the leaf (body 1; body 0 is a parent)
    assert off.tolist() == [[0, 0, 0], [0, -0.5, 0], [0, 0.25, 0]]
    poses = np.array([[[1, 2, 3, 0, 0, 0, 1], [2, 2, 3] + QZ90]], np.float64)
    x = Q.keypoints(CHAIN2, poses, (b, off, rel), np.float64)["xyz"][0]
    assert np.allclose(x, [[1, 2, 3], [2.5, 2, 3], [1.75, 2, 3]], atol=1e-15)      # (0,-0.5,0) turned to (0.5,0,0); (0,0.25,0) to (-0.25,0,0)
    x32 = Q.keypoints(CHAIN2, poses, (b, off, rel), np.float32)["xyz"][0]
    assert x32.dtype == np.float32 and np.allclose(x32, x, atol=1e-6)


def test_rel_conversions_in_both_directions_by_hand():
    one = lambda rel: (np.array([1]), np.array([[0.125, 0, 0]], F), np.array([rel]))
    pose = np.array([[[0, 0, 0, 0, 0, 0, 1], [1, 1, 1, 0, 0, 0, 1]]], F)
    k = lambda rel, com_poses: Q.keypoints(CHAIN2, pose, one(rel), np.float32, com_poses=com_poses)["xyz"][0, 0].tolist()
    assert k(0, False) == [1.125, 1, 1] and k(1, True) == [1.125, 1, 1]      # matching conventions: o' = o
    assert k(1, False) == [1.125, 1.25, 1]                                   # user poses, centre-of-mass offset: + com[1] = (0, 0.25, 0)
    assert k(0, True) == [1.125, 0.75, 1]                                    # centre-of-mass poses, user offset: - com[1]


def test_leaf_rule_on_the_chain_model():
    m = jr.Model(os.path.join(ROOT, "tests", "golden", "model_chain3.htfx"))
    b, off, rel = Q.skeleton(m)
    assert m.nb == 3 and m.nj == 2 and m.rb0.tolist() == [0, 1] and m.rb1.tolist() == [1, 2]
    assert b.tolist() == [0, 1, 2, 2] and not rel.any()      # 1 + 2 joints + the one leaf (body 2)
    assert np.array_equal(off[1:3], m.p1) and np.array_equal(off[3], m.com[2])
    b17 = Q.skeleton(ji.model("hand17"))[0]
    assert len(b17) == 22 and b17[17:].tolist() == [4, 7, 10, 13, 16]      # 1 + 16 + the five fingertips


def _one_point(x, y, z, cam, depth=None, **kw):
    m = Q.Chain(com=[[0, 0, 0]], joints=[])
    t = (np.array([0]), np.zeros((1, 3), F), np.array([0]))
    return Q.keypoints(m, np.array([[[x, y, z, 0, 0, 0, 1]]], F), t, np.float32, cams=cam, depth=depth, **kw)


def test_pixels_borders_and_the_five_codes_by_hand():
    cam = _cam(4, 4, 1.5, 0.5)
    near = np.full((1, 2, 4), 500, np.uint16)      # 0.5 m everywhere
    r = _one_point(0.25, 0.125, 1.0, cam, near, near_tol=0.25, far_tol=0.25)
    assert r["pix"][0, 0].tolist() == [2.5, 1.0] and r["zc"][0, 0] == 1.0      # 0.25 / 1 * 4 + 1.5, 0.125 / 1 * 4 + 0.5
    assert r["ixy"][0, 0].tolist() == [3, 1] and r["vis"][0, 0] == Q.OCCLUDED      # floor(3.0), floor(1.5); 0.5 < 1 - 0.25
    assert _one_point(0.25, 0.125, 1.0, cam, near, near_tol=0.5, far_tol=0)["vis"][0, 0] == Q.VISIBLE      # 0.5 < 0.5 fails, 0.5 > 1 fails
    assert _one_point(0.25, 0.125, 0.25, _cam(1, 1, 1.5, 0.5), near, near_tol=0, far_tol=0.125)["vis"][0, 0] == Q.NOTHING      # 0.5 > 0.25 + 0.125
    assert _one_point(0.25, 0.125, 0.25, _cam(1, 1, 1.5, 0.5), near, near_tol=0, far_tol=0.25)["vis"][0, 0] == Q.VISIBLE       # 0.5 > 0.5 fails
    for z in (-1.0, 0.0):      # behind the camera, and in its plane (u is infinite or NaN: tested before the pixel is)
        assert _one_point(0.25, 0.125, z, cam, near, near_tol=1, far_tol=1)["vis"][0, 0] == Q.BEHIND
    # the borders: u + 0.5 = w exactly is outside, u + 0.5 = 0 exactly is inside, on both axes (w = 4, h = 2)
    assert _one_point(0.5, 0.0, 1.0, cam, near, near_tol=1, far_tol=1)["pix"][0, 0].tolist() == [3.5, 0.5]
    assert _one_point(0.5, 0.0, 1.0, cam, near, near_tol=1, far_tol=1)["vis"][0, 0] == Q.OUTSIDE       # 3.5 + 0.5 = 4 = w
    assert _one_point(0.25, 0.25, 1.0, cam, near, near_tol=1, far_tol=1)["vis"][0, 0] == Q.OUTSIDE     # y: 1.5 + 0.5 = 2 = h
    r = _one_point(-0.5, -0.25, 1.0, cam, near, near_tol=1, far_tol=1)      # (-0.5, -0.5): u + 0.5 = 0 on both axes
    assert r["pix"][0, 0].tolist() == [-0.5, -0.5] and r["vis"][0, 0] == Q.VISIBLE and r["ixy"][0, 0].tolist() == [0, 0]
    assert _one_point(-0.53125, 0, 1.0, cam, near, near_tol=1, far_tol=1)["vis"][0, 0] == Q.OUTSIDE      # u + 0.5 = -0.125
    r = _one_point(0.46875, 0.21875, 1.0, cam, near, near_tol=1, far_tol=1)      # (3.375, 1.375): the last pixel
    assert r["ixy"][0, 0].tolist() == [3, 1] and r["vis"][0, 0] == Q.VISIBLE


def test_camera_pose_by_hand():
    cam = _cam(2, 2, 0, 0, pose=[1, 0, 0] + QZ90)      # a camera at (1,0,0) turned a quarter about z: world x is its -y ... conj turns y -> x, x -> -y
    r = Q.keypoints(Q.Chain(com=[[0, 0, 0]], joints=[]), np.array([[[1, 3, 2, 0, 0, 0, 1]]], np.float64), (np.array([0]), np.zeros((1, 3), F), np.array([0])), np.float64, cams=cam)
    assert np.allclose(r["pix"][0, 0], [3.0, 0.0], atol=1e-12) and np.isclose(r["zc"][0, 0], 2.0)      # X - pc = (0,3,2) -> v = (3,0,2): 3 / 2 * 2, 0


def test_depth_compare_by_hand():
    a = np.array([[[10, 20, 30], [40, 50, 60]]], np.uint16)
    b = np.array([[[12, 19, 99], [40, 10, 59]]], np.uint16)
    # lo 10, hi 60: a has 10 20 30 40 50 (60 is out: half open), b has 12 19 40 10 59; both at (10,12) (20,19) (40,40) (50,10) -> |d| = 2 1 0 40
    assert Q.depth_compare(a, b, 10, 60, 1).tolist() == [[5, 5, 4, 2, 43, 4 + 1 + 0 + 1600, 40, 0]]
    assert Q.depth_compare(a, b, 10, 61, 1).tolist() == [[6, 5, 5, 3, 44, 1606, 40, 0]]      # 60 comes in, paired with 59
    assert Q.depth_compare(a, b, 11, 60, 65535).tolist() == [[4, 4, 2, 2, 1, 1, 1, 0]]      # both 10s go out and take the pairs (10,12) and (50,10) along: (20,19) (40,40)
    assert Q.depth_compare(a, b + 100, 10, 60, 5).tolist() == [[5, 0, 0, 0, 0, 0, 0, 0]]         # an empty intersection
    assert Q.depth_compare(a, a, 0, 65536, 0).tolist() == [[6, 6, 6, 6, 0, 0, 0, 0]]


def test_errors_by_hand():
    a = np.zeros((2, 2, 3), F); b = np.zeros((2, 2, 3), F)
    b[0, 0] = (3, 4, 0); b[0, 1] = (0, 0, 1); b[1, 0] = (0, 0, 2); b[1, 1] = (np.nan, 0, 0)
    e = Q.errors(a, b, [1.0, 5.0])
    assert e["dist"][0].tolist() == [5, 1] and e["dist"][1, 0] == 2 and np.isnan(e["dist"][1, 1])
    assert e["frame"][0].tolist() == [3, 5] and np.isnan(e["frame"][1]).all()
    assert e["hits_kp"].tolist() == [1, 3] and e["hits_frame"].tolist() == [0, 1]
    assert e["sum_kp"][0] == 7 and np.isnan(e["sum_kp"][1])


# ---- left hands -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ji.MODELS)
def test_left_hands_are_the_x_flip_of_the_mirrored_poses(name):
    m, P = ji.model(name), ji.input_poses(name)
    for which in ((Q.FEATURE8, Q.SKELETON) if name != "chain3swap" else (Q.SKELETON,)):
        for com_poses in (False, True):
            t = Q.builtin(m, which)
            right = Q.keypoints(m, P, t, np.float32, com_poses=com_poses)["xyz"]
            left = Q.keypoints(m, mirror_ref.poses(P), t, np.float32, com_poses=com_poses, hands=np.ones(len(P), np.uint8))["xyz"]
            want = right.copy(); want.view(np.uint32)[..., 0] ^= np.uint32(0x80000000)
            assert np.array_equal(_bits(left), _bits(want)), (name, which, com_poses)


# ---- wrong restatements land far away ---------------------------------------------------------------------------------------------------------------------
def test_wrong_restatements_are_far_away(bench):
    m = ji.model("hand17")
    gt = bench["gtpose"][:64].astype(F)
    cams = bench["cam"][:64].astype(F).copy()
    rng = np.random.RandomState(5)
    q = np.array([0, 0, 0, 1.0]) + rng.normal(size=(64, 4)) * 0.05
    cams[:, 8:12] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F); cams[:, 5:8] = rng.uniform(-0.02, 0.02, (64, 3)).astype(F)
    depth = bench["depth"][:64]
    right = Q.keypoints(m, gt, Q.feature8(), np.float32, com_poses=False, cams=cams, depth=depth, near_tol=0.03, far_tol=0.02)
    ulp100 = 100 * 2.0 ** -23 * float(np.abs(right["xyz"]).max())
    rel = Q.keypoints(m, gt, Q.feature8(), np.float32, com_poses=False, wrong="rel")["xyz"]
    f_rel = float(np.abs(rel - right["xyz"]).max()) / ulp100
    tr = Q.keypoints(m, gt, Q.feature8(), np.float32, com_poses=False, cams=cams, depth=depth, near_tol=0.03, far_tol=0.02, wrong="trunc")
    f_tr = float(np.abs(tr["ixy"] - right["ixy"]).max()) / (100 * 2.0 ** -23 * float(np.abs(right["pix"]).max()))
    nc = Q.keypoints(m, gt, Q.feature8(), np.float32, com_poses=False, cams=cams, wrong="nocam")
    f_nc = float(np.abs(nc["pix"] - right["pix"]).max()) / (100 * 2.0 ** -23 * float(np.abs(right["pix"]).max()))
    print("wrong rel direction: %.0f x 100 ulp; truncation: %.0f x 100 ulp (of a pixel coordinate); forgotten camera pose: %.0f x 100 ulp" % (f_rel, f_tr, f_nc))
    assert f_rel > 1 and f_tr > 1 and f_nc > 1
    assert (tr["ixy"] != right["ixy"]).any() and (right["ixy"] >= 0).any()
