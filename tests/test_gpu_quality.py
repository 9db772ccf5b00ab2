"""GPU: the accuracy calls against tests/quality_ref.py, which tests/test_quality_ref.py pins: keypoints (xyz, pixels, depth along the ray, visibility)
bit for bit, keypoint errors bit for bit with exact counts, depth comparison exactly, and the composite byte for byte against conversion -> ht_render_depth -> comparison.
Host and device forms, guard bytes around every output, second calls, refusals, and an update's bytes before and after."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import htfx
import joints_inputs as ji
import joints_ref as jr
import pose_frame
import quality_ref as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 64
FRAME_OF_B = {1: (8, 8), 3: (36, 20), 70: (320, 240)}


@pytest.fixture(scope="module")
def ctxs():
    from hand_tracking_samples_amd import native
    made = {}

    def get(name):
        if name not in made:
            made[name] = native.Context(ji.model_path(name) if name else None, 4)
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def bench():
    return np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_numbers(a, b):
    """bit for bit where the restatement has a number, NaN where it has a NaN (IEEE 754 leaves a NaN's sign and payload to the implementation)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


class Guarded:
    """a device buffer of `nbytes` with GUARD bytes of 0xA5 on either side, `off` bytes further in for the misaligned views"""

    def __init__(self, nbytes, off=0):
        self.n, self.off = nbytes, GUARD + off
        self.t = torch.full((nbytes + 2 * GUARD + off,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ptr = self.t.data_ptr() + self.off

    def read(self, dtype, shape):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert np.all(h[:self.off] == 0xA5) and np.all(h[self.off + self.n:] == 0xA5), "written beside the output"
        return h[self.off:self.off + self.n].copy().view(dtype).reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.t == 0xA5).all())


def _caller_table(m, rng):
    """64 entries over every bone, both conventions, offsets up to a few centimetres"""
    return (rng.integers(0, m.nb, 64).astype(np.int32), (rng.standard_normal((64, 3)) * 0.02).astype(np.float32), rng.integers(0, 2, 64).astype(np.int32))


def _scene(name, B, seed):
    """poses [B,nb,7] around the tests' input poses, cameras with a pose of their own and frames whose depths straddle the keypoints'"""
    rng = np.random.default_rng(seed)
    m, P = ji.model(name), ji.input_poses(name)
    poses = np.ascontiguousarray(P[np.arange(B) % len(P)])
    w, h = FRAME_OF_B[B]
    cams = np.zeros((B, 12), np.float32)
    cams[:, 0] = cams[:, 1] = 0.9 * w; cams[:, 2] = (w - 1) / 2.0; cams[:, 3] = (h - 1) / 2.0; cams[:, 4] = 0.001
    q = np.array([0, 0, 0, 1.0]) + rng.standard_normal((B, 4)) * 0.05
    cams[:, 8:12] = q / np.linalg.norm(q, axis=1, keepdims=True); cams[:, 5:8] = rng.uniform(-0.02, 0.02, (B, 3))
    zs = np.abs(poses[:, :, 2]).mean(axis=1)
    depth = np.clip(zs[:, None, None] * 1000 + rng.integers(-120, 120, (B, h, w)), 0, 65535).astype(np.uint16)
    hands = (rng.random(B) < 0.5).astype(np.uint8)
    if B > 1:
        hands[0], hands[1] = 0, 1
    return m, poses, cams, depth, hands


def _tables(name, m):
    t = [("skeleton", Q.SKELETON, Q.skeleton(m)), ("caller", None, _caller_table(m, np.random.default_rng(7)))]
    if name != "chain3swap":
        t.insert(0, ("feature8", Q.FEATURE8, Q.feature8()))
    return t


# ---- keypoints -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("name", ji.MODELS)
def test_keypoints_equal_the_restatement(ctxs, name, B):
    ctx = ctxs(name)
    m, poses, cams, depth, hands = _scene(name, B, 100 + B)
    h, w = depth.shape[1:]
    d_poses, d_cams, d_depth, d_hands = _dev(poses), _dev(cams), _dev(depth), _dev(hands)
    codes = set()
    for label, which, table in _tables(name, m):
        K = len(table[0])
        if which is not None:      # the built-in table is the restatement's
            got = ctx.keypoint_table(which)
            assert all(_same(g, np.asarray(t, g.dtype)) for g, t in zip(got, table)), label
        for com_poses in (False, True):
            for hd in (None, hands):
                want = Q.keypoints(m, poses, table, np.float32, com_poses=com_poses, hands=hd, cams=cams, depth=depth, near_tol=0.03, far_tol=0.02)
                assert np.all(want["zc"] != 0)      # no NaN payload is compared
                got = ctx.keypoints(poses, which if which is not None else table, com_poses=com_poses, hands=hd, cams=cams, depth=depth, near_tol=0.03, far_tol=0.02)
                for k in ("xyz", "pix", "zc", "vis"):
                    assert _same(got[k], want[k]), (label, com_poses, hd is not None, k)
                codes |= set(np.unique(want["vis"]).tolist())
                # the device form: guard bytes, a second call, and each optional output left out in turn
                sizes = dict(xyz=12 * B * K, pix=8 * B * K, zc=4 * B * K, vis=B * K)
                dt = dict(xyz=(np.float32, (B, K, 3)), pix=(np.float32, (B, K, 2)), zc=(np.float32, (B, K)), vis=(np.uint8, (B, K)))
                for skip in (None, "xyz", "pix", "zc", "vis", "cams") if (com_poses and hd is not None) else (None,):
                    out = {k: Guarded(v) for k, v in sizes.items()}
                    absent = {"cams": ("pix", "zc", "vis")}.get(skip, (skip,))
                    p = lambda k: None if k in absent else out[k].ptr
                    for _ in range(2):
                        ctx.keypoints_dev(d_poses.data_ptr(), B, which if which is not None else table, p("xyz"), p("pix"), p("zc"), p("vis"), com_poses=com_poses,
                                          d_hands=None if hd is None else d_hands.data_ptr(), d_cams=None if skip == "cams" else d_cams.data_ptr(),
                                          d_depth=None if skip in ("cams", "vis") else d_depth.data_ptr(), w=w, h=h, near_tol=0.03, far_tol=0.02)
                        for k in sizes:
                            if k in absent:
                                assert out[k].untouched(), (label, skip, k)
                            else:
                                assert _same(out[k].read(*dt[k]), want[k]), (label, skip, k)
    if name != "chain3swap":
        assert {Q.VISIBLE, Q.OCCLUDED, Q.NOTHING, Q.OUTSIDE} <= codes, codes
    else:
        assert {Q.OUTSIDE, Q.BEHIND} <= codes and (B != 3 or len(codes) == 5), codes      # the chain's made-up poses lie on both sides of the camera


@pytest.mark.parametrize("w,h", [(8, 8), (36, 20), (320, 240)])
def test_visibility_on_every_border(ctxs, w, h):
    """64 points of bone 0 (identity orientation at (0,0,1): X = (ox, oy, 1) exactly) whose u + 0.5 is 0, just below 0, w, a quarter below w and in between, on both axes"""
    ctx, m = ctxs("hand17"), ji.model("hand17")
    F = np.float32
    cx, cy = F((w - 1) / 2.0), F((h - 1) / 2.0)
    def edge(n, c):
        v = [F(-0.5) - c, np.nextafter(F(-0.5) - c, F(-1e9)), F(n) - F(0.5) - c, F(n) - F(0.75) - c, F(0), F(1.25), F(-1.75), F(n) - F(1.5) - c]      # all exact in fp32: c is a multiple of a half
        return np.array(v, F)
    xs, ys = edge(w, cx), edge(h, cy)
    off = np.array([[x, y, 0] for y in ys for x in xs], F)
    table = (np.zeros(64, np.int32), off, np.zeros(64, np.int32))
    poses = np.zeros((2, m.nb, 7), F); poses[..., 6] = 1; poses[:, :, 2] = 1
    cams = np.zeros((2, 12), F); cams[:, 0] = cams[:, 1] = 1; cams[:, 2] = cx; cams[:, 3] = cy; cams[:, 4] = 0.001; cams[:, 11] = 1
    rng = np.random.default_rng(w)
    depth = rng.integers(900, 1100, (2, h, w)).astype(np.uint16)
    want = Q.keypoints(m, poses, table, F, cams=cams, depth=depth, near_tol=0.05, far_tol=0.05)
    got = ctx.keypoints(poses, table, cams=cams, depth=depth, near_tol=0.05, far_tol=0.05)
    for k in ("xyz", "pix", "zc", "vis"):
        assert _same(got[k], want[k]), k
    v = want["vis"][0].reshape(8, 8)
    assert (v[:, 1] == Q.OUTSIDE).all() and (v[:, 2] == Q.OUTSIDE).all() and (v[1, :] == Q.OUTSIDE).all() and (v[2, :] == Q.OUTSIDE).all()      # just below 0, and w exactly
    assert (v[0, 0] != Q.OUTSIDE) and (v[3, 3] != Q.OUTSIDE) and want["ixy"][0].reshape(8, 8, 2)[0, 0].tolist() == [0, 0] and want["ixy"][0].reshape(8, 8, 2)[3, 3].tolist() == [w - 1, h - 1]
    assert set(np.unique(v).tolist()) >= {Q.VISIBLE, Q.OUTSIDE}


def test_built_in_tables_follow_scale(ctxs):
    from hand_tracking_samples_amd import native
    m = copy.copy(ji.model("hand17"))
    s = np.float32(1.15)
    m.p1, m.com = m.p1 * s, m.com * s
    ctx = native.Context(ji.HAND17, 2)
    try:
        ctx.scale(1.15)
        poses = ji.input_poses("hand17")[:3]
        for which in (Q.FEATURE8, Q.SKELETON):
            table = Q.builtin(m, which, scales=(1.15,))
            got = ctx.keypoint_table(which)
            assert all(_same(g, np.asarray(t, g.dtype)) for g, t in zip(got, table)), which
            for com_poses in (False, True):
                assert _same(ctx.keypoints(poses, which, com_poses=com_poses)["xyz"], Q.keypoints(m, poses, table, np.float32, com_poses=com_poses)["xyz"])
        assert np.abs(got[1]).max() > 0
    finally:
        ctx.close()


def _tracked(weights, before=None):
    """a fresh context, optionally some accuracy calls first, then one update of the four golden frames -> (ctx, user poses, depth, cams)"""
    from hand_tracking_samples_amd import native
    g = htfx.load(os.path.join(ji.GOLDEN, "golden8.htfx"))
    depth = np.stack([g["f%d/depth" % f].reshape(-1) for f in range(4)]); cams = np.stack([g["f%d/cam" % f] for f in range(4)])
    ctx = native.Context(ji.HAND17, 4)
    ctx.load_weights(weights); ctx.set_params(microforce=3.0, mainthreadpasses=3)
    if before:
        before(ctx, depth.reshape(4, 64, 64), cams)
    ctx.tracker_reset(np.stack([g["f%d/startpose" % f] for f in range(4)]))
    return ctx, ctx.update_sync(depth, cams), depth.reshape(4, 64, 64), cams


def test_keypoints_of_a_tracked_hand_and_the_update_is_untouched(weights):
    """The user poses an update returns and the centre-of-mass poses of its state place the same keypoints; and the update gives the bytes it gives on a context that never
    ran an accuracy call."""
    def before(ctx, depth, cams):
        p = ji.input_poses("hand17")[:4]
        ctx.keypoints(p, Q.SKELETON, cams=cams, depth=depth)
        x = ctx.keypoints(p, Q.FEATURE8, com_poses=True)["xyz"]
        ctx.keypoint_errors(x, x + np.float32(0.01), [0.02])
        ctx.depth_compare(depth, depth[::-1], 0, 650, 10)
        ctx.pose_depth_residual(p, cams, depth, 0, 650, 10, com_poses=True)
    plain, user0, depth, cams = _tracked(weights)
    try:
        ctx, user, _, _ = _tracked(weights, before)
        try:
            assert _same(user, user0)
            assert _same(ctx.get_state(0, 4), plain.get_state(0, 4)) and _same(ctx.get_state(1, 4), plain.get_state(1, 4))
            com = np.ascontiguousarray(ctx.get_state(0, 4)[..., :7])
            bound = 8 * 2.0 ** -24 * float(np.abs(com[..., :3]).max())      # tests/test_gpu_joints.py's, for the same statement
            for which in (Q.FEATURE8, Q.SKELETON):
                a = ctx.keypoints(user, which, cams=cams, depth=depth)
                b = ctx.keypoints(com, which, com_poses=True, cams=cams, depth=depth)
                worst = float(np.abs(a["xyz"] - b["xyz"]).max())
                print("table %d: user against centre-of-mass keypoints %.3e, bound %.3e" % (which, worst, bound))
                assert worst <= bound
            r = ctx.pose_depth_residual(user, cams, depth, 1, 650, 10)
            print("tracked hand against its frames: IoU", r["iou"], "mean |residual| m", r["mean_abs"])
            assert np.all(r["info"][:, 2] > 0)
        finally:
            ctx.close()
    finally:
        plain.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8, 22, 64])
@pytest.mark.parametrize("B", [1, 3, 70, 1000])
def test_keypoint_errors_equal_the_restatement(ctxs, B, K):
    ctx = ctxs("")      # no model needed
    rng = np.random.default_rng(B * 100 + K)
    a = rng.standard_normal((B, K, 3)).astype(np.float32) * np.float32(0.05)
    b = a + (rng.standard_normal((B, K, 3)) * 0.01 * rng.random((B, 1, 1)) * 3).astype(np.float32)
    if B >= 3:
        b[1] = a[1]                          # a frame of zeros
        b[B - 1, K - 1, 1] = np.nan          # rows with a NaN: the last frame's last keypoint, and one in the middle
        a[B // 2, 0, 0] = np.nan
    d_a, d_b = _dev(a), _dev(b)
    for T in (0, 1, 32):
        thr = np.sort(rng.random(T).astype(np.float32) * np.float32(0.06)) if T != 1 else np.array([0.02], np.float32)
        if T == 32:
            thr[0] = 0.0; thr[31] = np.inf
        want = Q.errors(a, b, thr)
        got = ctx.keypoint_errors(a, b, thr)
        out = dict(dist=Guarded(4 * B * K), frame=Guarded(8 * B), sum_kp=Guarded(8 * K), hits_kp=Guarded(8 * max(T, 1)), hits_frame=Guarded(8 * max(T, 1)))
        for _ in range(2):      # the summary is zeroed by the call, not by the caller
            ctx.keypoint_errors_dev(d_a.data_ptr(), d_b.data_ptr(), B, K, thr, out["dist"].ptr, out["frame"].ptr, out["sum_kp"].ptr, out["hits_kp"].ptr if T else None, out["hits_frame"].ptr if T else None)
            dev = dict(dist=out["dist"].read(np.float32, (B, K)), frame=out["frame"].read(np.float32, (B, 2)), sum_kp=out["sum_kp"].read(np.float64, (K,)))
            if T:
                dev["hits_kp"] = out["hits_kp"].read(np.int64, (T,)); dev["hits_frame"] = out["hits_frame"].read(np.int64, (T,))
            else:
                assert out["hits_kp"].untouched() and out["hits_frame"].untouched()
            for g in (got, dev):
                assert _same_numbers(g["dist"], want["dist"]) and _same_numbers(g["frame"], want["frame"]), (T, "dist / frame")
                if T:
                    assert np.array_equal(g["hits_kp"], want["hits_kp"]) and np.array_equal(g["hits_frame"], want["hits_frame"]), (T, g["hits_kp"], want["hits_kp"])
                nan = np.isnan(want["sum_kp"])
                assert np.array_equal(np.isnan(g["sum_kp"]), nan)
                assert np.all(np.abs(g["sum_kp"][~nan] - want["sum_kp"][~nan]) <= B * 2.0 ** -52 * np.abs(want["sum_kp"][~nan]))
        if T == 32:
            fin = ~np.isnan(want["dist"])
            assert want["hits_kp"][31] == fin.sum() and want["hits_kp"][0] == (want["dist"] == 0).sum()
    # a summary alone
    s = Guarded(8 * K)
    ctx.keypoint_errors_dev(d_a.data_ptr(), d_b.data_ptr(), B, K, (), None, None, s.ptr, None, None)
    got = s.read(np.float64, (K,)); want = Q.errors(a, b)["sum_kp"]; nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.all(np.abs(got[~nan] - want[~nan]) <= B * 2.0 ** -52 * np.abs(want[~nan]))


# ---- depth compare ---------------------------------------------------------------------------------------------------------------------------------------------
LO, HI = 200, 650


def _frames(w, h, B, rng, kind="random"):
    a = rng.integers(LO - 60, HI + 60, (B, h, w)).astype(np.uint16)
    b = np.where(rng.random((B, h, w)) < 0.5, a, rng.integers(LO - 60, HI + 60, (B, h, w))).astype(np.uint16)
    a.reshape(B, -1)[:, 0] = LO; b.reshape(B, -1)[:, 0] = HI - 1      # values at lo and hi - 1
    if w * h > 2:
        a.reshape(B, -1)[:, -1] = HI; b.reshape(B, -1)[:, -1] = LO - 1      # and just outside
    return a, b


def _compare_both_forms(ctx, a, b, lo, hi, tol, offsets=((0, 0),)):
    B, h, w = a.shape
    want = Q.depth_compare(a, b, lo, hi, tol)
    assert np.array_equal(ctx.depth_compare(a, b, lo, hi, tol)["info"], want), ("host form", w, h, B, tol)
    n = 2 * a.size
    for oa, ob in offsets:      # bytes into an allocation: 0 the widest load the width allows, 8, 4, and 2 (a view one pixel in: single pixels) for either input
        da = torch.zeros(n + 32, dtype=torch.uint8, device=DEV); da[oa:oa + n] = _dev(a)
        db = torch.zeros(n + 32, dtype=torch.uint8, device=DEV); db[ob:ob + n] = _dev(b)
        info = Guarded(64 * B)
        for _ in range(2):      # info is zeroed by the call
            ctx.depth_compare_dev(da.data_ptr() + oa, db.data_ptr() + ob, w, h, B, lo, hi, tol, info.ptr)
            assert np.array_equal(info.read(np.int64, (B, 8)), want), ("device form", w, h, B, tol, oa, ob)
    return want


OFFSETS = ((0, 0), (8, 0), (0, 8), (4, 4), (2, 0), (0, 2), (2, 2))


@pytest.mark.parametrize("w,h,B", [(1, 1, 1), (1, 1, 70), (7, 5, 1), (7, 5, 70), (36, 20, 1), (36, 20, 70), (76, 20, 1), (76, 20, 70), (320, 240, 3), (640, 480, 2)])
def test_depth_compare_equals_numpy(ctxs, w, h, B):
    """Widths for every load: 1 and 7 single pixels, 36 = 4 * 9 eight bytes, 76 = 4 * 19 eight bytes (and four at an offset of 4), 320 and 640 sixteen"""
    ctx = ctxs("")
    rng = np.random.default_rng(w * 1000 + h + B)
    a, b = _frames(w, h, B, rng)
    small = w * h * B <= 76 * 20 * 70
    want = _compare_both_forms(ctx, a, b, LO, HI, 25, OFFSETS if small else OFFSETS[:5:2])
    if w * h >= 35:
        assert np.all(want[:, 2] > 0) and np.all(want[:, 3] < want[:, 2]) and np.all(want[:, 6] > 25)
    for tol in (0, 65535):
        _compare_both_forms(ctx, a, b, LO, HI, tol)
    if small:
        _compare_both_forms(ctx, a, a, LO, HI, 0)                                        # identical
        _compare_both_forms(ctx, a, b, 0, 65536, 3)                                      # all foreground
        _compare_both_forms(ctx, a, b, 60000, 65536, 3)                                  # all background
        dis = np.where(np.arange(w * h).reshape(h, w) % 2 == 0, 1, 0).astype(np.uint16)
        w0 = _compare_both_forms(ctx, (a * dis).astype(np.uint16), (b * (1 - dis)).astype(np.uint16), LO, HI, 3)      # disjoint
        assert not w0[:, 2:].any()
        ext = a.copy(); ext.reshape(B, -1)[:, 0] = 0; e2 = b.copy(); e2.reshape(B, -1)[:, 0] = 65535
        w1 = _compare_both_forms(ctx, ext, e2, 0, 65536, 65535)                          # the largest difference there is
        assert np.all(w1[:, 6] == 65535)


# ---- the composite ---------------------------------------------------------------------------------------------------------------------------------------------
def _composite_case(ctx, m, poses, cams, depth, com_poses, d_small=None):
    B, h, w = depth.shape
    conv = Q.pose_to_render(m, poses, cams, np.float32, com_poses=com_poses)
    rendered = ctx.render_depth(conv, cams, w, h, 4.0)
    want = Q.depth_compare(depth, rendered, 1, 650, 12)
    got = ctx.pose_depth_residual(poses, cams, depth, 1, 650, 12, com_poses=com_poses, want_rendered=True)
    assert _same(got["rendered"], rendered) and np.array_equal(got["info"], want), ("host form", com_poses)
    assert np.array_equal(ctx.pose_depth_residual(poses, cams, depth, 1, 650, 12, com_poses=com_poses)["info"], want)
    d_p, d_c, d_d = _dev(poses), _dev(cams), _dev(depth)
    info, rend = Guarded(64 * B), Guarded(2 * depth.size)
    for with_frames in (False, True, False):
        ctx.pose_depth_residual_dev(d_p.data_ptr(), d_c.data_ptr(), d_d.data_ptr(), w, h, B, 1, 650, 12, info.ptr, rend.ptr if with_frames else None, com_poses=com_poses)
        assert np.array_equal(info.read(np.int64, (B, 8)), want), ("device form", com_poses, with_frames)
        if with_frames:
            assert _same(rend.read(np.uint16, (B, h, w)), rendered)
    return want


def test_poses_against_frames(ctxs, bench):
    ctx, m = ctxs("hand17"), ji.model("hand17")
    gt, cams, depth = bench["gtpose"][:4].astype(np.float32), bench["cam"][:4].astype(np.float32), bench["depth"][:4]
    assert Q.identity_cams(cams).all()
    # a smaller call first: what it leaves in the staging must not show
    ctx.pose_depth_residual(gt[:1], cams[:1], depth[:1, :8, :8].copy(), 1, 650, 12, com_poses=True)
    want = _composite_case(ctx, m, gt, cams, depth, True)
    print("ground truths against their tiles: IoU %s" % (want[:, 2] / (want[:, 0] + want[:, 1] - want[:, 2])))
    assert np.all(want[:, 2] > 100)      # the hand is there
    _composite_case(ctx, m, jr.to_user(m, gt, np.float32), cams, depth, False)
    # two frames seen by a camera with a pose of its own: the world poses are cam.pose * (pose in the camera)
    rng = np.random.default_rng(3)
    c2 = cams[:2].copy(); c2[:, 0] = c2[:, 1] = 40; c2[:, 2] = 17.5; c2[:, 3] = 9.5
    q = np.array([0, 0, 0, 1.0]) + rng.standard_normal((2, 4)) * 0.2
    c2[:, 8:12] = q / np.linalg.norm(q, axis=1, keepdims=True); c2[:, 5:8] = rng.uniform(-0.1, 0.1, (2, 3))
    world = pose_frame.mul(np.broadcast_to(c2[:, None, 5:12], gt[:2].shape), gt[:2])
    assert not Q.identity_cams(c2).any()
    seen = ctx.render_depth(gt[:2], c2, 36, 20, 4.0)      # what that camera sees, up to the rounding of the way there and back
    w2 = _composite_case(ctx, m, world, c2, seen, True)
    assert np.all(w2[:, 2] > 20) and np.all(w2[:, 2] >= 0.8 * w2[:, 0])
    _composite_case(ctx, m, jr.to_user(m, world, np.float32), c2, seen, False)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctxs):
    from hand_tracking_samples_amd import native
    ctx, m = ctxs("hand17"), ji.model("hand17")
    poses = ji.input_poses("hand17")[:2]
    cams = np.zeros((2, 12), np.float32); cams[:, :5] = (30, 30, 17.5, 9.5, 0.001); cams[:, 11] = 1
    depth = np.full((2, 20, 36), 500, np.uint16)
    good = ctx.keypoints(poses, Q.FEATURE8, cams=cams, depth=depth)
    bad_tables = [(np.array([17]), np.zeros((1, 3)), np.array([0])), (np.array([-1]), np.zeros((1, 3)), np.array([0])), (np.array([0]), np.array([[np.inf, 0, 0]]), np.array([0])),
                  (np.zeros(65, int), np.zeros((65, 3)), np.zeros(65, int)), (np.array([0]), np.zeros((1, 3)), np.array([2]))]
    for t in bad_tables:
        with pytest.raises(native.HTError):
            ctx.keypoints(poses, t)
    for tol in ((-0.01, 0.02), (0.03, float("nan")), (float("inf"), 0.02)):
        with pytest.raises(native.HTError, match="tol"):
            ctx.keypoints(poses, Q.FEATURE8, cams=cams, depth=depth, near_tol=tol[0], far_tol=tol[1])
    with pytest.raises(native.HTError, match="hand layouts"):
        ctxs("chain3swap").keypoints(ji.input_poses("chain3swap")[:1], Q.FEATURE8)
    with pytest.raises(native.HTError):
        ctx.keypoints(poses, 5)
    L, h = ctx.L, ctx.h
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)); i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    xyz = np.zeros((2, 8, 3), np.float32); info = np.zeros((2, 8), np.int64)
    assert L.ht_keypoints(h, fp(poses), 2, 8, 0, 0, None, None, None, None, None, None, 0, 0, 0, 0, fp(xyz), None, None, None) != 0 and b"flags" in L.ht_last_error(h)
    assert L.ht_keypoints(h, fp(poses), 2, 0, 0, 0, None, None, None, None, None, None, 0, 0, 0, 0, fp(xyz), fp(xyz), None, None) != 0 and b"need cams" in L.ht_last_error(h)
    assert L.ht_keypoints(h, fp(poses), 2, 0, 0, 0, None, None, None, None, None, None, 0, 0, 0, 0, fp(poses), None, None, None) != 0 and b"overlaps" in L.ht_last_error(h)
    assert L.ht_keypoints(h, fp(poses), 0, 0, 0, 0, None, None, None, None, None, None, 0, 0, 0, 0, fp(xyz), None, None, None) == 0 and not xyz.any()      # B = 0 does nothing
    for w_, h_ in ((0, 20), (36, 4097)):
        assert L.ht_depth_compare(h, u16(depth), u16(depth), w_, h_, 2, 0, 650, 0, i64(info)) != 0
    for lo, hi, tol in ((650, 650, 0), (700, 650, 0), (-1, 650, 0), (0, 65537, 0), (0, 650, -1), (0, 650, 65536)):
        assert L.ht_depth_compare(h, u16(depth), u16(depth), 36, 20, 2, lo, hi, tol, i64(info)) != 0, (lo, hi, tol)
        assert L.ht_pose_depth_residual(h, fp(poses), fp(cams), u16(depth), 36, 20, 2, 0, 4.0, lo, hi, tol, i64(info), None) != 0
    assert L.ht_pose_depth_residual(h, fp(poses), fp(cams), u16(depth), 36, 20, 2, 0, 0.0, 0, 650, 0, i64(info), None) != 0 and b"far" in L.ht_last_error(h)
    assert L.ht_depth_compare(h, u16(depth), u16(depth), 36, 20, 2, 0, 650, 0, C.cast(u16(depth), C.POINTER(C.c_int64))) != 0 and b"overlaps" in L.ht_last_error(h)
    for K, T in ((0, 1), (65, 1), (8, -1), (8, 33)):
        assert L.ht_keypoint_errors(h, fp(xyz), fp(xyz), 2, K, fp(xyz), T, None, None, None, None, None) != 0, (K, T)
    assert not info.any()
    again = ctx.keypoints(poses, Q.FEATURE8, cams=cams, depth=depth)
    assert all(_same(again[k], good[k]) for k in good)
    only_net = ctxs("")
    f17 = np.zeros((1, 17, 7), np.float32)
    for rc in (L.ht_keypoint_table(only_net.h, 0, None, None, None, None), L.ht_keypoints(only_net.h, fp(f17), 1, 0, 0, 0, None, None, None, None, None, None, 0, 0, 0, 0, fp(xyz), None, None, None),
               L.ht_pose_depth_residual(only_net.h, fp(f17), fp(cams), u16(depth), 36, 20, 1, 0, 4.0, 0, 650, 0, i64(info), None)):
        assert rc == 4 and b"without a hand model" in L.ht_last_error(only_net.h)      # HT_ERR_STATE
    assert np.array_equal(only_net.depth_compare(depth, depth, 0, 650, 0)["info"], Q.depth_compare(depth, depth, 0, 650, 0))      # these two need no model


def test_cxx_quality_example_runs_on_the_device(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "quality")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_quality_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "model_hand17.htfx")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
