"""Two hands in one frame on the device: ht_split_hands against tests/split_ref.py byte for byte, and ht_update_two_hands_* against the calls it is
defined by.

A two-hand update is: split the frame (left hand mirrored), run the existing update on the 2B hand frames in slots 2i (right) and 2i + 1 (left), mirror the odd slots'
poses back.  So ht_update_two_hands_sync must equal  ht_split_hands(HT_SPLIT_MIRROR_LEFT) -> ht_update_frames_sized_sync -> mirror_ref  bit for bit: poses, cnn_out,
both models' state and the tracker flags, after each of two consecutive updates.  The scene is rendered: two hands far enough apart that the split of the composed frame
IS the two solo frames (asserted here, and on the host by tests/test_split_ref.py), so the same bytes also come from tracking each solo frame on its own."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import mirror_ref
import oracle_lib as ol
import split_ref as S
from hand_tracking_samples_amd import native, weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAR, HI = 4000, 650
SIZES = [(8, 8), (36, 20), (76, 20), (320, 240), (640, 480)]
# (max_step, min_pixels, flags): the depth test off and on, both flag bits
SETTINGS = [(65535, 1, 0), (40, 3, S.RIGHT_IS_LOW_X | S.MIRROR_LEFT), (65535, 2, S.MIRROR_LEFT), (25, 1, S.RIGHT_IS_LOW_X)]
KEYS = ("frames", "info", "n_components", "labels", "cams")


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(None, 2)      # no model, no weights: the split needs neither
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _blobs(w, h, n, rng):
    """n distinct frames of random blobs: cells in range at depths 200..649, some just out of range (650..699), the rest background"""
    W4, H4 = w // 4, h // 4
    out = []
    for i in range(n):
        coarse = rng.random((H4 // 3 + 2, W4 // 3 + 2)) < 0.45 + 0.1 * i      # blobs a few cells across, and single cells on top
        m = np.repeat(np.repeat(coarse, 3, axis=0), 3, axis=1)[:H4, :W4] ^ (rng.random((H4, W4)) < 0.08)
        cells = np.where(m, rng.integers(200, 700, (H4, W4)), 0)
        out.append(S.frame_of(cells, FAR, rng))
    return np.stack(out)


_REF = {}


def _ref(key, distinct, cams, lo, step, minpx, flags):
    """the restatement on the distinct frames of a batch, computed once per case"""
    k = (key, lo, step, minpx, flags)
    if k not in _REF:
        _REF[k] = S.split(distinct, lo, HI, FAR, max_step=step, min_pixels=minpx, flags=flags, cams=cams)
    return _REF[k]


def _tile(ref, B):
    n = len(ref["frames"])
    return {k: np.ascontiguousarray(v[np.arange(B) % n]) for k, v in ref.items()}


def _same(got, want, what):
    for k in KEYS:
        assert np.ascontiguousarray(got[k]).tobytes() == want[k].tobytes(), (what, k)


def _split_dev(ctx, d_in, in_off, d_cams, w, h, B, lo, step, minpx, flags, out_off, optional=True):
    """the device form into guarded buffers -> dict of host arrays; every output sits out_off bytes into an allocation filled with 0xA5"""
    n = B * w * h; cells = B * (w // 4) * (h // 4)
    sizes = dict(frames=4 * n, cams=B * 96, info=B * 64, n_components=B * 4, labels=2 * cells)
    off = dict(frames=out_off, cams=16, info=16, n_components=16, labels=16)
    buf = {k: torch.full((sizes[k] + 32,), 0xA5, dtype=torch.uint8, device=DEV) for k in sizes}
    torch.cuda.synchronize()      # the context runs on its own stream
    ptr = lambda k: buf[k].data_ptr() + off[k]
    got = None
    for _ in range(2):      # and so does a second call
        ctx.split_hands_dev(d_in.data_ptr() + in_off, d_cams.data_ptr() if optional else 0, w, h, B, lo, HI, step, minpx, FAR, flags, ptr("frames"), ptr("cams") if optional else 0, ptr("info"),
                            ptr("n_components") if optional else None, ptr("labels") if optional else None, None)
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in buf.items()}
        for k, v in host.items():
            used = sizes[k] if optional or k in ("frames", "info") else 0
            assert np.all(v[:off[k]] == 0xA5) and np.all(v[off[k] + used:] == 0xA5), ("written beside", k, in_off, out_off)      # nothing beside the outputs, nothing into what was not asked for
        now = {k: v[off[k]:off[k] + sizes[k]] for k, v in host.items()}
        assert got is None or all(now[k].tobytes() == got[k].tobytes() for k in now)
        got = now
    return got


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("w,h", SIZES)
def test_split_equals_the_restatement(ctx, w, h, B):
    """Seeded random blobs.  The device form on every load width: 16 bytes a thread where w % 8 == 0, 8 for the other widths or buffers 8 bytes into an allocation, 4 for
    outputs 4 bytes in, single pixels for views one pixel in (and then the label kernel reads pixel by pixel too)."""
    rng = np.random.default_rng(w * 1000 + h * 10 + B)
    distinct = _blobs(w, h, min(B, 3), rng)
    cams = rng.standard_normal((len(distinct), 12)).astype(np.float32); cams[:, 2] = rng.integers(0, w, len(distinct)) / 4.0
    depth = np.ascontiguousarray(distinct[np.arange(B) % len(distinct)]); bcams = np.ascontiguousarray(cams[np.arange(B) % len(distinct)])
    n = depth.size
    d_in = torch.zeros(2 * n + 32, dtype=torch.uint8, device=DEV); d_in[:2 * n] = _dev(depth)
    d_in2 = torch.zeros(2 * n + 32, dtype=torch.uint8, device=DEV); d_in2[2:2 + 2 * n] = _dev(depth)      # the same frames one pixel into an allocation
    d_cams = _dev(bcams)
    small = B * w * h <= 3 * 320 * 240
    for step, minpx, flags in (SETTINGS if small else SETTINGS[:2]):
        want = _tile(_ref((w, h, B), distinct, cams, 0, step, minpx, flags), B)
        if step == 65535 and minpx == 1:
            assert w * h < 100 or (want["info"][:, :, 0] > 0).any()      # there is something to split
        got = ctx.split_hands(depth, 0, HI, FAR, cams=bcams, max_step=step, min_pixels=minpx, flags=flags, want_labels=True)
        _same(got, want, ("host form", step, minpx, flags))
        for src, in_off, out_off in ((d_in, 0, 0), (d_in, 0, 8), (d_in, 0, 4), (d_in, 0, 2), (d_in2, 2, 0), (d_in2, 2, 2))[:6 if small else 1]:
            raw = _split_dev(ctx, src, in_off, d_cams, w, h, B, 0, step, minpx, flags, out_off)
            for k in KEYS:
                assert raw[k].tobytes() == want[k].tobytes(), ("device form", k, in_off, out_off, step, minpx, flags)
    # without the optional outputs: the same frames and info, nothing else written
    step, minpx, flags = SETTINGS[1]
    want = _tile(_ref((w, h, B), distinct, cams, 0, step, minpx, flags), B)
    raw = _split_dev(ctx, d_in, 0, d_cams, w, h, B, 0, step, minpx, flags, 0, optional=False)
    assert raw["frames"].tobytes() == want["frames"].tobytes() and raw["info"].tobytes() == want["info"].tobytes()
    got = ctx.split_hands(depth, 0, HI, FAR, max_step=step, min_pixels=minpx, flags=flags, want_n=False)
    assert sorted(got) == ["frames", "info"] and got["frames"].tobytes() == want["frames"].tobytes() and got["info"].tobytes() == want["info"].tobytes()


def _shapes():
    """quarter images of 160x120 cells: name -> (cells as depths, max_step, min_pixels)"""
    W4, H4 = 160, 120
    Y, X = np.indices((H4, W4))
    board = np.where((X + Y) % 2 == 0, 300, 400)
    specks = np.where((X % 3 == 0) & (Y % 3 == 0), 300 + (X + Y) % 50, 0)
    return {"spiral": (S.spiral(W4, H4) * 300, 65535, 1), "serpentine": (S.serpentine(W4, H4) * 300, 65535, 1), "checkerboard, depth test off": (board, 65535, 1),
            "checkerboard, depth test on": (board, 99, 1), "all foreground": (np.full((H4, W4), 500), 0, 1), "all background": (np.zeros((H4, W4), int), 65535, 1),
            "specks only": (specks, 65535, 1), "specks below min_pixels": (specks, 65535, 2), "a range from 301": (board, 65535, 1)}


@pytest.mark.parametrize("name", list(_shapes()))
def test_split_of_the_shapes_that_need_many_rounds_or_many_labels(ctx, name):
    """640x480: one component winding through the whole image (the label loops end, and are right, when links have to travel through thousands of cells), 19200 components of one
    cell, one of 19200, none.  The running time of the whole host call goes into the output."""
    cells, step, minpx = _shapes()[name]
    lo = 301 if name == "a range from 301" else 0
    depth = S.frame_of(cells, FAR, np.random.default_rng(3))[None]
    cams = np.arange(12, dtype=np.float32)[None]
    for flags in (0, 3):
        want = _ref(name, depth, cams, lo, step, minpx, flags)
        ctx.split_hands(depth, lo, HI, FAR, cams=cams, max_step=step, min_pixels=minpx, flags=flags)      # (warm: the staging exists)
        t0 = time.perf_counter()
        got = ctx.split_hands(depth, lo, HI, FAR, cams=cams, max_step=step, min_pixels=minpx, flags=flags, want_labels=True)
        dt = time.perf_counter() - t0
        print("%s, flags %d: %d components, host call %.2f ms" % (name, flags, int(got["n_components"][0]), dt * 1e3))
        _same(got, want, (name, flags))
    n = int(want["n_components"][0])
    assert n == {"spiral": 1, "serpentine": 1, "checkerboard, depth test off": 1, "checkerboard, depth test on": 19200, "all foreground": 1, "all background": 0, "specks only": 54 * 40,
                 "specks below min_pixels": 0, "a range from 301": 9600}[name]
    if name in ("spiral", "serpentine"):
        assert dt < 1.0      # a loop that did not end would not come back at all; one that crawls a cell a round is caught here


def test_overlap_is_refused_and_refused_calls_leave_the_context_usable(ctx):
    rng = np.random.default_rng(11)
    depth = _blobs(36, 20, 3, rng)
    want = S.split(depth, 0, HI, FAR)
    n2 = depth.size * 2
    d = torch.zeros(4 * n2, dtype=torch.uint8, device=DEV); d[:n2] = _dev(depth)
    info = torch.zeros(3 * 64, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    call = lambda src, dst, **kw: ctx.split_hands_dev(src, 0, kw.get("w", 36), kw.get("h", 20), kw.get("B", 3), kw.get("lo", 0), kw.get("hi", HI), 65535, kw.get("minpx", 1), kw.get("far", FAR), kw.get("flags", 0),
                                                      dst, 0, info.data_ptr(), None, None, None)
    p = d.data_ptr()
    for src, dst in ((p, p), (p, p + 2), (p, p + n2 - 2), (p + 2 * n2 - 2, p), (p + n2, p), (p + 2 * n2 - 2, p)):      # equal, a pixel on, the last pixel still inside; the input inside either half of the output
        with pytest.raises(native.HTError, match="must not overlap"):
            call(src, dst)
    for kw, msg in ((dict(w=38), "frame size"), (dict(w=4, h=4), "frame size"), (dict(w=644, h=480), "frame size"), (dict(lo=650), "range_lo"), (dict(lo=700), "range_lo"), (dict(far=649), "far"),
                    (dict(minpx=0), "min_pixels"), (dict(minpx=-5), "min_pixels"), (dict(flags=4), "flag"), (dict(flags=-1), "flag"), (dict(B=-1), "bad argument")):
        with pytest.raises(native.HTError, match=msg):
            call(p, p + n2, **kw)
    with pytest.raises(native.HTError, match="together"):
        ctx.split_hands_dev(p, p, 36, 20, 3, 0, HI, 65535, 1, FAR, 0, p + n2, 0, info.data_ptr(), None, None, None)      # cams without cams_out
    u16 = C.POINTER(C.c_uint16)
    assert ctx.L.ht_split_hands(ctx.h, depth.ctypes.data_as(u16), None, 36, 20, 3, 0, HI, 65535, 1, FAR, 0, depth.ctypes.data_as(u16), None, np.zeros(48, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), None, None) == 1
    call(p, p, B=0)      # B = 0 does nothing, whatever the pointers
    call(p, p + n2)      # side by side is fine; far == range_hi is allowed
    call(p, p + n2, far=HI)
    torch.cuda.synchronize()
    call(p, p + n2)
    torch.cuda.synchronize()
    assert d[n2:3 * n2].cpu().numpy().tobytes() == want["frames"].tobytes() and info.cpu().numpy().tobytes() == want["info"].tobytes()
    assert d[:n2].cpu().numpy().tobytes() == depth.tobytes()      # the input is only read
    _same(ctx.split_hands(depth, 0, HI, FAR, cams=np.zeros((3, 12), np.float32), want_labels=True), S.split(depth, 0, HI, FAR, cams=np.zeros((3, 12), np.float32)), "after the refusals")


# ---- the two-hand scene ---------------------------------------------------------------------------------------------------------------------------------------
W_, H_ = S.SCENE_W, S.SCENE_H
SPLIT = dict(range_lo=0, range_hi=S.SCENE_HI, far=S.SCENE_FAR, min_pixels=S.SCENE_MIN_PIXELS)


@pytest.fixture(scope="module")
def tracker():
    c = native.Context(ol.MODEL, 4)
    c.load_weights(W.make_cnnb()); c.set_params(microforce=3.0, mainthreadpasses=3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene(tracker):
    """B = 2 scenes: the poses [B][2][nb][7] (0 the hand at high x, 1 the one at low x), their solo frames [B][2][h][w] rendered on the device, the composed frames, the cameras"""
    poses = np.stack([S.scene_poses(k) for k in S.SCENES])
    cams = np.repeat(S.SCENE_CAM[None], 2, axis=0)
    solo = tracker.render_mesh_depth(poses.reshape(4, tracker.nb, 7), np.repeat(cams, 2, axis=0), W_, H_, far=4.0).reshape(2, 2, H_, W_)
    return dict(poses=poses, solo=solo, frames=np.minimum(solo[:, 0], solo[:, 1]), cams=cams)


def _roles(scene, flags):
    """which of a scene's two hands is the right one (slot 2i) and which the left (slot 2i + 1): the one at high x is the right hand unless HT_SPLIT_RIGHT_IS_LOW_X"""
    order = [1, 0] if flags & S.RIGHT_IS_LOW_X else [0, 1]
    return scene["poses"][:, order], scene["solo"][:, order]


def _seed(poses):
    """the slots' starting poses [2B][nb][7]: canonical, so the left hands' mirrored"""
    B = len(poses)
    return mirror_ref.poses(poses.reshape(2 * B, -1, 7), np.arange(2 * B) % 2)


def _snapshot(c, n, poses, cnn):
    return dict(poses=poses.reshape(n, c.nb, 7), cnn=cnn, hand=c.get_state(0, n), other=c.get_state(1, n), err=c.tracker_flags(n)[0], init=c.tracker_flags(n)[1])


def _same_track(a, b, what):
    for k in a:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (what, k)


def test_the_scene_splits_into_its_solo_frames(tracker, scene):
    for s in scene["solo"].reshape(4, H_, W_):
        assert s.max() == S.SCENE_FAR and (s < S.SCENE_HI).sum() > 2000
    assert all(S.separable(*s) for s in scene["solo"])
    for flags in (0, S.RIGHT_IS_LOW_X):
        _, solo = _roles(scene, flags)
        got = tracker.split_hands(scene["frames"], flags=flags, **SPLIT)
        assert np.all(got["n_components"] == 2) and np.all(got["info"][:, :, 0] > 300)
        assert got["frames"].tobytes() == solo.tobytes()
        _same(tracker.split_hands(scene["frames"], flags=flags | S.MIRROR_LEFT, cams=scene["cams"], want_labels=True, **SPLIT),
              S.split(scene["frames"], 0, S.SCENE_HI, S.SCENE_FAR, min_pixels=S.SCENE_MIN_PIXELS, flags=flags | S.MIRROR_LEFT, cams=scene["cams"]), "the scene against the restatement")


@pytest.mark.parametrize("flags", [0, S.RIGHT_IS_LOW_X])
def test_two_hand_update_is_split_update_mirror(tracker, scene, flags):
    c = tracker
    poses, solo = _roles(scene, flags)
    frames, cams = scene["frames"], scene["cams"]
    B, n = 2, 4
    seed = _seed(poses)
    odd = (np.arange(n) % 2).astype(np.uint8)
    # the definition: the mirrored split, the existing update on the 2B frames, the odd slots' poses mirrored back
    sp = c.split_hands(frames, flags=flags | S.MIRROR_LEFT, cams=cams, **SPLIT)
    want = []
    c.tracker_reset(seed)
    for _ in range(2):
        p, cnn = c.update_frames_sized_sync(sp["frames"].reshape(n, H_, W_), sp["cams"].reshape(n, 12), 64, 0.17, want_cnn=True)
        assert c.frames_overflow() == 0
        want.append(_snapshot(c, n, mirror_ref.poses(p, odd), cnn))
    assert np.isfinite(want[1]["poses"]).all() and want[0]["poses"].tobytes() != want[1]["poses"].tobytes()
    # the fused call
    c.tracker_reset(seed)
    for u in range(2):
        p, info, cnn = c.update_two_hands_sync(frames, cams, side=64, segment_scale=0.17, flags=flags, want_cnn=True, **SPLIT)
        assert c.frames_overflow() == 0 and info.tobytes() == sp["info"].tobytes()
        _same_track(want[u], _snapshot(c, n, p, cnn), ("fused, update %d" % u, flags))
    # HT_SPLIT_MIRROR_LEFT is implied: giving it changes nothing
    c.tracker_reset(seed)
    p, info, cnn = c.update_two_hands_sync(frames, cams, side=64, segment_scale=0.17, flags=flags | S.MIRROR_LEFT, want_cnn=True, **SPLIT)
    _same_track(want[0], _snapshot(c, n, p, cnn), ("fused with the mirror bit", flags))
    # the unmirrored split through ht_update_hands_sync with flags 0, 1, 0, 1
    un = c.split_hands(frames, flags=flags, cams=cams, **SPLIT)
    c.tracker_reset(seed)
    for u in range(2):
        p, cnn = c.update_hands_sync(un["frames"].reshape(n, H_, W_), un["cams"].reshape(n, 12), odd, 64, 0.17, want_cnn=True)
        _same_track(want[u], _snapshot(c, n, p, cnn), ("split, then the flagged update, update %d" % u, flags))
    # each solo frame on its own: the frames the scene was composed of, never split
    c.tracker_reset(seed)
    for u in range(2):
        p, cnn = c.update_hands_sync(solo.reshape(n, H_, W_), np.repeat(cams, 2, axis=0), odd, 64, 0.17, want_cnn=True)
        _same_track(want[u], _snapshot(c, n, p, cnn), ("solo frames, update %d" % u, flags))
    # the device form, re-seeded through d_start_poses (in the camera's space: the left hands' own poses)
    c.tracker_reset(np.zeros_like(seed) + np.array([0, 0, 0, 0, 0, 0, 1], np.float32))
    d_frames, d_cams, d_start = _dev(frames), _dev(cams), _dev(poses)
    d_out = torch.zeros(n * c.nb * 7, dtype=torch.float32, device=DEV); d_info = torch.zeros(B * 16, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    c.update_two_hands_dev(64, d_frames.data_ptr(), d_cams.data_ptr(), W_, H_, 0.17, 0, S.SCENE_HI, 65535, S.SCENE_MIN_PIXELS, S.SCENE_FAR, flags, d_start.data_ptr(), B, d_out.data_ptr(), d_info.data_ptr(), None)
    assert c.frames_overflow() == 0      # (waits for the stream)
    _, cnn, _ = c.cnn_results(n)
    _same_track(want[0], _snapshot(c, n, d_out.cpu().numpy(), cnn), ("device form", flags))
    assert d_info.cpu().numpy().tobytes() == sp["info"].tobytes()
    c.tracker_reset(seed)      # and without d_info and d_start_poses
    c.update_two_hands_dev(64, d_frames.data_ptr(), d_cams.data_ptr(), W_, H_, 0.17, 0, S.SCENE_HI, 65535, S.SCENE_MIN_PIXELS, S.SCENE_FAR, flags, None, B, d_out.data_ptr(), None, None)
    assert c.frames_overflow() == 0
    _same_track(want[0], _snapshot(c, n, d_out.cpu().numpy(), c.cnn_results(n)[1]), ("device form, optional arguments left out", flags))


@pytest.mark.parametrize("flags", [0, S.RIGHT_IS_LOW_X])
def test_a_removed_hand_is_absent_and_the_other_is_tracked_as_before(tracker, scene, flags):
    c = tracker
    poses, solo = _roles(scene, flags)
    seed = _seed(poses)
    c.tracker_reset(seed)
    both, info = c.update_two_hands_sync(scene["frames"], scene["cams"], flags=flags, **SPLIT)
    assert np.all(info[:, :, 0] > 0)
    for gone in (0, 1):
        c.tracker_reset(seed)
        p, info = c.update_two_hands_sync(np.ascontiguousarray(solo[:, 1 - gone]), scene["cams"], flags=flags, **SPLIT)
        assert np.all(info[:, gone, 0] == 0) and np.all(info[:, gone, 1] == 0xFFFF) and np.all(info[:, 1 - gone, 0] > 300)
        assert p[:, 1 - gone].tobytes() == both[:, 1 - gone].tobytes()
        assert c.frames_overflow() == 0


def test_refusals_and_no_side_effects(tracker, scene):
    c = tracker
    frames, cams = scene["frames"], scene["cams"]
    poses, solo = _roles(scene, 0)
    seed = _seed(poses)
    odd = (np.arange(4) % 2).astype(np.uint8)

    def existing():
        c.tracker_reset(seed)
        a = c.update_hands_sync(solo.reshape(4, H_, W_), np.repeat(cams, 2, axis=0), odd, 64, 0.17, want_cnn=True)
        c.tracker_reset(seed)
        b = c.update_frames_sized_sync(solo.reshape(4, H_, W_), np.repeat(cams, 2, axis=0), 64, 0.17, want_cnn=True)
        return [x.tobytes() for x in a + b] + [c.get_state(0, 4).tobytes(), c.get_state(1, 4).tobytes()]

    before = existing()
    c.tracker_reset(seed)
    good, _ = c.update_two_hands_sync(frames, cams, **SPLIT)
    three = np.repeat(frames[:1], 3, axis=0); cams3 = np.repeat(cams[:1], 3, axis=0)
    with pytest.raises(native.HTError, match="2 \\* B exceeds"):
        c.update_two_hands_sync(three, cams3, **SPLIT)      # six slots of four
    d = _dev(three); dc = _dev(cams3); do = torch.zeros(6 * c.nb * 7, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(native.HTError, match="2 \\* B exceeds"):
        c.update_two_hands_dev(64, d.data_ptr(), dc.data_ptr(), W_, H_, 0.17, 0, S.SCENE_HI, 65535, 50, S.SCENE_FAR, 0, None, 3, do.data_ptr(), None, None)
    for kw, msg in ((dict(range_lo=650), "range_lo"), (dict(far=600), "far"), (dict(min_pixels=0), "min_pixels"), (dict(flags=8), "flag")):
        with pytest.raises(native.HTError, match=msg):
            c.update_two_hands_sync(frames, cams, **dict(SPLIT, **kw))
    with pytest.raises(native.HTError, match="frame size"):
        c.update_two_hands_sync(np.zeros((2, 66, 66), np.uint16), cams, **SPLIT)
    with pytest.raises(native.HTError, match="side must be 64 or 128"):
        c.update_two_hands_sync(frames, cams, side=96, **SPLIT)
    with pytest.raises(native.HTError, match=r"128x128 net not loaded.*status 4"):
        c.update_two_hands_sync(frames, cams, side=128, **SPLIT)
    c.tracker_reset(seed)
    assert c.update_two_hands_sync(frames, cams, **SPLIT)[0].tobytes() == good.tobytes()      # the context still works
    assert existing() == before      # and the existing calls give the bytes they gave before any two-hand call
    net = native.Context(None, 4)      # a context that serves the net only
    try:
        with pytest.raises(native.HTError, match="without a hand model"):
            net.update_two_hands_sync(frames, cams, **SPLIT)
        assert net.split_hands(frames, **SPLIT)["frames"].tobytes() == solo.tobytes()      # the split uses no model
    finally:
        net.close()


def test_cxx_split_example_runs_on_the_device(tmp_path):
    """SplitHands and TwoHandTracker of include/ht_handtrack.hpp on two rectangles: the split's counts, the mirrored left frame, presence flags, both flag settings"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "split"); cnnb = str(tmp_path / "w.cnnb")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(root, "tests", "cxx_split_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    W.save_cnnb(cnnb, W.make_cnnb())
    r = subprocess.run([exe, ol.MODEL, cnnb], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "split components 2 right 30 cells at 10 left 32 cells at 1 mirrored pixel 400" in r.stdout
    assert "update without weights" in r.stdout and "update right 30 cells left 32 cells poses 17 17" in r.stdout and "one hand: right 0 left 1" in r.stdout
