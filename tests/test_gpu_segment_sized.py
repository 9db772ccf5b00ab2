"""ht_segment_vr_sized on the device: HandSegmentVR (handtrack.h:280-344) cut at either tile side, on frames up to 640x480.

What a result is held to:
  * side 64: the bytes of ht_segment_vr on the same context, wherever that call takes the frame;
  * side 128: the camera is the device's OWN side-64 camera with focal doubled and principal (64,64), byte for byte (dstcam is the only place the side enters, and the
    side is a power of two), so the last-bit trig differences between the device library and glibc are judged once, by tests/test_segment.py's rule on the side-64 camera;
  * every tile pixel, at either side: the float32 numpy SampleD (tests/segment_ref.py, pinned to the reference's tiles by tests/test_segment_sized_ref.py) taken through
    the device's own returned camera -- no differing pixel allowed;
  * past 320x240: the camera against the C restatement (oracle_lib.segment_vr) to 2e-7 * max(1, |ec|), and the side-64 tiles against the restatement's: 0 differing pixels
    where the camera bytes agree, at most 8 otherwise (tests/test_segment.py's rule).
"""
import os

import numpy as np
import pytest
import torch

import oracle_lib
import segment_ref
from hand_tracking_samples_amd import native

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "segment6.npz"))
CASES = [(i, o) for i in range(6) for o in ([15, 1, 2, 4, 8, 5] if i < 2 else [15])]
OPTS = (15, 1, 2, 4, 8, 5)
WRANGE = (0.1, 0.70)


def blob_frames(n, w, h, seed):
    """tests/test_segment.py's synth_frames at any size: a tapered arm from a random border point to a disc-shaped hand, at varying depth, in front of a 4 m background."""
    rng = np.random.RandomState(seed)
    s = min(w / 320.0, h / 240.0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.full((n, h, w), 4000, np.uint16)
    for k in range(n):
        side = rng.randint(4)
        e = np.array([rng.uniform(0.125 * w, 0.875 * w), h - 1.0]) if side == 0 else np.array([rng.uniform(0.125 * w, 0.875 * w), 0.0]) if side == 1 else \
            np.array([w - 1.0, rng.uniform(0.125 * h, 0.875 * h)]) if side == 2 else np.array([0.0, rng.uniform(0.125 * h, 0.875 * h)])
        c = np.array([rng.uniform(0.28 * w, 0.72 * w), rng.uniform(0.29 * h, 0.71 * h)])
        z = rng.uniform(250, 640)
        r = rng.uniform(22, 48) * s
        hand = (xx - c[0]) ** 2 + (yy - c[1]) ** 2 < r * r
        t = np.clip(((xx - e[0]) * (c[0] - e[0]) + (yy - e[1]) * (c[1] - e[1])) / max(1e-3, ((c - e) ** 2).sum()), 0, 1)
        arm = (xx - (e[0] + t * (c[0] - e[0]))) ** 2 + (yy - (e[1] + t * (c[1] - e[1]))) ** 2 < (0.45 * r) ** 2
        depth = z + (0.15 * (xx - c[0]) + 0.1 * (yy - c[1])) / s + rng.uniform(-3, 3, size=xx.shape)
        m = hand | arm
        out[k][m] = np.clip(depth[m], 120, 3000).astype(np.uint16)
    cams = np.tile(np.array([305 * s, 305 * s, w / 2.0, h / 2.0, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32), (n, 1))
    return out, cams


def doubled(depth, cam):
    c = np.array(cam, np.float32).copy(); c[:4] *= 2
    return np.repeat(np.repeat(depth, 2, axis=0), 2, axis=1), c


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(os.path.join(HERE, "golden", "model_hand17.htfx"), max_batch=1)      # segmentation needs no weights and no tracker slot
    yield c
    c.close()


def check_batch(ctx, depth, cams, opt=0xF, wrange=WRANGE, restatement=True):
    """Both sides, each in one call over the whole batch; returns per frame (camera bytes equal the restatement's, pixels outside the source at side 64 / 128)."""
    B = len(depth)
    t64, c64 = ctx.segment_vr_sized(depth, cams, 64, opt, wrange)
    t128, c128 = ctx.segment_vr_sized(depth, cams, 128, opt, wrange)
    assert t64.shape == (B, 64, 64) and t128.shape == (B, 128, 128)
    assert c128.tobytes() == segment_ref.side128_camera(c64).tobytes()
    stats = []
    for k in range(B):
        r64, o64 = segment_ref.sample_d(depth[k], cams[k], c64[k], 64)
        r128, o128 = segment_ref.sample_d(depth[k], cams[k], c128[k], 128)
        assert (t64[k] != r64).sum() == 0, (k, 64, int((t64[k] != r64).sum()))
        assert (t128[k] != r128).sum() == 0, (k, 128, int((t128[k] != r128).sum()))
        same = None
        if restatement:
            et, ec, _, _ = oracle_lib.segment_vr(depth[k], cams[k], opt, wrange)
            assert np.abs(c64[k] - ec).max() <= 2e-7 * max(1.0, np.abs(ec).max()), (k, c64[k] - ec)
            e128 = segment_ref.side128_camera(ec)
            assert np.abs(c128[k] - e128).max() <= 2e-7 * max(1.0, np.abs(e128).max()), (k, c128[k] - e128)
            same = c64[k].tobytes() == ec.tobytes()
            assert (t64[k] != et).sum() <= (0 if same else 8), (k, int((t64[k] != et).sum()))
        stats.append((same, int(o64.sum()), int(o128.sum())))
    return stats


def test_side64_equals_the_unsized_call(ctx):
    for opt in OPTS:
        frames = [i for i, o in CASES if o == opt]
        depth = np.stack([FIX["s%d__depth" % i] for i in frames]); cams = np.stack([FIX["s%d__cam" % i] for i in frames])
        t0, c0 = ctx.segment_vr(depth, cams, opt, WRANGE)
        t1, c1 = ctx.segment_vr_sized(depth, cams, 64, opt, WRANGE)
        assert t1.tobytes() == t0.tobytes() and c1.tobytes() == c0.tobytes(), opt


def test_side128_on_the_golden_cases(ctx):
    for opt in OPTS:
        frames = [i for i, o in CASES if o == opt]
        depth = np.stack([FIX["s%d__depth" % i] for i in frames]); cams = np.stack([FIX["s%d__cam" % i] for i in frames])
        check_batch(ctx, depth, cams, opt, WRANGE, restatement=False)      # the side-64 camera against the reference's: tests/test_segment.py


def test_640x480_batch(ctx):
    gold = [doubled(FIX["s%d__depth" % i], FIX["s%d__cam" % i]) for i in range(6)]
    bd, bc = blob_frames(12, 640, 480, seed=5)
    depth = np.concatenate([np.stack([g[0] for g in gold]), bd]); cams = np.concatenate([np.stack([g[1] for g in gold]), bc])
    assert depth.shape == (18, 480, 640)
    stats = check_batch(ctx, depth, cams)
    assert any(s[1] > 0 for s in stats) and any(s[1] == 0 for s in stats), stats      # tiles with pixels outside the source and tiles without
    assert any(s[2] > 0 for s in stats) and any(s[2] == 0 for s in stats), stats
    assert sum(bool(s[0]) for s in stats) >= len(stats) * 3 // 4      # the rare 1-ulp differences of sin/cos/atan2 aside, cameras are identical (tests/test_segment.py)


def _edge_shapes():
    out = {}
    out["324x240"] = blob_frames(1, 324, 240, seed=11)      # the first size past the unsized calls' capacity
    d = np.full((1, 8, 8), 4000, np.uint16); d[0, 2:8, 1:7] = 400 + np.arange(36, dtype=np.uint16).reshape(6, 6)
    out["8x8"] = (d, np.array([[8, 8, 4, 4, 0.001, 0, 0, 0, 0, 0, 0, 1]], np.float32))
    out["2560x120"] = blob_frames(1, 2560, 120, seed=12)     # more quarter-size columns (640) than a block has threads
    out["120x2560"] = blob_frames(1, 120, 2560, seed=13)     # ... and rows
    cam = np.array([[610, 610, 320, 240, 0.001, 0, 0, 0, 0, 0, 0, 1]], np.float32)
    out["640x480 none in range"] = (np.full((1, 480, 640), 4000, np.uint16), cam)      # count == 0
    rng = np.random.RandomState(14)
    out["640x480 all in range"] = ((450 + rng.randint(0, 60, size=(1, 480, 640))).astype(np.uint16), cam)      # the longest compacted list: 19200 entries
    return out


EDGE = _edge_shapes()


@pytest.mark.parametrize("name", list(EDGE))
def test_shapes_at_which_the_kernel_can_go_wrong(ctx, name):
    depth, cams = EDGE[name]
    h, w = depth.shape[1:]
    assert native.segment_vr_supported(w, h, 64) and native.segment_vr_supported(w, h, 128)
    check_batch(ctx, depth, cams, 0xF, (0.1, 0.65))


def test_pass_through(ctx):
    d = (np.arange(2 * 16384, dtype=np.uint32) * 7 % 5000).astype(np.uint16).reshape(2, 128, 128)
    cams = np.tile(np.array([200, 200, 64, 64, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32), (2, 1)); cams[1, 0] = 210
    t, c = ctx.segment_vr_sized(d, cams, 128)
    assert np.array_equal(t, d) and c.tobytes() == cams.tobytes()      # handtrack.h:283-284 for the net's own size
    t64, c64 = ctx.segment_vr_sized(d, cams, 64)
    assert t64.shape == (2, 64, 64) and c64[0, 2] == 32.0 and c64[0, 3] == 32.0      # the same frame is segmented at the other side
    r, _ = segment_ref.sample_d(d[0], cams[0], c64[0], 64)
    assert np.array_equal(t64[0], r)
    d64 = np.ascontiguousarray(d[:, :64, :64])
    t, c = ctx.segment_vr_sized(d64, cams, 64)
    assert np.array_equal(t, d64) and c.tobytes() == cams.tobytes()
    t128, c128 = ctx.segment_vr_sized(d64, cams, 128)      # ... and a 64x64 frame at side 128
    assert t128.shape == (2, 128, 128) and c128[0, 2] == 64.0
    r, _ = segment_ref.sample_d(d64[0], cams[0], c128[0], 128)
    assert np.array_equal(t128[0], r)


def test_refusals_leave_the_context_usable(ctx):
    cam = np.array([[610, 610, 320, 240, 0.001, 0, 0, 0, 0, 0, 0, 1]], np.float32)
    for w, h, side in ((644, 480, 128), (642, 480, 128), (644, 480, 64), (642, 480, 64), (640, 480, 96), (320, 240, 0)):
        with pytest.raises(native.HTError):
            ctx.segment_vr_sized(np.zeros((1, h, w), np.uint16), cam, side)
    d = np.zeros((1, 480, 640), np.uint16); tiles = np.zeros((1, 128, 128), np.uint16); co = np.zeros((1, 12), np.float32)
    import ctypes as C
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, f32(cam), u16(tiles), f32(co)), (u16(d), None, u16(tiles), f32(co)), (u16(d), f32(cam), None, f32(co)), (u16(d), f32(cam), u16(tiles), None)):
        assert ctx.L.ht_segment_vr_sized(ctx.h, 128, args[0], args[1], 640, 480, 1, 0xF, 0.1, 0.65, 0.17, args[2], args[3]) == 1      # HT_ERR_ARG
    assert ctx.L.ht_segment_vr_sized_dev(ctx.h, 128, None, None, 640, 480, 1, 0xF, 0.1, 0.65, 0.17, None, None, None) == 1
    depth = FIX["s0__depth"][None]; cams = FIX["s0__cam"][None]
    check_batch(ctx, depth, cams, 0xF, WRANGE, restatement=False)


def test_dev_form_on_a_side_stream_equals_the_host_form(ctx):
    depth, cams = blob_frames(3, 640, 480, seed=21)
    dev = torch.device("cuda:0")
    td = torch.from_numpy(depth.view(np.int16)).to(dev); tc = torch.from_numpy(cams).to(dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    for side in (64, 128):
        tt = torch.zeros((3, side, side), dtype=torch.int16, device=dev); tco = torch.zeros((3, 12), dtype=torch.float32, device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        ctx.segment_vr_sized_dev(side, td.data_ptr(), tc.data_ptr(), 640, 480, 3, tt.data_ptr(), tco.data_ptr(), s.cuda_stream)
        s.synchronize()
        want_t, want_c = ctx.segment_vr_sized(depth, cams, side)
        assert np.array_equal(tt.cpu().numpy().view(np.uint16), want_t) and tco.cpu().numpy().tobytes() == want_c.tobytes()
