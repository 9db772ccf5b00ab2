"""Left hands on the device: the mirror kernels against tests/mirror_ref.py byte for byte, and ht_update_hands_* against the call it is defined by.

A left-hand update is: mirror the frame, its camera and its start poses; run the existing update in the frame's slot; mirror the poses that come out.  So for every
flag vector ht_update_hands_sync(hands) must equal  mirror_ref -> ht_update_frames_sized_sync on that same mixed batch -> mirror_ref  bit for bit: poses, cnn_out (which
stays canonical), both models' state and the tracker flags, after each of two consecutive updates (the second carries the state).  Without flags the call is
ht_update_frames_sized_*: the same bytes, no mirror launch, no staging."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import htfx
import mirror_ref
import oracle_lib as ol
from hand_tracking_samples_amd import native, weights as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL26 = os.path.join(HERE, "golden", "model_hand26.htfx")
DEV = "cuda:0"


def _flag_vectors(B, rng):
    mixed = (rng.integers(0, 2, B) * 255).astype(np.uint8)      # any nonzero value is a left hand
    if B > 1:
        mixed[0], mixed[1] = 0, 7
    return [np.zeros(B, np.uint8), np.ones(B, np.uint8), mixed, None]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(ol.MODEL, 8)
    yield c
    c.close()


def _dev(a):
    """a numpy array as a device tensor of the same bytes"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


# ---- the mirror kernels ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (4, 4), (8, 4), (12, 8), (64, 64), (68, 12), (320, 240)])
def test_mirror_frames_equal_the_reference_bytes(ctx, w, h, B):
    """Every path of the frame kernel: 16 bytes a thread for (8,4) (64,64) (320,240), 8 for (4,4) (12,8) (68,12), 4 for an output two pixels into its allocation, and
    single pixels for views one pixel into an allocation, on input, on output and on both -- and for the odd widths (7,5) (1,1), whatever the alignment."""
    rng = np.random.default_rng(w * 1000 + h * 10 + B)
    depth = rng.integers(0, 65536, (B, h, w)).astype(np.uint16)
    n = depth.size
    d_in = _dev(depth)
    d_off_in = torch.zeros(2 * n + 16, dtype=torch.uint8, device=DEV); d_off_in[2:2 + 2 * n] = d_in      # the same frames one pixel into an allocation
    for hands in _flag_vectors(B, rng):
        want = mirror_ref.frames(depth, hands)
        assert ctx.mirror_frames(depth, hands).tobytes() == want.tobytes()
        d_hands = None if hands is None else _dev(hands)
        hp = 0 if hands is None else d_hands.data_ptr()
        for src, dst_off in ((d_in.data_ptr(), 0), (d_off_in.data_ptr() + 2, 0), (d_in.data_ptr(), 2), (d_off_in.data_ptr() + 2, 2), (d_in.data_ptr(), 4)):
            d_out = torch.full((2 * n + 16,), 0xA5, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize()      # the context runs on its own stream
            for _ in range(2):      # and so does a second call
                ctx.mirror_frames_dev(src, w, h, B, hp, d_out.data_ptr() + dst_off, None)
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()
                assert got[dst_off:dst_off + 2 * n].tobytes() == want.tobytes(), (hands, dst_off)
                assert np.all(got[:dst_off] == 0xA5) and np.all(got[dst_off + 2 * n:] == 0xA5)      # nothing beside the frames is written
        if hands is None or hands.all():      # mirrored twice: the original bytes
            assert ctx.mirror_frames(want, hands).tobytes() == depth.tobytes()


def _special_poses(B, per, rng):
    p = rng.standard_normal((B, per, 7)).astype(np.float32)
    p.reshape(-1)[::5] = 0.0; p.reshape(-1)[1::7] = -0.0
    p.view(np.uint32).reshape(-1)[3::11] = 0x7FC00001      # a NaN with a payload
    p.view(np.uint32).reshape(-1)[4::13] = 0xFFC00000      # and a negative one
    return p


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("per", [1, 17, 26])
def test_mirror_poses_in_place_with_zeros_and_nans(ctx, per, B):
    rng = np.random.default_rng(per * 100 + B)
    p = _special_poses(B, per, rng)
    fp = C.POINTER(C.c_float)
    for hands in _flag_vectors(B, rng):
        want = mirror_ref.poses(p, hands)
        assert ctx.mirror_poses(p, hands).tobytes() == want.tobytes()
        q = p.copy()      # the host form in place
        hp = None if hands is None else hands.ctypes.data_as(C.POINTER(C.c_uint8))
        assert ctx.L.ht_mirror_poses(ctx.h, q.ctypes.data_as(fp), per, B, hp, q.ctypes.data_as(fp)) == 0
        assert q.tobytes() == want.tobytes()
        d = _dev(p); d_hands = None if hands is None else _dev(hands)
        for k in range(2):      # the device form in place: once is the mirror, twice the original where every frame is flagged
            ctx.mirror_poses_dev(d.data_ptr(), per, B, 0 if hands is None else d_hands.data_ptr(), d.data_ptr(), None)
            torch.cuda.synchronize()
            if k == 0:
                assert _host(d, p).tobytes() == want.tobytes()
            elif hands is None or hands.all():
                assert _host(d, p).tobytes() == p.tobytes()
            else:
                assert _host(d, p).tobytes() == mirror_ref.poses(want, hands).tobytes()


@pytest.mark.parametrize("B", [1, 3, 70])
def test_mirror_cams_in_place(ctx, B):
    rng = np.random.default_rng(B)
    cams = rng.standard_normal((B, 12)).astype(np.float32)
    cams[:, 2] = rng.integers(0, 640, B) / 4.0      # principal points on quarter pixels
    cams[0, 5:] = _special_poses(1, 1, rng)[0, 0]
    for w in (64, 320, 640):
        for hands in _flag_vectors(B, rng):
            want = mirror_ref.cams(cams, w, hands)
            assert ctx.mirror_cams(cams, w, hands).tobytes() == want.tobytes()
            d = _dev(cams); d_hands = None if hands is None else _dev(hands)
            ctx.mirror_cams_dev(d.data_ptr(), w, B, 0 if hands is None else d_hands.data_ptr(), d.data_ptr(), None)
            torch.cuda.synchronize()
            assert _host(d, cams).tobytes() == want.tobytes()


def test_overlapping_frames_are_refused_and_empty_batches_do_nothing(ctx):
    depth = np.arange(3 * 8 * 8, dtype=np.uint16).reshape(3, 8, 8)
    d = torch.zeros(2 * depth.size * 2, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for off in (0, 2, depth.size * 2 - 2):      # equal, one pixel on, the last pixel still inside
        with pytest.raises(native.HTError, match="must not overlap"):
            ctx.mirror_frames_dev(d.data_ptr(), 8, 8, 3, 0, d.data_ptr() + off, None)
        with pytest.raises(native.HTError, match="must not overlap"):
            ctx.mirror_frames_dev(d.data_ptr() + off, 8, 8, 3, 0, d.data_ptr(), None)
    u16 = C.POINTER(C.c_uint16)
    assert ctx.L.ht_mirror_frames(ctx.h, depth.ctypes.data_as(u16), 8, 8, 3, None, depth.ctypes.data_as(u16)) == 1      # HT_ERR_ARG: the host form is not in place either
    ctx.mirror_frames_dev(d.data_ptr(), 8, 8, 3, 0, d.data_ptr() + depth.size * 2, None)      # side by side is fine
    ctx.mirror_frames_dev(d.data_ptr(), 8, 8, 0, 0, d.data_ptr(), None)                       # B = 0 does nothing, whatever the pointers
    torch.cuda.synchronize()
    assert ctx.mirror_frames(depth).tobytes() == mirror_ref.frames(depth).tobytes()          # the context still works


# ---- ht_update_hands_* against the existing call -------------------------------------------------------------------------------------------------------------
def _golden(name, n_key):
    G = htfx.load(os.path.join(HERE, "golden", name))
    n = len(G[n_key])
    return (np.ascontiguousarray(np.stack([G["f%d/depth" % f] for f in range(n)])), np.stack([G["f%d/cam" % f] for f in range(n)]).astype(np.float32),
            np.stack([G["f%d/startpose" % f] for f in range(n)]).astype(np.float32))


def _e2e128():
    G = htfx.load(os.path.join(HERE, "golden", "e2e128.htfx")); FR = np.load(os.path.join(HERE, "golden", "frames5_64.npz"))
    idx = [int(i) for i in G["frames"]]
    return np.ascontiguousarray(FR["depth"][idx]).reshape(len(idx), 128, 128), FR["cam"][idx].astype(np.float32), FR["startpose"][idx].astype(np.float32)


# fixture -> (frames, side, model): eight 64x64 tiles, two 320x240 frames for either net, four 128x128 frames that are their own segment
CASES = {"golden8": (lambda: _golden("golden8.htfx", "rows"), 64, ol.MODEL), "fullframe320": (lambda: _golden("fullframe320.htfx", "rows"), 64, ol.MODEL),
         "fullframe320close": (lambda: _golden("fullframe320close.htfx", "rows"), 128, ol.MODEL), "e2e128": (_e2e128, 128, MODEL26)}


@pytest.fixture(scope="module")
def trackers():
    """one context per model, both nets' seeded weights, the parameters of the fixtures' own tests"""
    w64, w128 = W.make_cnnb(), W.make_cnnb128()
    out = {}
    for model in (ol.MODEL, MODEL26):
        c = native.Context(model, 8)
        c.load_weights(w64); c.load_weights128(w128)
        c.set_params(microforce=3.0, mainthreadpasses=3)
        out[model] = c
    yield out
    for c in out.values():
        c.close()


def _snapshot(c, n, poses, cnn):
    return dict(poses=poses, cnn=cnn, hand=c.get_state(0, n), other=c.get_state(1, n), err=c.tracker_flags(n)[0], init=c.tracker_flags(n)[1])


def _same(a, b, what):
    for k in a:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (what, k)


@pytest.mark.parametrize("flags", ["all left", "alternating"])
@pytest.mark.parametrize("name", list(CASES))
def test_update_hands_is_mirror_update_mirror(trackers, name, flags):
    make, side, model = CASES[name]
    depth, cams, start = make()
    c = trackers[model]
    n, h, w = depth.shape
    hands = np.ones(n, np.uint8) if flags == "all left" else (np.arange(n) % 2).astype(np.uint8)
    seed = mirror_ref.poses(start, hands)      # a caller who seeds a left slot mirrors the poses first
    # the definition: the existing call on the mirrored batch
    want = []
    c.tracker_reset(seed)
    for _ in range(2):
        poses, cnn = c.update_frames_sized_sync(mirror_ref.frames(depth, hands), mirror_ref.cams(cams, w, hands), side, 0.17, want_cnn=True)
        assert c.frames_overflow() == 0
        want.append(_snapshot(c, n, mirror_ref.poses(poses, hands), cnn))
    assert np.isfinite(want[1]["poses"]).all() and want[0]["poses"].tobytes() != mirror_ref.poses(want[0]["poses"], hands).tobytes()
    # the host form
    c.tracker_reset(seed)
    for u in range(2):
        poses, cnn = c.update_hands_sync(depth, cams, hands, side, 0.17, want_cnn=True)
        assert c.frames_overflow() == 0
        _same(want[u], _snapshot(c, n, poses, cnn), (name, flags, "host form, update %d" % u))
    # the device form, re-seeded through d_start_poses (a left hand's own poses: they are mirrored on the way in)
    d_depth, d_cams, d_hands, d_start = _dev(depth), _dev(cams), _dev(hands), _dev(mirror_ref.poses(seed, hands))
    d_out = torch.zeros(n * c.nb * 7, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    c.update_hands_dev(side, d_depth.data_ptr(), d_cams.data_ptr(), w, h, 0.17, d_hands.data_ptr(), d_start.data_ptr(), n, d_out.data_ptr(), None)
    assert c.frames_overflow() == 0      # (waits for the stream)
    _, cnn, _ = c.cnn_results(n)
    _same(want[0], _snapshot(c, n, d_out.cpu().numpy().reshape(n, c.nb, 7), cnn), (name, flags, "device form"))


def test_without_flags_the_call_is_update_frames_sized(trackers):
    """The same bytes as ht_update_frames_sized_dev, no k_mirror_* launch in the profile, and the staging never allocated (a fresh context: ht_hands_capacity stays 0)."""
    depth, cams, start = _golden("fullframe320.htfx", "rows")
    n, h, w = depth.shape
    c = native.Context(ol.MODEL, 2)
    try:
        c.load_weights(W.make_cnnb()); c.set_params(microforce=3.0, mainthreadpasses=3)
        d_depth, d_cams, d_start = _dev(depth), _dev(cams), _dev(start)
        outs = []
        c.profile_enable(1)
        for hands_call in (False, True):
            d_out = torch.zeros(n * c.nb * 7, dtype=torch.float32, device=DEV)
            torch.cuda.synchronize()
            if hands_call:
                c.update_hands_dev(64, d_depth.data_ptr(), d_cams.data_ptr(), w, h, 0.17, 0, d_start.data_ptr(), n, d_out.data_ptr(), None)
            else:
                c.update_frames_sized_dev(64, d_depth.data_ptr(), d_cams.data_ptr(), w, h, 0.17, d_start.data_ptr(), n, d_out.data_ptr(), None)
            c.frames_overflow()
            outs.append((d_out.cpu().numpy(), c.get_state(0, n), c.get_state(1, n)) + tuple(c.tracker_flags(n)))
        for a, b in zip(*outs):
            assert a.tobytes() == b.tobytes()
        c.tracker_reset(start)
        assert c.update_hands_sync(depth, cams, None, 64, 0.17).tobytes() == outs[0][0].tobytes()      # the host form forwards too
        prof = c.profile_read()
        assert prof.get("solve", (0, 0))[1] > 0 and not any(k.startswith("k_mirror") and v[1] > 0 for k, v in prof.items()), prof
        assert c.hands_capacity() == 0
        # with flags the three kernels and the pose mirror are there, and the staging holds the frame
        c.update_hands_sync(depth, cams, np.ones(n, np.uint8), 64, 0.17)
        prof = c.profile_read()
        assert prof["k_mirror_frames"][1] == 1 and prof["k_mirror_cams"][1] == 1 and prof["k_mirror_poses"][1] == 1 and c.hands_capacity() == w * h
        c.reserve_hands(64, 64)
        assert c.hands_capacity() == w * h      # never smaller
    finally:
        c.close()


CAPTURE_CHILD = r'''
import os, sys
import numpy as np
import torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import htfx
from hand_tracking_samples_amd import native, weights as W
B = 4
G = htfx.load(os.path.join(%(root)r, "tests", "golden", "golden8.htfx"))
dev = torch.device("cuda:0")
c = native.Context(os.path.join(%(root)r, "tests", "golden", "model_hand17.htfx"), B)
c.load_weights(W.make_cnnb()); c.set_params(microforce=3.0, mainthreadpasses=3)
c.reserve_hands(64, 64)
assert c.hands_capacity() == 64 * 64
up = lambda key, dt: torch.from_numpy(np.stack([G["f%%d/%%s" %% (f, key)] for f in range(B)]).astype(dt).reshape(B, -1)).to(dev)
bufs = (up("depth", np.int16), up("cam", np.float32), up("startpose", np.float32), torch.tensor([0, 1, 1, 0], dtype=torch.uint8, device=dev),
        torch.empty((B, 17, 7), dtype=torch.float32, device=dev))
s = torch.cuda.Stream(dev)
def step(): c.update_hands_dev(64, bufs[0].data_ptr(), bufs[1].data_ptr(), 64, 64, 0.17, bufs[3].data_ptr(), bufs[2].data_ptr(), B, bufs[4].data_ptr(), s.cuda_stream)
with torch.cuda.stream(s):
    for _ in range(2): step()
torch.cuda.synchronize()
eager = bufs[4].clone()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, stream=s):
    step()
torch.cuda.synchronize()
for _ in range(2):
    bufs[4].zero_()
    g.replay(); torch.cuda.synchronize()
    assert bool(torch.isfinite(eager).all())
    assert torch.equal(bufs[4], eager), "replay differs from the direct call"
print("GRAPH-OK")
'''


def test_update_hands_survives_graph_capture():
    """As tests/test_gpu_graph.py captures ht_update_dev, in a child process (a capture that goes wrong dies inside the runtime): B = 4 tiles, mixed flags, replayed twice."""
    r = subprocess.run([sys.executable, "-c", CAPTURE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GRAPH-OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])


def test_refused_hand_updates_leave_the_context_usable():
    depth, cams, start = _golden("golden8.htfx", "rows")
    hands = (np.arange(8) % 2).astype(np.uint8)
    c = native.Context(ol.MODEL, 4)
    try:
        c.load_weights(W.make_cnnb()); c.set_params(microforce=3.0, mainthreadpasses=3)
        c.tracker_reset(start[:4])
        good = c.update_hands_sync(depth[:4], cams[:4], hands[:4], 64)
        with pytest.raises(native.HTError, match="capacity"):
            c.update_hands_sync(depth, cams, hands, 64)                                              # B > max_batch
        assert not native.segment_vr_supported(66, 66, 64)
        with pytest.raises(native.HTError, match="frame size"):
            c.update_hands_sync(np.zeros((4, 66, 66), np.uint16), cams[:4], hands[:4], 64)           # a shape ht_segment_vr_supported refuses
        with pytest.raises(native.HTError, match=r"128x128 net not loaded.*status 4"):
            c.update_hands_sync(np.zeros((4, 240, 320), np.uint16), cams[:4], hands[:4], 128)        # no weights for that side: HT_ERR_STATE
        with pytest.raises(native.HTError, match="side must be 64 or 128"):
            c.update_hands_sync(depth[:4], cams[:4], hands[:4], 96)
        d = torch.zeros(4 * 4096, dtype=torch.int16, device=DEV); dc = _dev(cams[:4]); dh = _dev(hands[:4]); do = torch.zeros(4 * 17 * 7, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        with pytest.raises(native.HTError, match="capacity"):
            c.update_hands_dev(64, d.data_ptr(), dc.data_ptr(), 64, 64, 0.17, dh.data_ptr(), 0, 5, do.data_ptr(), None)
        c.tracker_reset(start[:4])
        assert c.update_hands_sync(depth[:4], cams[:4], hands[:4], 64).tobytes() == good.tobytes()
    finally:
        c.close()
    net = native.Context(None, 2)      # a context that serves the net only
    try:
        with pytest.raises(native.HTError, match="without a hand model"):
            net.update_hands_sync(depth[:2], cams[:2], hands[:2], 64)
        with pytest.raises(native.HTError, match="without a hand model"):
            net.reserve_hands(64, 64)
        assert net.mirror_frames(depth[:2], hands[:2]).tobytes() == mirror_ref.frames(depth[:2], hands[:2]).tobytes()      # the mirror calls use no model
    finally:
        net.close()
