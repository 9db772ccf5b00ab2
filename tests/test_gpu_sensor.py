"""GPU: the sensor filters (ht_sensor_filter*, ht_sensor_background*; csrc/ht_sensor.hip) equal the restatement of RSCam's filters (tests/sensor_ref.py,
read against the reference's include/dcam.h:157-226) bit for bit, on frames on which a per-pixel kernel is wrong (tests/sensor_frames.py,
tests/test_sensor_ref.py), refuse what the contract refuses, and feed the tracker on one stream."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sensor_frames as F
import sensor_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL = os.path.join(HERE, "golden", "model_hand17.htfx")
CAM = np.array([305, 305, 160, 120, 0.001, 0.01, -0.02, 0.03, 0, 0, 0, 1], np.float32)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from hand_tracking_samples_amd import native
    c = native.Context(MODEL, 4)
    yield c
    c.close()


def _cams(B, scale=0.001):
    c = np.tile(CAM, (B, 1)); c[:, 4] = scale; c[:, 0] += np.arange(B, dtype=np.float32)
    return c


def _ds4_ref(D, I, bg=None):
    return np.stack([R.filter_ds4(D[b], I[b], None if bg is None else bg[b], max_width=D.shape[2]) for b in range(len(D))])


@pytest.mark.parametrize("family", sorted(F.FAMILIES))
@pytest.mark.parametrize("w,h,B", [(4, 4, 3), (16, 12, 3), (68, 12, 3), (76, 20, 3), (320, 240, 3), (16, 12, 70)])
def test_ds4_equals_the_sequential_loop(ctx, family, w, h, B):
    """4x4 has no interior, 16x12 is less than a wave's lanes, 68x12 just over, 76x20 leaves the last lanes without pixels and the lane before them with one;
    70 frames are more blocks than some launches' first round; with and without a background model"""
    from hand_tracking_samples_amd import native
    D, I = F.batch(family, w, h, B)
    cams = _cams(B)
    got, co = ctx.sensor_filter(native.SENSOR_DS4, D, cams, ir=I, max_width=max(w, 16))
    assert co.tobytes() == cams.tobytes()
    assert np.array_equal(got, _ds4_ref(D, I))
    bg = F.background_for(D, w)
    got, _ = ctx.sensor_filter(native.SENSOR_DS4, D, cams, ir=I, background=bg, max_width=w)
    want = _ds4_ref(D, I, bg)
    assert np.array_equal(got, want) and (want != _ds4_ref(D, I)).any()
    again, _ = ctx.sensor_filter(native.SENSOR_DS4, D, cams, ir=I, background=bg, max_width=w)
    assert again.tobytes() == got.tobytes()


def test_ds4_cascades_cross_every_lane_of_a_320x240_frame(ctx):
    """the frames on which one dark pixel at x = 2 (y = 2) decides the last interior pixel of its row (column): no missing carry can pass"""
    from hand_tracking_samples_amd import native
    frames = []
    for make, axis in ((F.cascade_rows, 1), (F.cascade_cols, 0)):
        d, ir = make(320, 240)
        dark = ir.copy()
        if axis == 1:
            dark[2:-2, 2] = 0
        else:
            dark[2, 2:-2] = 0
        frames += [(d, ir), (d, dark)]
    D = np.stack([f[0] for f in frames]); I = np.stack([f[1] for f in frames])
    want = _ds4_ref(D, I)
    assert (want[0] != want[1])[2:-2, -6:-2].any(axis=1).all() and (want[2] != want[3])[-6:-2, 2:-2].any(axis=0).all()
    got, _ = ctx.sensor_filter(native.SENSOR_DS4, D, _cams(4), ir=I)
    assert np.array_equal(got, want)


def test_ds4_on_device_buffers_and_a_callers_stream(ctx):
    from hand_tracking_samples_amd import native
    D, I = F.batch("staircase", 76, 20, 3)
    bg = F.background_for(D, 1)
    dev = torch.device("cuda:0")
    td = torch.from_numpy(D.view(np.int16)).to(dev); ti = torch.from_numpy(I).to(dev); tb = torch.from_numpy(bg.view(np.int16)).to(dev); tc = torch.from_numpy(_cams(3)).to(dev)
    to = torch.zeros((3, 20, 76), dtype=torch.int16, device=dev); tco = torch.zeros((3, 12), dtype=torch.float32, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    ctx.sensor_filter_dev(native.SENSOR_DS4, td.data_ptr(), ti.data_ptr(), tc.data_ptr(), 76, 20, 3, 320, tb.data_ptr(), to.data_ptr(), tco.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(to.cpu().numpy().view(np.uint16), _ds4_ref(D, I, bg)) and np.array_equal(tco.cpu().numpy(), _cams(3))


def test_refusals_and_the_empty_batch(ctx):
    from hand_tracking_samples_amd import native
    L, h = ctx.L, ctx.h
    d = np.full((2, 8, 16), 700, np.uint16); ir = np.full((2, 8, 16), 100, np.uint8); cams = _cams(2); out = np.full((2, 8, 16), 7, np.uint16); co = np.full((2, 12), 7, np.float32)
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)); u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)); fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ok = dict(kind=1, depth=u16(d), ir=u8(ir), cams=fp(cams), w=16, h=8, B=2, mw=320, bg=None, out=u16(out), co=fp(co))
    call = lambda **kw: (lambda a: L.ht_sensor_filter(h, a["kind"], a["depth"], a["ir"], a["cams"], a["w"], a["h"], a["B"], a["mw"], a["bg"], a["out"], a["co"]))(dict(ok, **kw))
    bad = [dict(mw=15), dict(mw=0), dict(out=u16(d)), dict(depth=None), dict(ir=None), dict(cams=None), dict(out=None), dict(co=None), dict(w=0), dict(h=4097), dict(B=-1), dict(kind=2),
           dict(kind=0, bg=u16(out)), dict(kind=0, mw=5), dict(kind=0, w=10, h=8, mw=3)]      # Ivy: a background; 16 -> 4 needs k = 2, fine; 10 wide is not divisible by 4
    for kw in bad:
        want = 0 if kw == dict(kind=0, mw=5) else 1
        assert call(**kw) == want, kw
        if want:
            assert "ht_sensor_filter" in L.ht_last_error(h).decode()
    assert (out.reshape(-1)[:16] == 700).all() and (out.reshape(-1)[16:] == 7).all()      # only the accepted Ivy call (two frames 16x8 -> 4x2) wrote
    out[:] = 7; co[:] = 7
    assert call(B=0) == 0 and call(B=0, kind=0, ir=None) == 0 and (out == 7).all() and (co == 7).all()
    # the device forms refuse the same before anything is launched
    assert L.ht_sensor_filter_dev(h, 1, 256, 512, 1024, 16, 8, 2, 15, None, 4096, 8192, None) == 1
    assert L.ht_sensor_filter_dev(h, 1, 256, 512, 1024, 16, 8, 2, 320, None, 256 + 100, 8192, None) == 1      # overlapping
    assert L.ht_sensor_filter_dev(h, 1, 256, None, 1024, 16, 8, 2, 320, None, 4096, 8192, None) == 1
    assert L.ht_sensor_background(h, None, 16, 8, 2, 3, 1, u16(out)) == 1 and L.ht_sensor_background(h, u16(d), 16, 8, 2, 3, 1, None) == 1
    assert L.ht_sensor_background(h, u16(d), 16, 8, 0, 3, 1, u16(out)) == 0 and (out == 7).all()
    with pytest.raises(native.HTError, match="wider than max_width"):
        ctx.sensor_filter(native.SENSOR_DS4, d, cams, ir=ir, max_width=8)
    got, _ = ctx.sensor_filter(native.SENSOR_DS4, d, cams, ir=ir)      # the context stays usable
    assert (got == 700).all()


@pytest.mark.parametrize("w,h,mw,k,scale", [(640, 480, 320, 1, 0.001), (640, 480, 320, 1, 0.000125), (1280, 960, 320, 2, 0.001), (320, 240, 320, 0, 0.0001), (320, 240, 320, 0, 0.00005),
                                            (36, 20, 9, 2, 0.001), (36, 20, 9, 2, 0.000125), (36, 20, 9, 2, 0.0001), (36, 20, 9, 2, 0.00005)])
def test_ivy_equals_the_halving_loop_and_the_fill(ctx, w, h, mw, k, scale):
    """frames with zeros both where the halving keeps them and where it drops them; cameras bit for bit; 0.00005 wraps the fill past 16 bits"""
    from hand_tracking_samples_amd import native
    rng = np.random.default_rng(w + k)
    B = 2
    D = (rng.integers(0, 4, (B, h, w)) > 0).astype(np.uint16) * rng.integers(1, 60000, (B, h, w)).astype(np.uint16)
    cams = _cams(B, scale)
    got, co = ctx.sensor_filter(native.SENSOR_IVY, D, cams, max_width=mw)
    assert got.shape == (B, h >> k, w >> k)
    for b in range(B):
        want, wc = R.filter_ivy(D[b], cams[b], mw)
        assert np.array_equal(got[b], want) and co[b].tobytes() == wc.tobytes()
        assert (want == R.ivy_fill(scale)).sum() >= (D[b][::1 << k, ::1 << k] == 0).sum() > 0


def test_ivy_refuses_a_width_the_halving_cannot_divide(ctx):
    from hand_tracking_samples_amd import native
    with pytest.raises(native.HTError, match="ht_sensor_filter"):
        ctx.sensor_filter(native.SENSOR_IVY, np.zeros((1, 480, 642), np.uint16), _cams(1))


def test_background_model_twice_then_ds4(ctx):
    from hand_tracking_samples_amd import native
    D, I = F.batch("blob", 76, 20, 3)
    D2, _ = F.batch("blob", 76, 20, 3, seed0=500)
    D2[0, 0, :3] = (0, 2, 3)      # dp < fudge wraps
    bg1 = ctx.sensor_background(D, None, 3)
    want1 = np.stack([R.add_background(None, D[b], 3) for b in range(3)])
    assert np.array_equal(bg1, want1)
    bg2 = ctx.sensor_background(D2, bg1, 5)
    want2 = np.stack([R.add_background(want1[b], D2[b], 5) for b in range(3)])
    assert np.array_equal(bg2, want2) and (want2 != want1).any() and np.array_equal(bg1, want1)
    got, _ = ctx.sensor_filter(native.SENSOR_DS4, D, _cams(3), ir=I, background=bg2)
    want = _ds4_ref(D, I, want2)
    assert np.array_equal(got, want) and (want != _ds4_ref(D, I)).any()
    # the device form, in place on the caller's model
    dev = torch.device("cuda:0")
    td = torch.from_numpy(D2.view(np.int16)).to(dev); tb = torch.from_numpy(bg1.view(np.int16)).to(dev)
    ctx.sensor_background_dev(td.data_ptr(), 76, 20, 3, 5, False, tb.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(tb.cpu().numpy().view(np.uint16), want2)


def test_render_filter_track_on_one_stream(weights):
    """raw 640x480 SR300-style frames (rendered, background reported as 0) -> FilterIvy -> ht_update_frames_dev on one stream, nothing synchronised in between:
    the poses equal update_frames_sync on the restatement's frames and cameras bit for bit"""
    from hand_tracking_samples_amd import native
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    n = 4
    idx = [3, 200, 470, 900]
    poses = z["gtpose"][idx].astype(np.float32); start = z["startpose"][idx].astype(np.float32)
    cams = np.tile(np.array([305 * 2, 305 * 2, 320, 240, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32), (n, 1))
    ctx = native.Context(MODEL, n)
    try:
        ctx.load_weights(weights)
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        raw = ctx.render_depth(poses, cams, 640, 480)
        far = int(raw.max())      # the 4 m background: (uint16)(4.0f / 0.001f) = 3999 counts
        assert far == R.ivy_fill(0.001) and (raw < far).any() and (raw == far).mean() > 0.5
        raw[raw == far] = 0       # as the sensor reports "no data"
        dev = torch.device("cuda:0")
        tr = torch.from_numpy(raw.view(np.int16)).to(dev); tc = torch.from_numpy(cams).to(dev); ts = torch.from_numpy(start).to(dev)
        td = torch.empty((n, 240, 320), dtype=torch.int16, device=dev); tco = torch.empty((n, 12), dtype=torch.float32, device=dev)
        out = torch.empty((n, 17, 7), dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        ctx.sensor_filter_dev(native.SENSOR_IVY, tr.data_ptr(), None, tc.data_ptr(), 640, 480, n, 320, None, td.data_ptr(), tco.data_ptr(), s.cuda_stream)
        ctx.update_frames_dev(td.data_ptr(), tco.data_ptr(), 320, 240, 0.17, ts.data_ptr(), n, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        got = out.cpu().numpy()
        ref = [R.filter_ivy(raw[b], cams[b]) for b in range(n)]
        frames = np.stack([r[0] for r in ref]); rcams = np.stack([r[1] for r in ref])
        assert np.array_equal(td.cpu().numpy().view(np.uint16), frames) and tco.cpu().numpy().tobytes() == rcams.tobytes()
        ctx.tracker_reset(start)
        want = ctx.update_frames_sync(frames, rcams, 0.17)
        assert np.array_equal(got, want)
    finally:
        ctx.close()
