"""GPU: ht_sensor_simulate* (csrc/ht_sensor.hip) equals the restatement of its definition (tests/sensor_sim_ref.py, which tests/test_sensor_sim_ref.py pins) bit for
bit: every size at which the kernel takes another path, both kinds, with and without the IR image, the wall and the disparity step, on frames that take every branch
(the counts are asserted, so an all-background input cannot pass); views that reach each narrower load width, guard bytes, host against device form, second calls,
stream independence, the ends of the probability range, refusals, and rendered hands made raw, filtered and tracked on one stream.

The width a call takes follows the one width rule (ht_frame_vec_pixels, csrc/ht_frame_vec.hpp): 8 pixels a thread (16 bytes) for w % 8 == 0 and 16-byte aligned frames with an 8-byte aligned IR image, then 4, 2
and 1.  Of the sizes below 40x12, 320x240 and 640x480 take 16 bytes; 36x20 and 76x20 (divisible by 4, not by 8) take 8; 17x9, 3x3 and 1x1 single pixels; 4x4 eight bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import sensor_ref as R
import sensor_sim_frames as F
import sensor_sim_ref as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL = os.path.join(HERE, "golden", "model_hand17.htfx")
DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from hand_tracking_samples_amd import native
    c = native.Context(MODEL, 4)
    yield c
    c.close()


def _nat(nz):
    from hand_tracking_samples_amd import native
    return native.SensorNoise(**{k: getattr(nz, k) for k in S.FIELDS})


def _ref(n):
    return S.Noise(**{k: getattr(n, k) for k in S.FIELDS})


CONFIGS = (("ivy", S.IVY, F.NOISE_IVY, F.FAR, ("edge_drop", "fly", "slope_drop", "hole")),
           ("ivy, zero background", S.IVY, F.NOISE_IVY.but(seed=99), 0, ("edge_drop", "fly", "slope_drop", "hole")),
           ("ds4, coarse disparity", S.DS4, F.NOISE_DS4, F.FAR, ("edge_drop", "fly", "slope_drop", "hole", "disp_drop")),
           ("ds4, the default's disparity", S.DS4, F.NOISE_DS4_FINE, 0, ("edge_drop", "fly", "slope_drop", "hole")),
           ("ds4, wall", S.DS4, F.NOISE_DS4_WALL, F.FAR, ("edge_drop", "fly", "slope_drop", "hole")))


@pytest.mark.parametrize("w,h,B", [(1, 1, 64), (3, 3, 64), (4, 4, 64), (17, 9, 3), (36, 20, 3), (40, 12, 3), (76, 20, 3), (320, 240, 3), (640, 480, 2), (36, 20, 70)])
def test_host_form_equals_the_restatement(ctx, w, h, B):
    """borders everywhere (1x1, 3x3, 4x4), an odd width, the 8- and 16-byte paths, more blocks than one, more frames than a launch's first round of blocks"""
    for name, kind, nz, background, branches in CONFIGS:
        frames = F.blobs(w, h, B, seed=kind, background=background)
        if w >= 3 and h >= 3:
            c = F.counts(kind, frames, nz)
            assert all(c[k] > 0 for k in branches + ("foreground", "background")), (name, c)
        want_d, want_i = S.simulate(kind, frames, nz)
        got_d, got_i = ctx.sensor_simulate(kind, frames, _nat(nz), want_ir=True)
        assert np.array_equal(got_d, want_d), name
        assert np.array_equal(got_i, want_i), name
        if kind == S.IVY:
            alone, none = ctx.sensor_simulate(kind, frames, _nat(nz), want_ir=False)
            assert none is None and np.array_equal(alone, want_d), name


def test_more_frames_than_blocks_along_y(ctx):
    """320x240 frames are 38 blocks each, so a launch has 54 blocks along y: with 60 frames the threads of the first six walk two frames each"""
    four = F.blobs(320, 240, 4)
    frames = np.ascontiguousarray(four[np.arange(60) % 4])
    want_d, want_i = S.simulate(S.IVY, frames, F.NOISE_IVY)
    got_d, got_i = ctx.sensor_simulate(S.IVY, frames, _nat(F.NOISE_IVY), want_ir=True)
    assert np.array_equal(got_d, want_d) and np.array_equal(got_i, want_i)
    assert not np.array_equal(got_d[0], got_d[4])      # the same input, another stream


def _buffers(n, in_off, out_off, ir_off, frames):
    """device buffers with GUARD elements before and after, the views `off` elements further in"""
    tin = torch.zeros(n + 2 * GUARD, dtype=torch.int16, device=DEV)
    tin[GUARD + in_off:GUARD + in_off + n] = torch.from_numpy(frames.reshape(-1).view(np.int16)).to(DEV)
    tout = torch.full((n + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device=DEV)
    tir = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert tin.data_ptr() % 256 == 0 and tout.data_ptr() % 256 == 0 and tir.data_ptr() % 256 == 0 and GUARD * 2 % 16 == 0
    return tin, tout, tir, tin.data_ptr() + 2 * (GUARD + in_off), tout.data_ptr() + 2 * (GUARD + out_off), tir.data_ptr() + GUARD + ir_off


@pytest.mark.parametrize("in_off,out_off,ir_off", [(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
@pytest.mark.parametrize("kind", [S.IVY, S.DS4])
def test_device_form_on_views_with_guard_bytes(ctx, kind, in_off, out_off, ir_off):
    """40x12 frames: aligned buffers take 16 bytes a thread; a view 4, 2 or 1 elements in -- the input, the output or the IR image -- takes 8, 4, or single pixels.
    Nothing is written outside the outputs, and the result is the restatement's and the host form's."""
    w, h, B = 40, 12, 3
    n = w * h * B
    nz = F.NOISE_IVY if kind == S.IVY else F.NOISE_DS4_FINE
    frames = F.blobs(w, h, B, seed=3)
    want_d, want_i = S.simulate(kind, frames, nz)
    tin, tout, tir, pin, pout, pir = _buffers(n, in_off, out_off, ir_off, frames)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    ctx.sensor_simulate_dev(kind, pin, w, h, B, _nat(nz), pout, pir, s.cuda_stream)
    s.synchronize()
    out = tout.cpu().numpy().view(np.uint16); ir = tir.cpu().numpy()
    a, b = GUARD + out_off, GUARD + ir_off
    assert (out[:a] == 0x5A5A).all() and (out[a + n:] == 0x5A5A).all() and (ir[:b] == 0xA5).all() and (ir[b + n:] == 0xA5).all()
    assert np.array_equal(out[a:a + n].reshape(B, h, w), want_d) and np.array_equal(ir[b:b + n].reshape(B, h, w), want_i)
    host_d, host_i = ctx.sensor_simulate(kind, frames, _nat(nz), want_ir=True)
    assert host_d.tobytes() == want_d.tobytes() and host_i.tobytes() == want_i.tobytes()
    if kind == S.IVY:      # without ir_out nothing is written beyond depth_out
        tout.fill_(0x5A5A); tir.fill_(0xA5)
        ctx.sensor_simulate_dev(kind, pin, w, h, B, _nat(nz), pout, None, s.cuda_stream)
        s.synchronize()
        out = tout.cpu().numpy().view(np.uint16)
        assert (tir.cpu().numpy() == 0xA5).all() and (out[:a] == 0x5A5A).all() and (out[a + n:] == 0x5A5A).all() and np.array_equal(out[a:a + n].reshape(B, h, w), want_d)


def test_a_second_call_after_a_smaller_and_a_larger_one(ctx):
    from hand_tracking_samples_amd import native
    c = native.Context(MODEL, 1)      # its staging starts empty
    try:
        for w, h, B in ((36, 20, 3), (320, 240, 3), (17, 9, 3), (320, 240, 3), (36, 20, 5)):
            frames = F.blobs(w, h, B, seed=w)
            want = S.simulate(S.DS4, frames, F.NOISE_DS4_WALL)
            got = c.sensor_simulate(S.DS4, frames, _nat(F.NOISE_DS4_WALL))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (w, h, B)
    finally:
        c.close()


def test_a_frames_stream_is_first_index_plus_f(ctx):
    frames = F.blobs(36, 20, 12)
    for first in (10, (1 << 64) - 7):      # the second wraps inside the call
        nz = F.NOISE_DS4.but(first_index=first)
        d12, i12 = ctx.sensor_simulate(S.DS4, frames, _nat(nz))
        d5, i5 = ctx.sensor_simulate(S.DS4, frames[5:10], _nat(nz.but(first_index=(first + 5) & S.M64)))
        assert np.array_equal(d12[5:10], d5) and np.array_equal(i12[5:10], i5)
        want = S.simulate(S.DS4, frames, nz)
        assert np.array_equal(d12, want[0]) and np.array_equal(i12, want[1])
    other = ctx.sensor_simulate(S.DS4, frames, _nat(F.NOISE_DS4.but(seed=1)))[0]
    assert not np.array_equal(other, d12)


@pytest.mark.parametrize("change", [dict(), dict(p_edge_drop=65536), dict(p_edge_fly=65536), dict(p_slope_drop=65536), dict(p_hole=65536), dict(p_edge_drop=1, p_edge_fly=65535)])
def test_probabilities_at_the_ends_of_their_range(ctx, change):
    frames = F.blobs(76, 20, 3)
    off = dict(p_edge_drop=0, p_edge_fly=0, p_slope_drop=0, p_hole=0)
    for kind, base in ((S.IVY, F.NOISE_IVY), (S.DS4, F.NOISE_DS4_FINE)):
        nz = base.but(**dict(off, **change))
        want = S.simulate(kind, frames, nz)
        got = ctx.sensor_simulate(kind, frames, _nat(nz), want_ir=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        fg = frames < F.FAR
        if not change:
            assert (got[0][fg] != 0).all()
        if change == dict(p_hole=65536):
            assert (got[0] == 0).all() and (got[1] < 8).all()


def test_everything_off_keeps_the_foreground(ctx):
    frames = F.blobs(76, 20, 3)
    off = F.NOISE_IVY.but(sigma0_256=0, sigma2=0, p_edge_drop=0, p_edge_fly=0, p_slope_drop=0, p_hole=0)
    fg = frames < F.FAR
    d, _ = ctx.sensor_simulate(S.IVY, frames, _nat(off))
    assert np.array_equal(d[fg], frames[fg]) and (d[~fg] == 0).all()
    d, _ = ctx.sensor_simulate(S.DS4, frames, _nat(off.but(wall_count=1234)))
    assert np.array_equal(d[fg], frames[fg]) and (d[~fg] == 1234).all()


def _tracked(weights, before=None):
    """a fresh context, optionally some calls first, then one update of four golden frames -> what the update and the state are, as bytes"""
    import htfx
    from hand_tracking_samples_amd import native
    g = htfx.load(os.path.join(HERE, "golden", "golden8.htfx"))
    depth = np.stack([g["f%d/depth" % f].reshape(-1) for f in range(4)]); cams = np.stack([g["f%d/cam" % f] for f in range(4)])
    c = native.Context(MODEL, 4)
    try:
        c.load_weights(weights); c.set_params(microforce=3.0, mainthreadpasses=3)
        if before:
            before(c)
        c.tracker_reset(np.stack([g["f%d/startpose" % f] for f in range(4)]))
        poses = c.update_sync(depth, cams)
        return [np.ascontiguousarray(poses).tobytes(), c.get_state(0, 4).tobytes(), c.get_state(1, 4).tobytes()]
    finally:
        c.close()


def test_refusals_leave_the_context_usable_and_the_update_untouched(weights):
    from hand_tracking_samples_amd import native

    def before(c):
        L, h = c.L, c.h
        d = np.full((2, 4, 4), 500, np.uint16); out = np.full((2, 4, 4), 7, np.uint16); ir = np.full((2, 4, 4), 7, np.uint8)
        u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)); u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        base = native.sensor_noise_default(0)
        for kw in F.refusals(u16(d)):
            a = dict(dict(kind=0, depth=u16(d), w=4, h=4, B=2, noise=True, out=u16(out), ir=u8(ir)), **{k: v for k, v in kw.items() if k != "nz"})
            nz = None if a["noise"] is None else C.byref(base.but(**kw.get("nz", {})))
            assert L.ht_sensor_simulate(h, a["kind"], a["depth"], a["w"], a["h"], a["B"], nz, a["out"], a["ir"]) == 1, kw
            assert "ht_sensor_simulate: bad argument" in L.ht_last_error(h).decode(), kw
        assert (out == 7).all() and (ir == 7).all()
        # the device form refuses the same before anything is launched (made-up addresses: nothing may touch them)
        assert L.ht_sensor_simulate_dev(h, 0, 4096, 4, 4, 2, C.byref(base), 4096 + 32, None, None) == 1      # overlapping
        assert L.ht_sensor_simulate_dev(h, 1, 4096, 4, 4, 2, C.byref(base), 8192, None, None) == 1           # DS4 without ir_out
        assert L.ht_sensor_simulate_dev(h, 0, 4096, 4, 4, 2, C.byref(base.but(p_hole=65537)), 8192, None, None) == 1
        assert L.ht_sensor_simulate(h, 0, u16(d), 4, 4, 0, C.byref(base), u16(out), u8(ir)) == 0 and (out == 7).all() and (ir == 7).all()      # B = 0 does nothing
        with pytest.raises(native.HTError, match="far_count"):
            c.sensor_simulate(0, d, base.but(far_count=0))
        frames = F.blobs(36, 20, 3)
        got = c.sensor_simulate(S.DS4, frames, _nat(F.NOISE_DS4))      # the context works afterwards
        want = S.simulate(S.DS4, frames, F.NOISE_DS4)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert _tracked(weights, before) == _tracked(weights)


def _bench_hands(idx):
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    return z["gtpose"][idx].astype(np.float32), z["startpose"][idx].astype(np.float32)


def test_render_simulate_filter_track_on_one_stream_ivy(weights):
    """rendered 640x480 hands -> SR300-style raw frames -> FilterIvy -> ht_update_frames_sized_dev on one stream, nothing synchronised in between: the poses equal
    ht_update_frames_sized_sync on the restatement's simulated-then-filtered frames bit for bit"""
    from hand_tracking_samples_amd import native
    n, w, h = 4, 640, 480
    poses, start = _bench_hands([3, 200, 470, 900])
    cams = np.tile(np.array([610, 610, 320, 240, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32), (n, 1))
    noise = native.sensor_noise_default(native.SENSOR_IVY, 0.001, 4.0, seed=2024, first_index=7)
    c = native.Context(MODEL, n)
    try:
        c.load_weights(weights); c.set_params(microforce=3.0, mainthreadpasses=3)
        clean = c.render_depth(poses, cams, w, h)
        counts = F.counts(S.IVY, clean, _ref(noise))
        assert all(counts[k] > 0 for k in ("edge_drop", "fly", "slope_drop", "hole", "foreground", "background")), counts
        dev = torch.device(DEV)
        tclean = torch.from_numpy(clean.view(np.int16)).to(dev); tc = torch.from_numpy(cams).to(dev); ts = torch.from_numpy(start).to(dev)
        traw = torch.empty((n, h, w), dtype=torch.int16, device=dev); tf = torch.empty((n, h, w), dtype=torch.int16, device=dev); tco = torch.empty((n, 12), dtype=torch.float32, device=dev)
        out = torch.empty((n, 17, 7), dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        c.sensor_simulate_dev(native.SENSOR_IVY, tclean.data_ptr(), w, h, n, noise, traw.data_ptr(), None, s.cuda_stream)
        c.sensor_filter_dev(native.SENSOR_IVY, traw.data_ptr(), None, tc.data_ptr(), w, h, n, w, None, tf.data_ptr(), tco.data_ptr(), s.cuda_stream)
        c.update_frames_sized_dev(64, tf.data_ptr(), tco.data_ptr(), w, h, 0.17, ts.data_ptr(), n, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        raw = S.simulate(S.IVY, clean, _ref(noise))[0]
        assert np.array_equal(traw.cpu().numpy().view(np.uint16), raw)
        ref = [R.filter_ivy(raw[b], cams[b], w) for b in range(n)]
        frames = np.stack([r[0] for r in ref]); rcams = np.stack([r[1] for r in ref])
        assert np.array_equal(tf.cpu().numpy().view(np.uint16), frames) and tco.cpu().numpy().tobytes() == rcams.tobytes()
        c.tracker_reset(start)
        want = c.update_frames_sized_sync(frames, rcams, 64, 0.17)
        assert np.array_equal(out.cpu().numpy(), want)
    finally:
        c.close()


def test_render_simulate_filter_track_on_one_stream_ds4(weights):
    """the same at 320x240 for an R200: simulate with the IR image -> FilterDS4 -> ht_update_frames_dev"""
    from hand_tracking_samples_amd import native
    n, w, h = 4, 320, 240
    poses, start = _bench_hands([3, 200, 470, 900])
    cams = np.tile(np.array([305, 305, 160, 120, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32), (n, 1))
    noise = native.sensor_noise_default(native.SENSOR_DS4, 0.001, 4.0, seed=2025, first_index=1 << 40)
    c = native.Context(MODEL, n)
    try:
        c.load_weights(weights); c.set_params(microforce=3.0, mainthreadpasses=3)
        clean = c.render_depth(poses, cams, w, h)
        counts = F.counts(S.DS4, clean, _ref(noise))
        assert all(counts[k] > 0 for k in ("edge_drop", "fly", "slope_drop", "hole", "foreground", "background")), counts
        dev = torch.device(DEV)
        tclean = torch.from_numpy(clean.view(np.int16)).to(dev); tc = torch.from_numpy(cams).to(dev); ts = torch.from_numpy(start).to(dev)
        traw = torch.empty((n, h, w), dtype=torch.int16, device=dev); tir = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        tf = torch.empty((n, h, w), dtype=torch.int16, device=dev); tco = torch.empty((n, 12), dtype=torch.float32, device=dev)
        out = torch.empty((n, 17, 7), dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        c.sensor_simulate_dev(native.SENSOR_DS4, tclean.data_ptr(), w, h, n, noise, traw.data_ptr(), tir.data_ptr(), s.cuda_stream)
        c.sensor_filter_dev(native.SENSOR_DS4, traw.data_ptr(), tir.data_ptr(), tc.data_ptr(), w, h, n, 320, None, tf.data_ptr(), tco.data_ptr(), s.cuda_stream)
        c.update_frames_dev(tf.data_ptr(), tco.data_ptr(), w, h, 0.17, ts.data_ptr(), n, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        raw, ir = S.simulate(S.DS4, clean, _ref(noise))
        assert np.array_equal(traw.cpu().numpy().view(np.uint16), raw) and np.array_equal(tir.cpu().numpy(), ir)
        frames = np.stack([R.filter_ds4(raw[b], ir[b], None, max_width=320) for b in range(n)])
        assert np.array_equal(tf.cpu().numpy().view(np.uint16), frames) and tco.cpu().numpy().tobytes() == cams.tobytes()
        assert ((frames == 4096) | (ir >= 8)).all() and (ir < 8).any()
        c.tracker_reset(start)
        want = c.update_frames_sync(frames, cams, 0.17)
        assert np.array_equal(out.cpu().numpy(), want)
    finally:
        c.close()


def test_cxx_sensor_sim_example_runs_on_the_device(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "sensor_sim")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_sensor_sim_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, MODEL], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
