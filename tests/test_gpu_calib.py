"""GPU: ht_calibrate_view (include/ht_mi355x.h "a view's extrinsics") against tests/calib_ref.py, which tests/test_calib_ref.py holds alone, bit for
bit on T_out and on every float64 of stats.  hand17 with B = 3 and B = 1, hand26 with B = 2, 37x29 frames, fraction 1 and 4, iterations 0, 1 and 6, both modes, a centre
off the origin, damping 0 and 1e-3, model 0 and 1, explicit poses against the slots' state; slots masked to exactly 0, 1, 255, 256 and 257 points (the stride's tail, an
empty wave); the device form on a side stream into guarded buffers one word into their allocations; a second identical call; everything else the context holds left as it
was; a fused update after a calibration equal to one without."""
import functools

import numpy as np
import pytest
import torch

import calib_ref as cr
import joints_inputs as ji
import kpfit_inputs as ki
import kpfit_ref as kr
import oracle_lib as ol
import views_ref as vr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = {"hand17": 6, "hand26": 3}
W, H = 37, 29
# (model, B, fraction, mode, iterations, damping, centre, which, explicit poses)
CASES = [("hand17", 3, 1, cr.RIG, 6, 1e-3, (0.0, 0.0, 0.0), 0, False),
         ("hand17", 3, 4, cr.PER_SLOT, 6, 0.0, (0.02, -0.01, 0.4), 0, True),
         ("hand17", 3, 1, cr.PER_SLOT, 1, 1e-3, (0.0, 0.0, 0.0), 1, False),
         ("hand17", 3, 4, cr.RIG, 0, 0.0, (0.0, 0.0, 0.0), 1, True),
         ("hand17", 1, 1, cr.RIG, 6, 0.0, (0.02, -0.01, 0.4), 0, False),
         ("hand17", 1, 4, cr.PER_SLOT, 1, 1e-3, (0.0, 0.0, 0.0), 0, True),
         ("hand26", 2, 1, cr.RIG, 1, 0.0, (0.0, 0.0, 0.0), 1, False),
         ("hand26", 2, 4, cr.PER_SLOT, 6, 1e-3, (0.02, -0.01, 0.4), 0, False),
         ("hand26", 2, 1, cr.PER_SLOT, 0, 1e-3, (0.0, 0.0, 0.0), 0, True)]


@pytest.fixture(scope="module")
def ctxs(weights):
    from hand_tracking_samples_amd import native
    made = {}

    def get(name):
        if name not in made:
            made[name] = native.Context(ji.model_path(name), CAP[name])
            if name == "hand17":
                made[name].load_weights(weights)
        return made[name]
    yield get
    for c in made.values():
        c.close()


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


def _same(got, want):
    T, s = got; rT, rs = want
    assert T.shape == rT.shape and s.shape == rs.shape
    assert np.array_equal(T.view(np.uint32), rT.view(np.uint32)), "T differs: %s against %s" % (T, rT)
    bad = np.argwhere(s.view(np.uint64) != rs.view(np.uint64))
    assert not len(bad), "%d of %d stats differ, the first at %s: %r against %r" % (len(bad), s.size, bad[0], s[tuple(bad[0])], rs[tuple(bad[0])])


@functools.lru_cache(None)
def scene(name, B, w=W, h=H):
    """slot i: frame 3 i's ground truth seen by one fixed second camera, half way round frame 0's palm; the guess 2 degrees and 8 mm off that camera"""
    sc = cr.rig_scene(name, tuple(3 * i for i in range(B)), w, h, 180.0)
    depth, cams = np.ascontiguousarray(sc["depth"][:, 1]), np.ascontiguousarray(sc["cams"][:, 1])
    return depth, np.stack([cr.perturbed(c, 2.0, 0.008) for c in cams]), np.ascontiguousarray(sc["truth"], np.float32)


def _options(ctx, fraction, mode, iterations, damping, centre, **kw):
    o = ctx.calib_default(fraction=fraction, mode=mode, iterations=iterations, damping=damping, centre=centre, **kw)
    return o, cr.options(range_hi=float(o.range_hi), fraction=fraction, mode=mode, iterations=iterations, damping=damping, centre=centre, **kw)


def _fill(ctx, name, which, truth):
    """model `which` of slots [0,B) at the truth, the other model and the slots behind at another frame's with momenta: nothing of these may be read or written"""
    full = CAP[name]; P = ki.truths(name)
    rest = ki.states_of(P[40:40 + full]); rest[:, :, 7:13] = 0.25
    ctx.set_state(1 - which, rest)
    mine = rest.copy(); mine[:len(truth)] = ki.states_of(truth)
    ctx.set_state(which, mine)
    return {which: mine, 1 - which: rest}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(i) for i in c[:5]) + "-w%d%s" % (c[7], "-poses" if c[8] else ""))
def test_calibration_equals_the_restatement(ctxs, oracles, case):
    name, B, fraction, mode, iterations, damping, centre, which, explicit = case
    ctx, orc = ctxs(name), oracles(name)
    depth, guess, truth = scene(name, B)
    o, ro = _options(ctx, fraction, mode, iterations, damping, centre)
    want = cr.calibrate(orc, depth, guess, truth, ro)
    states = _fill(ctx, name, which, truth)
    flags = ctx.tracker_flags(CAP[name])
    got = ctx.calibrate_view(depth, guess, truth if explicit else None, which, o)
    _same(got, want)
    assert (want[1][:, :, 0] > 12).all() and not want[1][:, :, 5].any() and (iterations == 0 or not np.array_equal(want[0][0].view(np.uint32), guess[0, 5:12].view(np.uint32)))
    other = ctx.calibrate_view(depth, guess, None if explicit else truth, which, o)      # the other source of the same poses: the same bits
    _same(other, want)
    _same(ctx.calibrate_view(depth, guess, truth if explicit else None, which, o), want)      # a second identical call
    for k in (0, 1):
        assert np.array_equal(ctx.get_state(k, CAP[name]).view(np.uint32), states[k].view(np.uint32))
    f2 = ctx.tracker_flags(CAP[name])
    assert np.array_equal(flags[0].view(np.uint32), f2[0].view(np.uint32)) and np.array_equal(flags[1], f2[1])


@pytest.mark.parametrize("mode", [cr.PER_SLOT, cr.RIG])
def test_slots_of_exactly_0_1_255_256_257_points(ctxs, oracles, mode):
    """the stride's tail (255, 256, 257 points over 256 threads), one point, and a slot -- every wave of its block -- without any"""
    name, counts = "hand17", (0, 1, 255, 256, 257)
    ctx, orc = ctxs(name), oracles(name)
    depth, guess, truth = scene(name, 1, 80, 60)
    o, ro = _options(ctx, 1, mode, 2, 1e-3, (0.0, 0.0, 0.0), min_points=0)
    d = depth[0].astype(np.float32) * guess[0, 4]
    kept = np.flatnonzero(((d >= np.float32(0.1)) & (d < np.float32(o.range_hi))).reshape(-1))
    assert len(kept) > 257
    frames = []
    for k in counts:
        f = np.zeros(depth[0].size, np.uint16); f[kept[:k]] = depth[0].reshape(-1)[kept[:k]]
        frames.append(f.reshape(depth[0].shape))
    frames = np.stack(frames); B = len(counts)
    g = np.tile(guess, (B, 1)); P = np.tile(truth, (B, 1, 1))
    want = cr.calibrate(orc, frames, g, P, ro)
    assert want[1][0, :, 1].tolist() == (list(counts) if mode == cr.PER_SLOT else [sum(counts)])
    if mode == cr.PER_SLOT:
        assert want[1][0, 0, 5] == cr.BAD_PIVOT and not want[1][:, 2:, 5].any()      # no point: a zero pivot, no step, T keeps its bits (one point: Marquardt's scaling keeps the pivots positive)
        assert np.array_equal(want[0][0].view(np.uint32), g[0, 5:12].view(np.uint32)) and np.isfinite(want[1]).all() and np.isfinite(want[0]).all()
    _same(ctx.calibrate_view(frames, g, P, 0, o), want)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def test_device_form_on_a_side_stream_into_guarded_buffers(ctxs, oracles):
    name, B = "hand17", 3
    ctx, orc = ctxs(name), oracles(name)
    depth, guess, truth = scene(name, B)
    for mode, explicit in ((cr.RIG, True), (cr.PER_SLOT, False)):
        o, ro = _options(ctx, 1, mode, 6, 1e-3, (0.0, 0.0, 0.0))
        want = cr.calibrate(orc, depth, guess, truth, ro)
        _fill(ctx, name, 0, truth)
        N = want[0].shape[0]; nT, ns = N * 7, want[1].size
        G = 7.0
        d_T = torch.full((nT + 9,), G, dtype=torch.float32, device=DEV); d_s = torch.full((2 * ns + 9,), G, dtype=torch.float32, device=DEV)
        d_depth, d_cams, d_poses = _dev(depth), _dev(guess), _dev(truth)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            ctx.calibrate_view_dev(d_depth.data_ptr(), d_cams.data_ptr(), W, H, B, d_T.data_ptr() + 4, d_s.data_ptr() + 4, d_poses=d_poses.data_ptr() if explicit else None, which=0, options=o,
                                   stream=stream.cuda_stream)
        stream.synchronize()
        T, s = d_T.cpu().numpy(), d_s.cpu().numpy()
        assert T[0] == G and (T[1 + nT:] == G).all() and s[0] == G and (s[1 + 2 * ns:] == G).all()      # the guards
        _same((T[1:1 + nT].reshape(N, 7), s[1:1 + 2 * ns].copy().view(np.float64).reshape(want[1].shape)), want)


def test_prepared_points_stay_and_a_fused_update_is_unchanged(ctxs):
    """the calibration keeps its cloud in a buffer of its own: the slots' fused cloud reads the same rows afterwards, and ht_update_views_sync gives the same poses, states
    and flags whether a calibration ran before it or not"""
    name, B, w, h = "hand17", 3, 80, 60
    ctx = ctxs(name); m = ji.model(name)
    sc = vr.two_view_scene(name, (0, 3, 6), w, h, 180.0)
    depth, cams, truth = sc["depth"], sc["cams"], np.ascontiguousarray(sc["truth"], np.float32)
    guess = np.stack([cr.perturbed(c, 2.0, 0.008) for c in cams[:, 1]])
    opt = ctx.views_default(fraction=2)
    ctx.fuse_views(depth, cams, None, opt)
    ctx.set_state(0, ki.states_of(truth))
    rows, n = ctx.stage_view_rows(0, B)
    T, s = ctx.calibrate_view(np.ascontiguousarray(depth[:, 1]), guess, None, 0, ctx.calib_default(fraction=1))
    assert not s[:, :, 5].any() and s[-1, 0, 2] < s[0, 0, 2]
    rows2, n2 = ctx.stage_view_rows(0, B)
    assert np.array_equal(n, n2) and np.array_equal(rows.view(np.uint32), rows2.view(np.uint32)) and (n > 100).all()
    start = kr.user_poses(m, ki.states_of(np.stack([ki.truths(name)[3 * i + 1] for i in range(B)])))

    def update(calibrate):
        ctx.tracker_reset(start)
        if calibrate:
            ctx.calibrate_view(np.ascontiguousarray(depth[:, 1]), guess, None, 0, ctx.calib_default(fraction=1, mode=cr.PER_SLOT))
        poses = ctx.update_views_sync(depth, cams, None, side=64, options=opt, passes=2)
        return [poses, ctx.get_state(0, CAP[name]), ctx.get_state(1, CAP[name])] + list(ctx.tracker_flags(CAP[name]))
    for a, b in zip(update(False), update(True)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refused_calls_leave_the_context_usable(ctxs, oracles):
    from hand_tracking_samples_amd import native
    name, B = "hand17", 3
    ctx, orc = ctxs(name), oracles(name)
    depth, guess, truth = scene(name, B)
    D = ctx.calib_default
    big = np.zeros((CAP[name] + 1, H, W), np.uint16); bigc = np.tile(guess[:1], (CAP[name] + 1, 1))
    for call, text in ((lambda: ctx.calibrate_view(depth, guess, None, 0, D(fraction=0)), "fraction"), (lambda: ctx.calibrate_view(depth, guess, None, 0, D(mode=2)), "mode"),
                       (lambda: ctx.calibrate_view(depth, guess, None, 0, D(iterations=65)), "iterations"), (lambda: ctx.calibrate_view(depth, guess, None, 2, None), "which is 0"),
                       (lambda: ctx.calibrate_view(big, bigc, None, 0, None), "batch"), (lambda: ctx.calibrate_view(np.zeros((1, 480, 640), np.uint16), guess[:1], None, 0, D(fraction=1)), "307200 points"),
                       (lambda: ctx.calibrate_view_dev(16, 16, W, H, B, 18, 16, options=D()), "4-byte aligned")):
        with pytest.raises(native.HTError, match=text):
            call()
    c2 = native.Context(None, 2)
    try:
        with pytest.raises(native.HTError, match="without a hand model"):
            c2.calibrate_view(depth[:2], guess[:2], None, 0, None)
    finally:
        c2.close()
    # explicit poses are not bounded by the context's slots: more frames than max_batch, and the same call as before still gives the same result
    P = ki.truths(name); n = CAP[name] + 2
    o, ro = _options(ctx, 2, cr.RIG, 2, 1e-3, (0.0, 0.0, 0.0))
    many = np.tile(depth[:1], (n, 1, 1)); mg = np.tile(guess[:1], (n, 1)); mp = np.tile(truth[:1], (n, 1, 1))
    _same(ctx.calibrate_view(many, mg, mp, 0, o), cr.calibrate(orc, many, mg, mp, ro))
    _same(ctx.calibrate_view(depth, guess, truth, 0, o), cr.calibrate(orc, depth, guess, truth, ro))


def test_cxx_form_equals_the_c_call(ctxs, tmp_path):
    """tests/cxx_calib_driver.cpp: HandTracker::CalibrateView on a tracker of one slot against ht_calibrate_view on a context of its own, and both against the binding"""
    import os
    import subprocess
    from hand_tracking_samples_amd import native
    name, B = "hand17", 3
    ctx = ctxs(name)
    depth, guess, truth = scene(name, B)
    exe = str(tmp_path / "calib"); libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ji.ROOT, "tests", "cxx_calib_driver.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    files = {k: str(tmp_path / k) for k in ("frames.u16", "cams.f32", "poses.f32")}
    depth.tofile(files["frames.u16"]); guess.tofile(files["cams.f32"]); truth.tofile(files["poses.f32"])
    r = subprocess.run([exe, ji.model_path(name), str(W), str(H), files["frames.u16"], files["cams.f32"], files["poses.f32"], "4", "2"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    assert lines[0] == "frames=3 records=5 degenerate=0 equal=1"
    T, s = ctx.calibrate_view(depth, guess, truth, 0, ctx.calib_default(iterations=4, fraction=2))
    got = np.array([float.fromhex(x) for x in lines[1].split()[1:]], np.float32)
    assert np.array_equal(got.view(np.uint32), T[0].view(np.uint32))
    assert [float.fromhex(x) for x in lines[2].split()[1:]] == [s[0, 0, 2], s[-1, 0, 2]]
