"""GPU: ht_estimate_scale (include/ht_mi355x.h "the hand's size") against tests/size_ref.py, which tests/test_size_ref.py holds alone, bit for bit on
scale_out, T_out and every float64 of stats.  hand17 with B = 3 and B = 1, hand26 with B = 2, 37x29 frames of a hand 1.1 times the model's size, fraction 1 and 4,
iterations 0, 1 and 6, both modes with both values of free_pose, scale0 of 0.9, 1 and 1.2, damping 0 and 1e-3, model 0 and 1, explicit poses against the slots' state;
slots masked to exactly 0, 1, 255, 256 and 257 points; a SHARED batch with one degenerate slot (the Schur path's exclusion); the device form on a side stream into guarded
buffers one word into their allocations; a second identical call; everything else the context holds left as it was; ht_calibrate_view and a fused update equal with and
without an estimate before them; every refusal."""
import functools

import numpy as np
import pytest
import torch

import calib_ref as cr
import joints_inputs as ji
import kpfit_inputs as ki
import kpfit_ref as kr
import oracle_lib as ol
import size_ref as sr
import views_ref as vr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = {"hand17": 6, "hand26": 3}
W, H = 37, 29
S_TRUE = 1.1
# (model, B, fraction, mode, free_pose, iterations, scale0, damping, which, explicit poses)
CASES = [("hand17", 3, 1, sr.SHARED, 1, 6, 1.0, 1e-3, 0, False),
         ("hand17", 3, 4, sr.SHARED, 0, 6, 0.9, 0.0, 0, True),
         ("hand17", 3, 1, sr.PER_SLOT, 1, 6, 1.2, 0.0, 1, False),
         ("hand17", 3, 4, sr.PER_SLOT, 0, 1, 1.0, 1e-3, 1, True),
         ("hand17", 3, 1, sr.SHARED, 1, 0, 1.2, 1e-3, 0, True),
         ("hand17", 1, 1, sr.SHARED, 1, 6, 0.9, 0.0, 0, False),
         ("hand17", 1, 4, sr.PER_SLOT, 1, 1, 1.0, 1e-3, 0, True),
         ("hand17", 1, 1, sr.SHARED, 0, 1, 1.2, 1e-3, 1, False),
         ("hand26", 2, 1, sr.SHARED, 1, 1, 1.0, 0.0, 1, False),
         ("hand26", 2, 4, sr.PER_SLOT, 1, 6, 0.9, 1e-3, 0, False),
         ("hand26", 2, 1, sr.PER_SLOT, 0, 0, 1.0, 1e-3, 0, True),
         ("hand26", 2, 4, sr.SHARED, 0, 6, 1.2, 0.0, 0, True)]


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
    assert len(got) == 3
    for g, r in zip(got[:2], want[:2]):
        assert g.shape == r.shape and np.array_equal(g.view(np.uint32), r.view(np.uint32)), "%s against %s" % (g, r)
    s, rs = got[2], want[2]
    assert s.shape == rs.shape
    bad = np.argwhere(s.view(np.uint64) != rs.view(np.uint64))
    assert not len(bad), "%d of %d stats differ, the first at %s: %r against %r" % (len(bad), s.size, bad[0], s[tuple(bad[0])], rs[tuple(bad[0])])


@functools.lru_cache(None)
def scene(name, B, w=W, h=H):
    """slot i: frame 3 i's ground truth, the hand S_TRUE times the model's size (model scaled, poses stretched about the wrist), seen by the frame camera; the poses given
    to the estimator are the unstretched ones"""
    from hand_tracking_samples_amd import native
    P = ki.truths(name); truth = np.ascontiguousarray(np.stack([P[(3 * i) % len(P)] for i in range(B)]), np.float32)
    cam = vr.frame_camera(w, h)
    m = native.HostModel(ji.model_path(name))
    try:
        m.scale(S_TRUE)
        depth = np.stack([m.raster_mesh(p, cam, w, h, 4.0, 0.5)[0] for p in sr.stretched(truth, S_TRUE)])
    finally:
        m.close()
    return depth, np.tile(cam, (B, 1)), truth


def _options(ctx, **kw):
    o = ctx.size_default(**kw)
    return o, sr.options(range_hi=float(o.range_hi), **kw)


def _fill(ctx, name, which, truth):
    """model `which` of slots [0,B) at the truth, the other model and the slots behind at another frame's with momenta: nothing of these may be read or written"""
    full = CAP[name]; P = ki.truths(name)
    rest = ki.states_of(P[40:40 + full]); rest[:, :, 7:13] = 0.25
    ctx.set_state(1 - which, rest)
    mine = rest.copy(); mine[:len(truth)] = ki.states_of(truth)
    ctx.set_state(which, mine)
    return {which: mine, 1 - which: rest}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(i) for i in c[:7]) + "-w%d%s" % (c[8], "-poses" if c[9] else ""))
def test_estimate_equals_the_restatement(ctxs, oracles, case):
    name, B, fraction, mode, free_pose, iterations, scale0, damping, which, explicit = case
    ctx, orc = ctxs(name), oracles(name)
    depth, cams, truth = scene(name, B)
    o, ro = _options(ctx, fraction=fraction, mode=mode, free_pose=free_pose, iterations=iterations, scale0=scale0, damping=damping)
    want = sr.estimate(orc, depth, cams, truth, ro)
    states = _fill(ctx, name, which, truth)
    flags = ctx.tracker_flags(CAP[name])
    got = ctx.estimate_scale(depth, cams, truth if explicit else None, which, o)
    _same(got, want)
    N = B if mode == sr.PER_SLOT else 1
    rec = want[2][:, :N * sr.STATS].reshape(iterations + 1, N, sr.STATS)
    assert (rec[:, :, 0] > 12).all() and not rec[:, :, 5].any() and (iterations == 0 or (want[0] != np.float32(scale0)).all())      # the case is not a degenerate one
    assert free_pose == 0 or iterations == 0 or not np.array_equal(want[1].view(np.uint32), cams[:, 5:12].view(np.uint32))
    _same(ctx.estimate_scale(depth, cams, None if explicit else truth, which, o), want)      # the other source of the same poses: the same bits
    _same(ctx.estimate_scale(depth, cams, truth if explicit else None, which, o), want)      # a second identical call
    for k in (0, 1):
        assert np.array_equal(ctx.get_state(k, CAP[name]).view(np.uint32), states[k].view(np.uint32))
    f2 = ctx.tracker_flags(CAP[name])
    assert np.array_equal(flags[0].view(np.uint32), f2[0].view(np.uint32)) and np.array_equal(flags[1], f2[1])


def _masked(name, counts):
    depth, cams, truth = scene(name, 1, 80, 60)
    d = depth[0].astype(np.float32) * cams[0, 4]
    kept = np.flatnonzero(((d >= np.float32(0.1)) & (d < np.float32(0.7))).reshape(-1))
    assert len(kept) > max(counts)
    frames = []
    for k in counts:
        f = np.zeros(depth[0].size, np.uint16); f[kept[:k]] = depth[0].reshape(-1)[kept[:k]]
        frames.append(f.reshape(depth[0].shape))
    B = len(counts)
    return np.stack(frames), np.tile(cams, (B, 1)), np.tile(truth, (B, 1, 1))


@pytest.mark.parametrize("mode,free_pose", [(sr.PER_SLOT, 1), (sr.PER_SLOT, 0), (sr.SHARED, 1), (sr.SHARED, 0)])
def test_slots_of_exactly_0_1_255_256_257_points(ctxs, oracles, mode, free_pose):
    """the stride's tail (255, 256, 257 points over 256 threads), one point, and a slot -- every wave of its block -- without any; min_points 0, so the empty slot's and
    the one-point slot's pivots decide"""
    name, counts = "hand17", (0, 1, 255, 256, 257)
    ctx, orc = ctxs(name), oracles(name)
    frames, g, P = _masked(name, counts)
    o, ro = _options(ctx, fraction=1, mode=mode, free_pose=free_pose, iterations=2, min_points=0)
    want = sr.estimate(orc, frames, g, P, ro)
    N = len(counts) if mode == sr.PER_SLOT else 1
    assert want[2][0, :N * sr.STATS].reshape(N, sr.STATS)[:, 1].tolist() == (list(counts) if mode == sr.PER_SLOT else [sum(counts)])
    slot = want[2][:, N * sr.STATS:].reshape(3, len(counts), sr.SLOT_STATS)
    assert slot[0, 0, 2] == sr.BAD_PIVOT and np.array_equal(want[1][0].view(np.uint32), g[0, 5:12].view(np.uint32)) and not slot[:, 2:, 2].any()      # no point: no pivot, no step
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    _same(ctx.estimate_scale(frames, g, P, 0, o), want)


@pytest.mark.parametrize("free_pose", [1, 0])
def test_shared_batch_leaves_a_degenerate_slot_out(ctxs, oracles, free_pose):
    """one slot of a SHARED batch below min_points: flagged, its T's bits kept, and the scale exactly what the batch without that slot gives"""
    name, counts = "hand17", (300, 5, 280)
    ctx, orc = ctxs(name), oracles(name)
    frames, g, P = _masked(name, counts)
    o, ro = _options(ctx, fraction=1, free_pose=free_pose, iterations=3)
    want = sr.estimate(orc, frames, g, P, ro)
    slot = want[2][:, sr.STATS:].reshape(4, 3, sr.SLOT_STATS)
    assert (slot[:, 1, 2] == sr.FEW_INLIERS).all() and not slot[:, [0, 2], 2].any() and not want[2][:, 5].any() and want[0][0] != np.float32(1.0)
    assert np.array_equal(want[1][1].view(np.uint32), g[1, 5:12].view(np.uint32))
    got = ctx.estimate_scale(frames, g, P, 0, o)
    _same(got, want)
    two = ctx.estimate_scale(frames[[0, 2]], g[[0, 2]], P[[0, 2]], 0, o)
    assert np.array_equal(two[0].view(np.uint32), got[0].view(np.uint32)) and np.array_equal(two[1].view(np.uint32), got[1][[0, 2]].view(np.uint32))


@pytest.mark.parametrize("mode", [sr.SHARED, sr.PER_SLOT])
def test_more_slots_than_a_solve_block_has_threads(ctxs, oracles, mode):
    """257 slots of explicit poses: SHARED's threads take a second slot each at stride 256 and the slot-order sums run past the block; PER_SLOT needs a second block"""
    name, n = "hand17", 257
    ctx, orc = ctxs(name), oracles(name)
    depth, cams, truth = scene(name, 3)
    pick = np.arange(n) % 3
    many, mc, mp = depth[pick], cams[pick], truth[pick]
    o, ro = _options(ctx, fraction=4, mode=mode, iterations=2)
    want = sr.estimate(orc, many, mc, mp, ro)
    assert not want[2][:, 5].any() and (want[0] != np.float32(1.0)).all()
    _same(ctx.estimate_scale(many, mc, mp, 0, o), want)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def test_device_form_on_a_side_stream_into_guarded_buffers(ctxs, oracles):
    name, B = "hand17", 3
    ctx, orc = ctxs(name), oracles(name)
    depth, cams, truth = scene(name, B)
    for mode, free_pose, explicit in ((sr.SHARED, 1, True), (sr.PER_SLOT, 1, False), (sr.SHARED, 0, False)):
        o, ro = _options(ctx, fraction=1, mode=mode, free_pose=free_pose, iterations=6)
        want = sr.estimate(orc, depth, cams, truth, ro)
        _fill(ctx, name, 0, truth)
        N = want[0].shape[0]; nT, ns = B * 7, want[2].size
        G = 7.0
        d_sc = torch.full((N + 9,), G, dtype=torch.float32, device=DEV); d_T = torch.full((nT + 9,), G, dtype=torch.float32, device=DEV)
        d_s = torch.full((2 * ns + 9,), G, dtype=torch.float32, device=DEV)
        d_depth, d_cams, d_poses = _dev(depth), _dev(cams), _dev(truth)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            ctx.estimate_scale_dev(d_depth.data_ptr(), d_cams.data_ptr(), W, H, B, d_sc.data_ptr() + 4, d_T.data_ptr() + 4, d_s.data_ptr() + 4, d_poses=d_poses.data_ptr() if explicit else None,
                                   which=0, options=o, stream=stream.cuda_stream)
        stream.synchronize()
        sc, T, s = d_sc.cpu().numpy(), d_T.cpu().numpy(), d_s.cpu().numpy()
        assert sc[0] == G and (sc[1 + N:] == G).all() and T[0] == G and (T[1 + nT:] == G).all() and s[0] == G and (s[1 + 2 * ns:] == G).all()      # the guards
        _same((sc[1:1 + N].copy(), T[1:1 + nT].reshape(B, 7), s[1:1 + 2 * ns].copy().view(np.float64).reshape(want[2].shape)), want)


def test_everything_else_is_unchanged_by_an_estimate(ctxs, oracles):
    """the estimate keeps its cloud in the calibration's buffer: the slots' fused cloud reads the same rows afterwards, the model's scale is what it was (a render gives the
    same frame), and ht_calibrate_view and ht_update_views_sync give the same bits whether an estimate ran before them or not"""
    name, B, w, h = "hand17", 3, 80, 60
    ctx, orc = ctxs(name), oracles(name); m = ji.model(name)
    sc = vr.two_view_scene(name, (0, 3, 6), w, h, 180.0)
    depth, cams, truth = sc["depth"], sc["cams"], np.ascontiguousarray(sc["truth"], np.float32)
    guess = np.stack([cr.perturbed(c, 2.0, 0.008) for c in cams[:, 1]])
    opt = ctx.views_default(fraction=2)
    ctx.fuse_views(depth, cams, None, opt)
    ctx.set_state(0, ki.states_of(truth))
    rows, n = ctx.stage_view_rows(0, B)
    frame = ctx.raster_mesh_depth(truth[:1], cams[:1, 0], w, h)
    view0 = np.ascontiguousarray(depth[:, 0]); cam0 = np.ascontiguousarray(cams[:, 0])

    def estimate(mode=sr.SHARED):
        return ctx.estimate_scale(view0, cam0, None, 0, ctx.size_default(fraction=1, mode=mode, scale0=1.1))
    s, T, st = estimate()
    assert not st[:, 5].any() and st[-1, 2] < st[0, 2] and abs(float(s[0]) - 1.0) < abs(1.1 - 1.0)      # the frames show the model's own size: from 1.1 it comes back towards 1
    rows2, n2 = ctx.stage_view_rows(0, B)
    assert np.array_equal(n, n2) and np.array_equal(rows.view(np.uint32), rows2.view(np.uint32)) and (n > 100).all()
    assert np.array_equal(frame, ctx.raster_mesh_depth(truth[:1], cams[:1, 0], w, h))
    view1 = np.ascontiguousarray(depth[:, 1])
    co = ctx.calib_default(fraction=1, iterations=3)
    before = ctx.calibrate_view(view1, guess, None, 0, co)
    estimate(sr.PER_SLOT)
    after = ctx.calibrate_view(view1, guess, None, 0, co)
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1].view(np.uint64), after[1].view(np.uint64))
    start = kr.user_poses(m, ki.states_of(np.stack([ki.truths(name)[3 * i + 1] for i in range(B)])))

    def update(est):
        ctx.tracker_reset(start)
        if est:
            estimate(sr.PER_SLOT)
        poses = ctx.update_views_sync(depth, cams, None, side=64, options=opt, passes=2)
        return [poses, ctx.get_state(0, CAP[name]), ctx.get_state(1, CAP[name])] + list(ctx.tracker_flags(CAP[name]))
    for a, b in zip(update(False), update(True)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refused_calls_leave_the_context_usable(ctxs, oracles):
    from hand_tracking_samples_amd import native
    name, B = "hand17", 3
    ctx, orc = ctxs(name), oracles(name)
    depth, cams, truth = scene(name, B)
    D = ctx.size_default
    E = lambda o, **kw: ctx.estimate_scale(kw.get("depth", depth), kw.get("cams", cams), None, kw.get("which", 0), o)      # noqa: E731
    big = np.zeros((CAP[name] + 1, H, W), np.uint16); bigc = np.tile(cams[:1], (CAP[name] + 1, 1))
    nan, inf = float("nan"), float("inf")
    for call, text in ((lambda: E(D(fraction=0)), "fraction"), (lambda: E(D(mode=2)), "mode"), (lambda: E(D(mode=-1)), "mode"), (lambda: E(D(free_pose=2)), "free_pose"),
                       (lambda: E(D(free_pose=-1)), "free_pose"), (lambda: E(D(iterations=65)), "iterations"), (lambda: E(D(iterations=-1)), "iterations"),
                       (lambda: E(None, which=2), "which is 0"), (lambda: E(None, depth=big, cams=bigc), "batch"),
                       (lambda: E(D(fraction=1), depth=np.zeros((1, 480, 640), np.uint16), cams=cams[:1]), "307200 points"),
                       (lambda: E(D(range_lo=0.5, range_hi=0.4)), "range"), (lambda: E(D(max_dist=0.0)), "max_dist"), (lambda: E(D(damping=-1.0)), "damping"),
                       (lambda: E(D(min_points=-1)), "min_points"),
                       (lambda: E(D(scale0=nan)), "scale0"), (lambda: E(D(scale_lo=inf)), "scale0"), (lambda: E(D(scale_hi=inf)), "scale0"), (lambda: E(D(scale_lo=0.0)), "scale0"),
                       (lambda: E(D(scale0=0.4)), "scale0"), (lambda: E(D(scale0=2.5)), "scale0"), (lambda: E(D(scale_lo=1.5, scale_hi=1.2, scale0=1.3)), "scale0"),
                       (lambda: ctx.estimate_scale_dev(16, 16, W, H, B, 18, 16, 16, options=D()), "4-byte aligned"),
                       (lambda: ctx.estimate_scale_dev(16, 16, W, H, B, 16, 16, 17, options=D()), "4-byte aligned"),
                       (lambda: ctx.estimate_scale_dev(16, 16, W, H, B, None, 16, 16, options=D()), "scale_out"),
                       (lambda: ctx.estimate_scale_dev(None, 16, W, H, B, 16, 16, 16, options=D()), "frames")):
        with pytest.raises(native.HTError, match=text):
            call()
    c2 = native.Context(None, 2)
    try:
        with pytest.raises(native.HTError, match="without a hand model"):
            c2.estimate_scale(depth[:2], cams[:2], None, 0, None)
    finally:
        c2.close()
    # explicit poses are not bounded by the context's slots: more frames than max_batch, and the same call as before still gives the same result
    n = CAP[name] + 2
    o, ro = _options(ctx, fraction=2, iterations=2)
    many = np.tile(depth[:1], (n, 1, 1)); mc = np.tile(cams[:1], (n, 1)); mp = np.tile(truth[:1], (n, 1, 1))
    _same(ctx.estimate_scale(many, mc, mp, 0, o), sr.estimate(orc, many, mc, mp, ro))
    _same(ctx.estimate_scale(depth, cams, truth, 0, o), sr.estimate(orc, depth, cams, truth, ro))
