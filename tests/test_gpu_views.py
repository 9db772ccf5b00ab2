"""GPU: several views (include/ht_mi355x.h "several views") against tests/views_ref.py, which tests/test_views_ref.py pins on the oracle.
(1) The fused cloud -- points, sources, counts, origins -- bit for bit: hand17 with B = 3 and V = 1, 2, 4, hand26 with B = 2 and V = 2, fraction 1 and 4, a view without
a pixel in range, cameras away from the origin, a mirror inside a posed view, the mirror scene; cut exactly at the capacity and one point over; the device form on a side
stream into odd-aligned guarded buffers.  (2) One identity view is the cloud ht_stage_prepare leaves.  (3) ht_stage_view_rows is the restated rows.  (4) Every origin
zero: ht_fit_views is ht_fit_rows on the fused xyz.  (5) Passes against the oracle, teacher-forced, inside parity_rule.TIGHT on every frame; slots >= B and the other
model left alone.  (6) ht_update_views_* is the existing update, the fused cloud and the fit, byte for byte.  (7) Refusals that need a device."""
import functools

import numpy as np
import pytest
import torch

import joints_inputs as ji
import kpfit_inputs as ki
import kpfit_ref as kr
import oracle_lib as ol
import parity_rule
import views_ref as vr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = {"hand17": 4, "hand26": 2}
# (model, B, V, w, h, fraction)
CASES = [("hand17", 3, 1, 37, 29, 4), ("hand17", 3, 2, 37, 29, 1), ("hand17", 3, 4, 80, 60, 4), ("hand26", 2, 2, 37, 29, 1)]
EPS = 0.005      # the mirror inside a posed view cuts through the hand: a thin coplanar band, so that all three classes occur


@pytest.fixture(scope="module")
def ctxs(weights):
    from hand_tracking_samples_amd import native
    made = {}

    def get(name):
        if name not in made:
            made[name] = native.Context(ji.model_path(name), CAP[name])
            made[name].set_params(microforce=3.0)      # force limits that differ between the wrist bodies and the rest
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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


@functools.lru_cache(None)
def scene(name, B, V, w, h):
    """slot i: frame 3 i's ground truth seen by the frame camera and by V - 1 cameras on orbits about its palm, each lifted off the orbit (no camera but view 0's sits at
    the origin).  V >= 2: slot 1's second view sees nothing (an empty frame).  V = 4: view 1 of every slot holds a mirror plane through the palm's depth in its own space"""
    P = ki.truths(name); cam0 = vr.frame_camera(w, h)
    degrees = {1: (), 2: (180.0,), 4: (90.0, 180.0, 270.0)}[V]
    depth, cams, planes, truth = [], [], [], []
    for i in range(B):
        pose = P[(3 * i) % len(P)]
        cv = [cam0] + [vr.orbit(cam0, vr.palm(pose), d, lift=(0.01 * (i + 1), -0.02, 0.015 * k)) for k, d in enumerate(degrees)]
        dv = [vr.render(name, pose, c, w, h) for c in cv]
        if V >= 2 and i == 1:
            dv[1] = np.zeros_like(dv[1])
        pl = [vr.NONE_PLANE.copy() for _ in cv]
        if V == 4:
            pl[1] = np.array([0, 0, -1, vr.palm(pose)[2]], np.float32)      # the palm keeps its place in the camera's own space on the orbit (before the lift)
        depth.append(np.stack(dv)); cams.append(np.stack(cv)); planes.append(np.stack(pl)); truth.append(pose)
    return dict(depth=np.stack(depth), cams=np.stack(cams), planes=np.stack(planes) if V == 4 else None, truth=np.stack(truth))


def _stale(name, B):
    """the start states: the ground truth a frame on"""
    P = ki.truths(name)
    return ki.states_of(np.stack([P[(3 * i + 1) % len(P)] for i in range(B)]))


def _same_cloud(got, ref, B, V):
    assert got["npoints"].tolist() == ref["npoints"].tolist() and got["cut"] == ref["cut"]
    assert np.array_equal(got["per_source"], ref["per_source"])
    assert np.array_equal(_bits(got["origins"]), _bits(ref["origins"]))
    for b in range(B):
        n = ref["npoints"][b]
        assert np.array_equal(_bits(got["points"][b, :n]), _bits(ref["points"][b])), "slot %d: %d of %d points differ" % (b, int((_bits(got["points"][b, :n]) != _bits(ref["points"][b])).any(1).sum()), n)


# ---- 1: the fused cloud -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(i) for i in c))
def test_fused_cloud_equals_the_restatement(ctxs, case):
    name, B, V, w, h, fraction = case
    ctx = ctxs(name); sc = scene(name, B, V, w, h)
    opt = ctx.views_default(fraction=fraction, mirror_eps=EPS)
    ref = vr.fuse(sc["depth"], sc["cams"], sc["planes"], 0.1, opt.range_hi, fraction, EPS)
    got = ctx.fuse_views(sc["depth"], sc["cams"], sc["planes"], opt)
    _same_cloud(got, ref, B, V)
    assert (ref["per_source"][:, 0] > 10).all()
    if V >= 2:
        assert ref["per_source"][1, 2] == 0 and (ref["per_source"][[0, B - 1][:B - 1], 2] > 10).all()      # the view that sees nothing (slot 1), beside views that do
        assert (np.abs(ref["origins"][:, 2:]).max(axis=2)[:, ::2] > 0.01).all()                    # cameras away from the origin
    if V == 4:
        seen = [0]      # (slot 1's view sees nothing, and slot 2's hand lies wholly in front of its mirror)
        assert (ref["per_source"][seen, 2:4] > 0).all() and (ref["per_source"][:, [5, 7]] == 0).all()      # the mirror inside the posed view: direct and virtual points
        assert (ref["per_source"][seen, 2:4].sum(1) < vr.fuse(sc["depth"], sc["cams"], None, 0.1, opt.range_hi, 1, EPS)["per_source"][seen, 2]).all()      # and a coplanar band dropped


def test_mirror_scene(ctxs):
    ctx = ctxs("hand17")
    ms = vr.mirror_scene("hand17", (0, 3), 80, 60)
    opt = ctx.views_default(fraction=1, range_hi=0.9)
    ref = vr.fuse(ms["depth"], ms["cams"], ms["planes"], 0.1, 0.9, 1, opt.mirror_eps)
    _same_cloud(ctx.fuse_views(ms["depth"], ms["cams"], ms["planes"], opt), ref, 2, 1)
    assert (ref["per_source"] > 20).all()


def test_cut_at_the_capacity_and_one_over(ctxs):
    name, B, V, w, h, fraction = CASES[1]
    ctx = ctxs(name); sc = scene(name, B, V, w, h)
    opt = ctx.views_default(fraction=fraction)
    full = vr.fuse(sc["depth"], sc["cams"], None, 0.1, opt.range_hi, fraction)
    n0 = int(full["npoints"][0])
    assert n0 == full["npoints"].max() and (full["npoints"][1:] < n0 - 1).all()
    for cap, cut in ((n0, 0), (n0 - 1, 1), (int(full["npoints"][1]) - 1, 3)):      # exactly the capacity; one point over it; every slot over it
        ref = vr.fuse(sc["depth"], sc["cams"], None, 0.1, opt.range_hi, fraction, cap=cap)
        got = ctx.fuse_views(sc["depth"], sc["cams"], None, opt, cap=cap)
        assert ref["cut"] == cut
        _same_cloud(got, ref, B, V)
        assert got["points"].shape[1] == cap and (got["npoints"] <= cap).all()


def test_device_form_on_a_side_stream_into_guarded_buffers(ctxs):
    name, B, V, w, h, fraction = CASES[2]
    ctx = ctxs(name); sc = scene(name, B, V, w, h)
    opt = ctx.views_default(fraction=fraction, mirror_eps=EPS)
    ref = vr.fuse(sc["depth"], sc["cams"], sc["planes"], 0.1, opt.range_hi, fraction, EPS)
    d_depth, d_cams, d_planes = _dev(sc["depth"]), _dev(sc["cams"]), _dev(sc["planes"])
    G = 7.0
    outs = {k: torch.full((n + 9,), G, dtype=t, device=DEV) for k, n, t in (("n", B, torch.int32), ("per", B * 2 * V, torch.int32), ("org", B * 2 * V * 3, torch.float32), ("cut", 1, torch.int32))}
    ptr = {k: v.data_ptr() + 4 for k, v in outs.items()}      # one word into the allocation: 4-byte aligned and no more
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.fuse_views_dev(d_depth.data_ptr(), d_cams.data_ptr(), w, h, V, B, d_planes=d_planes.data_ptr(), options=opt, d_npoints=ptr["n"], d_per_source=ptr["per"], d_origins=ptr["org"],
                           d_cut=ptr["cut"], stream=stream.cuda_stream)
    stream.synchronize()
    o = {k: v.cpu().numpy() for k, v in outs.items()}
    for k, want in (("n", ref["npoints"]), ("per", ref["per_source"].reshape(-1)), ("cut", np.array([0], np.int32))):
        assert np.array_equal(o[k][1:1 + want.size], want) and o[k][0] == 7 and (o[k][1 + want.size:] == 7).all(), k
    assert np.array_equal(_bits(o["org"][1:1 + B * 2 * V * 3]), _bits(ref["origins"].reshape(-1))) and o["org"][0] == G and (o["org"][1 + B * 2 * V * 3:] == G).all()
    # the cloud it left in the slots is the host form's: the rows of both are the same
    ctx.set_state(0, _stale(name, B))
    rows_dev, n_dev = ctx.stage_view_rows(0, B, cap=int(ref["npoints"].max()))
    ctx.fuse_views(sc["depth"], sc["cams"], sc["planes"], opt)
    rows_host, n_host = ctx.stage_view_rows(0, B, cap=int(ref["npoints"].max()))
    assert np.array_equal(n_dev, ref["npoints"]) and np.array_equal(n_host, n_dev) and np.array_equal(_bits(rows_dev), _bits(rows_host)) and rows_dev.any()


# ---- 2: one identity view is the existing cloud ---------------------------------------------------------------------------------------------------------------------------
def test_single_identity_view_is_the_prepared_cloud(ctxs, golden):
    ctx = ctxs("hand17")
    depth = np.stack([golden["f%d/depth" % f].reshape(64, 64) for f in range(3)]); cams = np.stack([golden["f%d/cam" % f] for f in range(3)]).astype(np.float32)
    cams[:, 5:] = (0, 0, 0, 0, 0, 0, 1)
    _, pts, n = ctx.stage_prepare(depth.reshape(3, -1), cams)
    got = ctx.fuse_views(depth[:, None], cams[:, None], None, None)      # the tracker's own range and fraction
    assert np.array_equal(got["npoints"], n) and (n > 100).all()
    for b in range(3):
        assert np.array_equal(_bits(got["points"][b, :n[b]]), _bits(pts[b, :n[b]]))      # .w included: source 0 is the 0 k_prepare writes
    assert np.array_equal(got["per_source"], np.stack([n, np.zeros_like(n)], 1)) and not got["origins"].any() and got["cut"] == 0


# ---- 3: the rows ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused(ctxs):
    """per case: the scene, the restated cloud and the start states (computed once)"""
    @functools.lru_cache(None)
    def get(case):
        name, B, V, w, h, fraction = case
        sc = scene(name, B, V, w, h)
        opt = ctxs(name).views_default(fraction=fraction, mirror_eps=EPS)
        return sc, opt, vr.fuse(sc["depth"], sc["cams"], sc["planes"], 0.1, opt.range_hi, fraction, EPS), _stale(name, B)
    return get


def _restated_rows(ctx, orc, state, ref, B):
    p = ctx.params
    return [vr.rows(ol, orc, 0, state[b], ref["points"][b], ref["origins"][b], p.microforce, p.physics_weak_force) for b in range(B)]


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[3]], ids=lambda c: "-".join(str(i) for i in c))
def test_view_rows_equal_the_restated_rows(ctxs, oracles, fused, case):
    name, B = case[0], case[1]
    ctx, orc = ctxs(name), oracles(name)
    sc, opt, ref, state = fused(case)
    ctx.fuse_views(sc["depth"], sc["cams"], sc["planes"], opt)
    ctx.set_state(0, state)
    rows, n = ctx.stage_view_rows(0, B, cap=int(ref["npoints"].max()) + 3)
    want = _restated_rows(ctx, orc, state, ref, B)
    hits = 0
    for b in range(B):
        assert n[b] == len(want[b])
        bad = (_bits(rows[b, :n[b]]) != _bits(want[b])).any(axis=1)
        assert not bad.any(), "slot %d: %d of %d rows differ, the first at %d (source %d)" % (b, int(bad.sum()), n[b], int(np.flatnonzero(bad)[0]), int(ref["points"][b][np.flatnonzero(bad)[0], 3]))
        assert not rows[b, n[b]:].any()
        hits += int((np.abs(want[b][:, 8:11] - want[b][0, 8:11]).max() > 0))
    assert hits == B


# ---- 4: every origin zero ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_zero_origins_equal_fit_rows_on_the_fused_points(ctxs):
    """cameras turned about the origin, not moved: every ray starts at zero, which is ht_fit_rows' origin; one pass on every float of the state"""
    name, B, w, h = "hand17", 3, 37, 29
    ctx = ctxs(name); P = ki.truths(name); cam0 = vr.frame_camera(w, h)
    cams = np.stack([np.stack([cam0, vr.turned(cam0, 4.0 + i), vr.turned(cam0, -3.0, (1.0, 0.2 * i, 0.0))]) for i in range(B)])
    depth = np.stack([np.stack([vr.render(name, P[3 * i], c, w, h) for c in cams[i]]) for i in range(B)])
    opt = ctx.views_default(fraction=1)
    cloud = ctx.fuse_views(depth, cams, None, opt)
    assert not cloud["origins"].any() and (cloud["per_source"][:, ::2] > 10).all()
    state = _stale(name, B); state[:, :, 7:13] = np.random.default_rng(2).standard_normal(state[:, :, 7:13].shape).astype(np.float32) * 1e-3
    ctx.set_state(0, state)
    ctx.fit_views(0, B, 1)
    got = ctx.get_state(0, B)
    ctx.set_state(0, state)
    none = [np.zeros((0, 16), np.float32)] * B
    ctx.fit_rows(0, [cloud["points"][b, :cloud["npoints"][b], :3] for b in range(B)], none, [np.zeros((0, 8), np.float32)] * B, microforce=float(ctx.params.microforce))
    want = ctx.get_state(0, B)
    assert np.abs(want[:, :, :7] - state[:, :, :7]).max() > 1e-4
    assert np.array_equal(_bits(got), _bits(want)), "states differ by %g" % np.abs(got - want).max()


# ---- 5: the passes against the oracle ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1], CASES[3], "mirror"], ids=lambda c: c if isinstance(c, str) else "-".join(str(i) for i in c))
def test_passes_against_the_oracle_teacher_forced(ctxs, oracles, fused, case):
    if case == "mirror":
        name, B = "hand17", 2
        ms = vr.mirror_scene(name, (0, 3), 80, 60)
        opt = ctxs(name).views_default(fraction=4, range_hi=0.9)
        sc, ref = ms, vr.fuse(ms["depth"], ms["cams"], ms["planes"], 0.1, 0.9, 4, opt.mirror_eps)
        state = ki.states_of(np.stack([vr.moved(ki.truths(name)[f + 1], (-0.05, 0.0, 0.35)) for f in (0, 3)]))      # near the hand in front of the mirror
    else:
        name, B = case[0], case[1]
        sc, opt, ref, state = fused(case)
    ctx, orc = ctxs(name), oracles(name)
    full = CAP[name]
    rest = ki.states_of(ki.truths(name)[40:40 + full - B]); rest[:, :, 7:13] = 0.25
    other = np.concatenate([state, rest])
    ctx.fuse_views(sc["depth"], sc["cams"], sc.get("planes"), opt)
    cur = state.copy(); worst = (0.0, 0.0)
    for p in range(3):
        rws = _restated_rows(ctx, orc, cur, ref, B)
        nxt = np.stack([vr.oracle_pass(ol, orc, 0, cur[b], rws[b]) for b in range(B)])
        ctx.set_state(0, cur)
        if full > B:
            ctx.set_state(0, rest, first=B)
        ctx.set_state(1, other)
        ctx.fit_views(0, B, 1, want_poses=False)
        got = ctx.get_state(0, full)
        dp, dq = parity_rule.pose_diff(got[:B], nxt)
        print("%s pass %d: per frame |dpos| %s |dquat| %s" % (name, p, np.array2string(dp, precision=2), np.array2string(dq, precision=2)))
        worst = (max(worst[0], float(dp.max())), max(worst[1], float(dq.max())))
        assert np.isfinite(got).all()
        assert (dp <= parity_rule.TIGHT[0]).all() and (dq <= parity_rule.TIGHT[1]).all(), "pass %d leaves the tight band: %g m, %g" % (p, dp.max(), dq.max())
        assert np.array_equal(_bits(got[B:]), _bits(rest)) and np.array_equal(_bits(ctx.get_state(1, full)), _bits(other))      # slots >= B and the other model
        assert np.abs(nxt[:, :, :3] - cur[:, :, :3]).max() > 1e-5
        cur = nxt
    print("%s: worst |dpos| %.2e m, |dquat| %.2e over 3 passes (TIGHT %s)" % (case, worst[0], worst[1], parity_rule.TIGHT))


def test_three_passes_are_three_single_passes_and_the_device_form(ctxs, fused):
    """momenta kept from pass to pass, nothing else between them; the poses are GetPoseUser of the last state; the _dev form on a side stream; the other model"""
    case = CASES[1]; name, B = case[0], case[1]
    ctx = ctxs(name); m = ji.model(name)
    sc, opt, ref, state = fused(case)
    ctx.fuse_views(sc["depth"], sc["cams"], sc["planes"], opt)
    flags = ctx.tracker_flags(B)
    ctx.set_state(0, state)
    for _ in range(3):
        ctx.fit_views(0, B, 1, want_poses=False)
    want = ctx.get_state(0, B)
    assert want[:, :, 7:13].any()
    ctx.set_state(0, state)
    poses = ctx.fit_views(0, B, 3)
    assert np.array_equal(_bits(ctx.get_state(0, B)), _bits(want)) and np.array_equal(_bits(poses), _bits(kr.user_poses(m, want)))
    f2 = ctx.tracker_flags(B)
    assert np.array_equal(flags[0], f2[0]) and np.array_equal(flags[1], f2[1])      # the tracker's flags are not touched
    ctx.set_state(0, state)
    d_poses = torch.full((B * m.nb * 7 + 8,), 7.0, dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.fit_views_dev(0, B, 3, d_poses=d_poses.data_ptr() + 4, stream=stream.cuda_stream)
    stream.synchronize()
    p = d_poses.cpu().numpy()
    assert np.array_equal(_bits(ctx.get_state(0, B)), _bits(want)) and np.array_equal(_bits(p[1:1 + poses.size]), _bits(poses.reshape(-1))) and p[0] == 7 and (p[1 + poses.size:] == 7).all()
    ctx.set_state(1, state); before = ctx.get_state(0, B)
    ctx.fit_views(1, B, 3, want_poses=False)
    assert np.array_equal(_bits(ctx.get_state(1, B)), _bits(want)) and np.array_equal(_bits(ctx.get_state(0, B)), _bits(before))


def test_small_cloud_against_fit_rows_with_the_rows_as_linears(ctxs, oracles):
    """Clouds of at most 5 nb + 128 rows fit ht_fit_rows' caller rows: the same rows solved as linears give the same state bit for bit (measured so on the device, DESIGN
    section 37: k_view_rows' records are the ones k_solve's prologue makes of the same rows, in the same chain order)."""
    name, B, V, w, h = "hand17", 3, 2, 37, 29
    ctx, orc = ctxs(name), oracles(name); sc = scene(name, B, V, w, h)
    opt = ctx.views_default(fraction=8)
    ref = vr.fuse(sc["depth"], sc["cams"], None, 0.1, opt.range_hi, 8)
    assert 20 < ref["npoints"].max() <= 5 * 17 + 128
    state = _stale(name, B)
    ctx.fuse_views(sc["depth"], sc["cams"], None, opt)
    ctx.set_state(0, state); ctx.fit_views(0, B, 1, want_poses=False)
    got = ctx.get_state(0, B)
    ctx.set_state(0, state)
    ctx.fit_rows(0, [np.zeros((0, 3), np.float32)] * B, _restated_rows(ctx, orc, state, ref, B), [np.zeros((0, 8), np.float32)] * B, microforce=float(ctx.params.microforce))
    want = ctx.get_state(0, B)
    dp, dq = parity_rule.pose_diff(got, want)
    print("ht_fit_views against ht_fit_rows(linears = rows): bit for bit %s; |dpos| %s |dquat| %s" % (np.array_equal(_bits(got), _bits(want)), dp, dq))
    assert np.array_equal(_bits(got), _bits(want))


# ---- 6: the update ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_update_views_is_update_then_fuse_then_fit(ctxs):
    name, B, V, w, h = "hand17", 3, 2, 80, 60
    ctx = ctxs(name); m = ji.model(name); sc = scene(name, B, 4, w, h)
    depth, cams = np.ascontiguousarray(sc["depth"][:, :V]), np.ascontiguousarray(sc["cams"][:, :V])
    start = kr.user_poses(m, _stale(name, B))
    opt = ctx.views_default(fraction=2)
    # the parts, one call each
    ctx.tracker_reset(start)
    poses0 = ctx.update_frames_sized_sync(depth[:, 0], cams[:, 0], side=64)      # the view-0 part IS the existing call: what the fused passes start from
    ctx.fuse_views(depth, cams, None, opt)
    want_poses = ctx.fit_views(0, B, 3)
    want = [ctx.get_state(0, B), ctx.get_state(1, B)] + list(ctx.tracker_flags(B))
    assert np.abs(want_poses - poses0).max() > 1e-5
    # the call
    ctx.tracker_reset(start)
    poses, cnn = ctx.update_views_sync(depth, cams, None, side=64, options=opt, passes=3, want_cnn=True)
    got = [ctx.get_state(0, B), ctx.get_state(1, B)] + list(ctx.tracker_flags(B))
    assert np.array_equal(_bits(poses), _bits(want_poses)) and np.isfinite(cnn).all() and cnn.any()
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the device form on a side stream, start poses given
    d_depth, d_cams, d_start = _dev(depth), _dev(cams), _dev(start)
    d_poses = torch.full((B * m.nb * 7 + 8,), 7.0, dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.update_views_dev(64, d_depth.data_ptr(), d_cams.data_ptr(), w, h, V, 0.17, d_start.data_ptr(), B, d_poses.data_ptr(), options=opt, passes=3, stream=stream.cuda_stream)
    stream.synchronize()
    p = d_poses.cpu().numpy()
    assert np.array_equal(_bits(p[:poses.size]), _bits(poses.reshape(-1))) and (p[poses.size:] == 7).all()
    assert np.array_equal(_bits(ctx.get_state(0, B)), _bits(want[0]))
    # one view: the frames are taken where they lie
    ctx.tracker_reset(start)
    ctx.update_frames_sized_sync(depth[:, 0], cams[:, 0], side=64); ctx.fuse_views(depth[:, :1], cams[:, :1], None, opt); one = ctx.fit_views(0, B, 1)
    ctx.tracker_reset(start)
    assert np.array_equal(_bits(ctx.update_views_sync(depth[:, :1], cams[:, :1], None, side=64, options=opt, passes=1)), _bits(one))


# ---- 7: refusals that need a device ----------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_context_usable(ctxs, fused):
    from hand_tracking_samples_amd import native
    case = CASES[1]; name, B, V, w, h, fraction = case
    ctx = ctxs(name)
    sc, opt, ref, state = fused(case)
    ctx.set_state(0, state)
    D = ctx.views_default
    big = scene(name, B, 4, 80, 60)
    posed0 = big["cams"][:, :2].copy(); posed0[0, 0, 5] = 0.01
    for call, text in ((lambda: ctx.fuse_views(sc["depth"], sc["cams"], None, D(fraction=0)), "fraction"), (lambda: ctx.fuse_views(sc["depth"], sc["cams"], None, D(range_lo=0.8)), "range"),
                       (lambda: ctx.fuse_views(sc["depth"], sc["cams"], None, D(mirror_eps=-1.0)), "mirror_eps"),
                       (lambda: ctx.fuse_views(np.zeros((1, 5, 8, 8), np.uint16), np.zeros((1, 5, 12), np.float32)), "HT_VIEWS_MAX"),
                       (lambda: ctx.fuse_views(np.zeros((CAP[name] + 1, 1, 8, 8), np.uint16), np.zeros((CAP[name] + 1, 1, 12), np.float32)), "batch"),
                       (lambda: ctx.fuse_views(sc["depth"], sc["cams"], np.zeros((B, V, 4), np.float32)), "zero normal"),
                       (lambda: ctx.fuse_views_dev(1, 1, 320, 240, 4, 1, options=D(fraction=1)), "307200 points"),
                       (lambda: ctx.fit_views(0, B, 0), "passes"), (lambda: ctx.fit_views(2, B, 1), "which is 0"), (lambda: ctx.stage_view_rows(0, CAP[name] + 1, cap=8), "batch"),
                       (lambda: ctx.update_views_sync(big["depth"][:, :2], posed0, None, side=64), "must be identity"), (lambda: ctx.update_views_sync(sc["depth"], sc["cams"], None, side=64), "multiple of 4")):
        with pytest.raises(native.HTError, match=text):
            call()
        assert np.array_equal(_bits(ctx.get_state(0, B)), _bits(state)), text
    # the exact-order solver build serves the update entry points only
    ctx.fuse_views(sc["depth"], sc["cams"], None, opt)
    ctx.L.ht_debug_solver_build(ctx.h, 5)
    try:
        with pytest.raises(native.HTError, match="exact-order"):
            ctx.fit_views(0, B, 1)
    finally:
        ctx.L.ht_debug_solver_build(ctx.h, 0)
    # a context without a hand model, and one that has not fused anything
    c2 = native.Context(None, 2)
    try:
        with pytest.raises(native.HTError, match="without a hand model"):
            c2.fuse_views(sc["depth"][:2], sc["cams"][:2])
        with pytest.raises(native.HTError, match="without a hand model"):
            c2.fit_views(0, 1, 1)
    finally:
        c2.close()
    c3 = native.Context(ji.model_path(name), 2)
    try:
        with pytest.raises(native.HTError, match="no fused cloud"):
            c3.fit_views(0, 1, 1)
        c3.fuse_views(sc["depth"][:1], sc["cams"][:1], None, opt)
        with pytest.raises(native.HTError, match="no fused cloud"):
            c3.fit_views(0, 2, 1)      # one slot was fused
    finally:
        c3.close()
    # still usable: the same call as before gives the same result
    ctx.set_state(0, state)
    _same_cloud(ctx.fuse_views(sc["depth"], sc["cams"], sc["planes"], opt), ref, B, V)
    assert np.array_equal(_bits(ctx.get_state(0, B)), _bits(state))


# ---- 8: the C++ example -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_cxx_example_prints_the_c_calls_figures(ctxs, weights, tmp_path):
    """tests/cxx_views_example.cpp: HandTracker::FuseViews on a posed second view with a mirror in it, then HandTracker::update_views; the same through the C calls"""
    import os
    import subprocess
    from hand_tracking_samples_amd import native, weights as W
    name, w, h, V = "hand17", 80, 60, 2
    ctx = ctxs(name); m = ji.model(name); sc = scene(name, 3, 4, w, h)
    depth, cams, planes = np.ascontiguousarray(sc["depth"][:1, :V]), np.ascontiguousarray(sc["cams"][:1, :V]), np.ascontiguousarray(sc["planes"][:1, :V])
    start = kr.user_poses(m, _stale(name, 1))
    exe = str(tmp_path / "views"); libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ji.ROOT, "tests", "cxx_views_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    files = {k: str(tmp_path / k) for k in ("frames.u16", "cams.f32", "planes.f32", "w.cnnb", "start.f32")}
    depth.tofile(files["frames.u16"]); cams.tofile(files["cams.f32"]); planes.tofile(files["planes.f32"]); start.astype(np.float32).tofile(files["start.f32"]); W.save_cnnb(files["w.cnnb"], weights)
    r = subprocess.run([exe, ji.model_path(name), str(w), str(h), files["frames.u16"], files["cams.f32"], files["planes.f32"], files["w.cnnb"], files["start.f32"]], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    ctx.set_params(microforce=1.0)      # a fresh tracker's
    try:
        opt = ctx.views_default(fraction=1)
        cloud = ctx.fuse_views(depth, cams, planes, opt)
        n = int(cloud["npoints"][0]); p = cloud["points"][0, :n]
        lines = r.stdout.splitlines()
        assert lines[0] == "views=%d points=%d cut=0" % (V, n)
        for s in range(2 * V):
            sel = p[p[:, 3] == s]
            tot = np.zeros(3, np.float32)
            for q in sel:
                tot = tot + q[:3]
            f = lines[1 + s].split()
            assert f[:3] == ["source", str(s), "n=%d" % cloud["per_source"][0, s]]
            got = np.array([float.fromhex(x) for x in f[4:7] + f[8:11]], np.float32)
            assert np.array_equal(_bits(got), _bits(np.concatenate([tot, cloud["origins"][0, s]])))
        assert cloud["per_source"][0, 2] > 0 and cloud["per_source"][0, 3] > 0
        ctx.tracker_reset(start)
        want = ctx.update_views_sync(depth, cams, planes, side=64, options=opt, passes=3)
        got = np.array([float.fromhex(x) for x in [l for l in lines if l.startswith("pose ")][0].split()[1:]], np.float32)
        assert np.array_equal(_bits(got), _bits(want.reshape(-1)))
    finally:
        ctx.set_params(microforce=3.0)
