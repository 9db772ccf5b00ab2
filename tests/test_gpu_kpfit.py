"""GPU: ht_fit_keypoints against tests/kpfit_ref.py, which tests/test_kpfit_ref.py pins on the reference-pinned restatement of the solver.
(1) The call equals, on every float of ht_get_state, a host loop of ht_get_state -> the restatement's rows -> ht_fit_rows: the rows k_keypoint_rows writes are the
restatement's bit for bit and the step loop is ht_fit_rows' own.  (2) Residuals and user poses bit for bit.  (3) One step against the C restatement of the solver,
teacher-forced, inside parity_rule.TIGHT.  (4) Convergence no worse than the restatement loop's.  (5) Device form against host form, slots >= B, refusals.
(6) The C++ example."""
import os
import subprocess

import numpy as np
import pytest
import torch

import joints_inputs as ji
import kpfit_inputs as ki
import kpfit_ref as kr
import oracle_lib as ol
import parity_rule
import quality_ref as Q

pytestmark = pytest.mark.gpu
ROOT = ji.ROOT
DEV = "cuda:0"
CAP = {"hand17": 8, "hand26": 4}
# (model, B, table, steps): hand17 with B = 3, 1 and 8, hand26 with B = 2; SKELETON, FEATURE8, a caller table with K = 1 and with the largest K the row bound admits
CASES = [("hand17", 3, "skeleton", 3), ("hand17", 1, "feature8", 1), ("hand17", 8, "caller1", 6), ("hand17", 8, "callermax", 3), ("hand26", 2, "skeleton", 6)]
# the device-minus-restatement difference of a frame's final mean residual measured on test_convergence's frames, and the margin: 4 x the largest
CONV_DIFF_MAX = 4.23e-9      # metres, hand17 frame 0 (hand26: 3.95e-9); the residuals themselves are 4e-6 .. 6e-5 m
CONV_MARGIN = 4 * CONV_DIFF_MAX


@pytest.fixture(scope="module")
def ctxs():
    from hand_tracking_samples_amd import native
    made = {}

    def get(name):
        if name not in made:
            made[name] = native.Context(ji.model_path(name), CAP[name])
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


def _table(name, which):
    """(the table argument of the wrapper, the table as arrays, kinds of the "mixed" variant)"""
    m = ji.model(name)
    if which == "skeleton":
        t = Q.skeleton(m); return Q.SKELETON, t, ki.mixed_kind(len(t[0]))
    if which == "feature8":
        t = Q.feature8(); return Q.FEATURE8, t, ki.mixed_kind(8)
    if which == "caller1":
        t = (np.array([7], np.int32), np.array([[0.001, 0.002, -0.01]], np.float32), np.array([1], np.int32)); return t, t, np.ones(1, np.int32)
    # 64 entries over every bone, both conventions; 43 points and 21 pixels: 3 * 43 + 4 * 21 = 213 = 5 * 17 + 128 rows, the most a frame's scratch slot holds
    rng = np.random.default_rng(7)
    t = (rng.integers(0, m.nb, 64).astype(np.int32), (rng.standard_normal((64, 3)) * 0.02).astype(np.float32), rng.integers(0, 2, 64).astype(np.int32))
    kind = np.zeros(64, np.int32); kind[rng.permutation(64)[:21]] = 1
    assert 3 * 43 + 4 * 21 == 5 * m.nb + 128
    return t, t, kind


def _case(name, B, which, variant, away=True, weighted=True, seed=11):
    arg, tab, mixed = _table(name, which)
    K = len(tab[0])
    sc = ki.scene(name, B, tab, away=away)
    kind = {"point": np.zeros(K, np.int32), "pixel": np.ones(K, np.int32), "mixed": mixed}[variant]
    if which == "callermax":
        kind = mixed      # all pixels would be 256 rows: refused
    rng = np.random.default_rng(seed)
    state = sc["state"].copy(); state[:, :, 7:13] = rng.standard_normal(state[:, :, 7:13].shape).astype(np.float32) * 1e-3      # momenta to keep or to zero
    tg = dict(kind=kind, xyz=sc["xyz"], pix=sc["pix"], cams=sc["cams"])
    if weighted:
        tg["weights"] = ki.ragged_weights(B, K)
    return ji.model(name), arg, tab, state, tg


def _options(native, steps, keep=False, max_force=1e5):
    return native.kpfit_default(steps=steps, max_force=max_force, keep_momenta=keep)


def _host_loop(ctx, m, tab, state, tg, steps, keep, max_force=1e5):
    """ht_get_state -> the restatement's rows -> ht_fit_rows without points, the momenta zeroed as the flags say; leaves the result in the slots"""
    B = len(state)
    none_p, none_a = [np.zeros((0, 3), np.float32)] * B, [np.zeros((0, 8), np.float32)] * B
    ctx.set_state(0, state)
    for st in range(steps):
        s = ctx.get_state(0, B)
        if not keep:
            s[:, :, 7:13] = 0; ctx.set_state(0, s)
        ctx.fit_rows(0, none_p, kr.rows(m, s, tab, max_force=max_force, **tg), none_a, microforce=float(ctx.params.microforce))
    s = ctx.get_state(0, B)
    if not keep:
        s[:, :, 7:13] = 0; ctx.set_state(0, s)
    return s


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1 and 2: bit for bit against the existing solver; residuals and poses ------------------------------------------------------------------------------------------
RUNS = [(c, v, False) for c in CASES for v in ("point", "pixel", "mixed") if not (c[2] == "callermax" and v != "mixed") and not (c[2] == "caller1" and v == "mixed")]
RUNS += [(CASES[0], "mixed", True), (CASES[2], "point", True), (CASES[4], "pixel", True)]      # HT_KPFIT_KEEP_MOMENTA


@pytest.mark.parametrize("case,variant,keep", RUNS, ids=lambda x: "-".join(str(i) for i in x) if isinstance(x, tuple) else str(x))
def test_equals_the_host_loop_bit_for_bit(ctxs, case, variant, keep):
    from hand_tracking_samples_amd import native
    name, B, which, steps = case
    ctx = ctxs(name)
    m, arg, tab, state, tg = _case(name, B, which, variant)
    K = len(tab[0])
    nrows = [len(r) for r in kr.rows(m, state, tab, **tg)]
    assert B < 3 or K < 2 * B or len(set(nrows)) == B         # every frame another row count ...
    assert B == 1 or nrows[-1] == 0                           # ... and one has none
    ref = _host_loop(ctx, m, tab, state, tg, steps, keep)
    assert np.abs(ref[:, :, :7] - state[:, :, :7]).max() > 1e-4
    ctx.set_state(0, state)
    out = ctx.fit_keypoints(B, arg, options=_options(native, steps, keep), **tg)
    got = ctx.get_state(0, B)
    assert np.array_equal(_bits(got), _bits(ref)), "states differ: %g" % np.abs(got - ref).max()
    assert keep or not got[:, :, 7:13].any()
    # residuals at the start pose and after the last step; the user poses
    rk = {k: v for k, v in tg.items()}
    first = state.copy()
    want = np.stack([kr.residuals(m, first, tab, **rk), kr.residuals(m, got, tab, **rk)], axis=1)
    assert np.array_equal(_bits(out["resid"]), _bits(want))
    assert np.array_equal(_bits(out["poses"]), _bits(kr.user_poses(m, got)))
    assert (out["resid"][:, :, :][tg["weights"][:, None, :].repeat(2, 1) == 0] == -1).all()


def test_identity_camera_and_default_options(ctxs):
    """the nail with ht_kpfit_default's own figures (FLT_MAX, 6 steps) and pixel targets through a camera at the origin, unweighted"""
    ctx = ctxs("hand17")
    for which, variant in (("caller1", "point"), ("feature8", "pixel")):
        m, arg, tab, state, tg = _case("hand17", 3, which, variant, away=False, weighted=False)
        ref = _host_loop(ctx, m, tab, state, tg, 6, False, max_force=kr.FLT_MAX)
        ctx.set_state(0, state)
        ctx.fit_keypoints(3, arg, options=None, want_poses=False, want_resid=False, **tg)
        assert np.array_equal(_bits(ctx.get_state(0, 3)), _bits(ref))


# ---- 3: against the C restatement of the solver, teacher-forced ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4]], ids=lambda c: "-".join(str(i) for i in c))
def test_one_step_against_the_oracle(ctxs, oracles, case):
    from hand_tracking_samples_amd import native
    name, B, which, steps = case
    ctx, orc = ctxs(name), oracles(name)
    m, arg, tab, state, tg = _case(name, B, which, "mixed")
    trace, _ = kr.fit_loop(ol, orc, m, state, tab, steps=steps, max_force=1e5, **tg)
    worst = (0.0, 0.0)
    for st in range(steps):
        ctx.set_state(0, trace[st])
        ctx.fit_keypoints(B, arg, options=_options(native, 1), want_poses=False, want_resid=False, **tg)
        got = ctx.get_state(0, B)
        dp, dq = parity_rule.pose_diff(got, trace[st + 1])
        print("%s step %d: per frame |dpos| %s |dquat| %s" % (name, st, np.array2string(dp, precision=2), np.array2string(dq, precision=2)))
        worst = (max(worst[0], float(dp.max())), max(worst[1], float(dq.max())))
        assert np.isfinite(got).all() and not got[:, :, 7:13].any()
        assert (dp <= parity_rule.TIGHT[0]).all() and (dq <= parity_rule.TIGHT[1]).all(), "step %d leaves the tight band: %g m, %g" % (st, dp.max(), dq.max())
    print("%s: worst |dpos| %.2e m, |dquat| %.2e (TIGHT %s)" % (name, worst[0], worst[1], parity_rule.TIGHT))


# ---- 4: convergence on the device -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hand17", "hand26"])
def test_convergence(ctxs, oracles, name):
    from hand_tracking_samples_amd import native
    ctx, orc, m = ctxs(name), oracles(name), ji.model(name)
    B = CAP[name]
    tab = Q.skeleton(m)
    sc = ki.scene(name, B, tab)
    _, ref = kr.fit_loop(ol, orc, m, sc["state"], tab, steps=10, xyz=sc["xyz"], max_force=1e5)
    ctx.set_state(0, sc["state"])
    out = ctx.fit_keypoints(B, Q.SKELETON, xyz=sc["xyz"], options=_options(native, 10))
    a, b = kr.mean_residual(out["resid"][:, 1]), kr.mean_residual(ref[:, 1])
    print("%s: final mean residual per frame, device %s\n restatement %s\n device - restatement %s (largest %.3g)" % (name, a, b, a - b, (a - b).max()))
    assert np.isfinite(ctx.get_state(0, B)).all()
    assert (kr.mean_residual(out["resid"][:, 1]) < kr.mean_residual(out["resid"][:, 0])).all()
    assert (a <= b + CONV_MARGIN).all()


# ---- 5: device form against host form; slots >= B; refusals -----------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def test_device_form_equals_host_form(ctxs):
    from hand_tracking_samples_amd import native
    name, B, steps = "hand17", 3, 3
    ctx = ctxs(name)
    m, arg, tab, state, tg = _case(name, B, "skeleton", "mixed")
    K = len(tab[0])
    rest = ki.states_of(ki.truths(name)[40:40 + CAP[name] - B]); rest[:, :, 7:13] = 0.25      # slots >= B
    opt = _options(native, steps)
    ctx.set_state(0, state); ctx.set_state(0, rest, first=B); ctx.set_state(1, np.concatenate([state, rest]))
    host = ctx.fit_keypoints(B, arg, options=opt, **tg)
    want = ctx.get_state(0, CAP[name])
    assert np.array_equal(_bits(want[B:]), _bits(rest))                                        # untouched
    assert np.array_equal(_bits(ctx.get_state(1, CAP[name])), _bits(np.concatenate([state, rest])))      # the other model too
    ctx.set_state(0, state)
    d = {k: _dev(tg[k]) for k in ("xyz", "pix", "cams", "weights")}
    d_poses = torch.full((B * m.nb * 7 + 32,), 7.0, dtype=torch.float32, device=DEV); d_resid = torch.full((B * 2 * K + 32,), 7.0, dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.fit_keypoints_dev(B, arg, d_xyz=d["xyz"].data_ptr(), d_pix=d["pix"].data_ptr(), d_cams=d["cams"].data_ptr(), d_weights=d["weights"].data_ptr(), kind=tg["kind"], options=opt,
                              d_poses=d_poses.data_ptr(), d_resid=d_resid.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got = ctx.get_state(0, CAP[name])
    assert np.array_equal(_bits(got), _bits(want))
    p, r = d_poses.cpu().numpy(), d_resid.cpu().numpy()
    assert np.array_equal(_bits(p[:-32].reshape(B, m.nb, 7)), _bits(host["poses"])) and (p[-32:] == 7.0).all()
    assert np.array_equal(_bits(r[:-32].reshape(B, 2, K)), _bits(host["resid"])) and (r[-32:] == 7.0).all()
    # the other model
    ctx.set_state(1, state)
    ctx.fit_keypoints(B, arg, options=opt, which_model=1, want_poses=False, want_resid=False, **tg)
    assert np.array_equal(_bits(ctx.get_state(1, B)), _bits(want[:B])) and np.array_equal(_bits(ctx.get_state(0, CAP[name])), _bits(want))


def test_refused_calls_leave_the_context_usable(ctxs):
    from hand_tracking_samples_amd import native
    name, B = "hand17", 3
    ctx = ctxs(name)
    m, arg, tab, state, tg = _case(name, B, "skeleton", "mixed")
    K = len(tab[0])
    ctx.set_state(0, state)
    bad_w = tg["weights"].copy(); bad_w[0, 5] = 1.5
    nan_w = tg["weights"].copy(); nan_w[1, 0] = np.nan
    def made_up(b, k):
        return dict(xyz=np.zeros((b, k, 3), np.float32), pix=np.zeros((b, k, 2), np.float32), weights=np.ones((b, k), np.float32), cams=ki.camera(max(b, 1))[:b])

    one = (np.array([17], np.int32), np.zeros((1, 3), np.float32), np.array([0], np.int32))        # hand17 has bones 0..16
    pixels = (tab[0].repeat(3)[:64], tab[1].repeat(3, axis=0)[:64], tab[2].repeat(3)[:64])      # 64 pixel targets: 256 rows
    D = native.kpfit_default
    refusals = [
        (dict(B=CAP[name] + 1, **made_up(CAP[name] + 1, K)), "batch"), (dict(B=0, **made_up(0, K)), "batch"), (dict(which_model=2), "which_model"),
        (dict(table=one, kind=None, **made_up(B, 1)), "outside"),
        (dict(kind=np.full(K, 2, np.int32)), "kind is 0"), (dict(table=pixels, kind=np.ones(64, np.int32), **made_up(B, 64)), "caller rows"),
        (dict(xyz=None), "need xyz"), (dict(pix=None), "need pix"), (dict(cams=None), "need pix and cams"),
        (dict(options=D(steps=0)), "steps"), (dict(options=D(steps=65)), "steps"), (dict(options=D(flags=2)), "flags"),
        (dict(options=D(max_force=0.0)), "max_force"), (dict(options=D(max_force=float("nan"))), "max_force"),
        (dict(options=D(ray_radius=-1.0)), "ray_radius"), (dict(options=D(ray_force=0.0)), "ray_force"),
        (dict(weights=bad_w), "weights between"), (dict(weights=nan_w), "weights between"),
    ]
    for change, text in refusals:
        kw = dict(B=B, table=arg, options=None, **tg); kw.update(change)
        with pytest.raises(native.HTError, match=text):
            ctx.fit_keypoints(kw.pop("B"), kw.pop("table"), **kw)
        assert np.array_equal(_bits(ctx.get_state(0, B)), _bits(state)), text
    with pytest.raises(native.HTError, match="which must be"):
        ctx.fit_keypoints_dev(B, 5)
    # an output that overlaps an input (the raw call: the wrapper allocates its own outputs)
    import ctypes as C
    xyz = np.ascontiguousarray(tg["xyz"]); fp = C.POINTER(C.c_float)
    rc = ctx.L.ht_fit_keypoints(ctx.h, 0, B, Q.SKELETON, 0, None, None, None, None, xyz.ctypes.data_as(fp), None, None, None, None, None, xyz.ctypes.data_as(fp))
    assert rc != 0 and b"overlaps" in ctx.L.ht_last_error(ctx.h)
    assert np.array_equal(_bits(ctx.get_state(0, B)), _bits(state))
    # the exact-order solver build serves the update entry points only
    ctx.L.ht_debug_solver_build(ctx.h, 5)
    try:
        with pytest.raises(native.HTError, match="exact-order"):
            ctx.fit_keypoints(B, arg, **tg)
    finally:
        ctx.L.ht_debug_solver_build(ctx.h, 0)
    # a context without a hand model
    c2 = native.Context(None, 2)
    try:
        with pytest.raises(native.HTError, match="without a hand model"):
            c2.L.ht_fit_keypoints.restype = C.c_int
            c2._chk(c2.L.ht_fit_keypoints(c2.h, 0, 1, Q.SKELETON, 0, None, None, None, None, xyz.ctypes.data_as(fp), None, None, None, None, None, None))
    finally:
        c2.close()
    # still usable: the same call as before gives the same result
    ref = _host_loop(ctx, m, tab, state, tg, 2, False)
    ctx.set_state(0, state)
    ctx.fit_keypoints(B, arg, options=_options(native, 2), **tg)
    assert np.array_equal(_bits(ctx.get_state(0, B)), _bits(ref))


# ---- 6: the C++ example -------------------------------------------------------------------------------------------------------------------------------------------------
def test_cxx_example_prints_the_c_calls_residuals(ctxs, tmp_path):
    """tests/cxx_kpfit_example.cpp: HandTracker::fit_keypoints on frame 1's ground truth towards frame 0's skeleton keypoints, 6 steps; the same through the C calls"""
    from hand_tracking_samples_amd import native
    exe = str(tmp_path / "kpfit")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_kpfit_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    m = ji.model("hand17"); tab = Q.skeleton(m)
    sc = ki.scene("hand17", 1, tab)
    pose_file, target_file = tmp_path / "start.f32", tmp_path / "targets.f32"
    np.ascontiguousarray(sc["state"][0, :, :7]).tofile(pose_file); sc["xyz"].astype(np.float32).tofile(target_file)
    r = subprocess.run([exe, ji.model_path("hand17"), str(pose_file), str(target_file)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    ctx = ctxs("hand17")
    ctx.set_state(0, sc["state"])
    out = ctx.fit_keypoints(1, Q.SKELETON, xyz=sc["xyz"], options=native.kpfit_default(max_force=1e5))
    lines = [l for l in r.stdout.splitlines() if l.startswith("resid ")]
    got = np.array([[float.fromhex(x) for x in l.split()[1:]] for l in lines], np.float32)
    assert np.array_equal(_bits(got), _bits(out["resid"][0]))
