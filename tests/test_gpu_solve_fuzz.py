"""k_solve through ht_physics_update, the door that takes arbitrary caller-built rows, on the seeded scenes of tests/solve_scenes.py: against PhysicsUpdate in float64
(tests/solve_ref.py), bit for bit between the builds, slots, strides and contexts, and refusal by refusal.  The golden frames, the teacher-forced steps and the bit pins feed
k_solve one body graph (the hand's); these scenes give the host's grouping, the level schedule, the angular runs and the single-body chains body graphs and row counts
a tracked hand never produces.

The bound.  BOUND(quantity, family) = 8 x E_ref(quantity, family), E_ref = max |fp32 restatement - float64| over the family's scenes (tests/solve_oracle.py; pinned and
put against mutated references by tests/test_solve_ref.py).  The product applies the same rows in the same order with the same clamps as the restatement and differs in
association only (Jacobian form, fused multiply-adds, coefficients formed once): a few roundings per row application.  No bound comes from the device's output.

What the door does not let through.  A caller hands over at most 126 angular rows per frame (include/ht_mi355x.h, upload_angulars): more are refused before anything
is uploaded.  So the counts beyond that which k_solve itself holds or drops (127 to 252 rows in the build with four row slots per lane, more than 252 rows, more than
128 runs) cannot be reached through it; those lists are checked here as refusals, and the capacity counters stay zero on every family.  More than 128 runs are reached
through ht_fit_rows, where the model's joint rows follow the caller's (test_more_angular_runs_than_the_schedule_holds): dropped and counted, as documented.

Build 4 (nothing in LDS) is a test build whose lanes hold two angular rows each like the ordinary builds (126 rows); the launcher moves builds 1 to 3 to the build with
four slots when a call may carry more, and the scenes end at 126 rows, so every build listed keeps every row.

HT_SOLVE_FUZZ_REPORT=<file>: the device's measured ratio max |device - f64| / E_ref per family and quantity, merged into that JSON (profiles/solve_fuzz.json)."""
import ctypes as C
import time

import numpy as np
import pytest

import solve_oracle as so
import solve_scenes as ss
from test_solve_ref import merge_report

pytestmark = pytest.mark.gpu
BUILDS = (0, 1, 2, 3, 4, 6)
FAMILIES = tuple(ss.FAMILIES)
SLOTS = {"hand17": 64, "hand26": 32}


@pytest.fixture(scope="module")
def contexts():
    from hand_tracking_samples_amd import native
    made = {}

    def get(family, fresh=False):
        """the family's context: one per model with a slot per scene; chains_long, whose prefixes make the context grow its per-point arrays, has a small one of its own.
        fresh: a new context of two slots, the caller's to close"""
        name = ss.scenes(family)[0]["model"]
        if fresh:
            return native.Context(ss.MODEL_PATH[name], 2)
        key = "long" if family == "chains_long" else name
        if key not in made:
            made[key] = native.Context(ss.MODEL_PATH[name], 4 if key == "long" else SLOTS[name])
        return made[key]
    yield get
    for c in made.values():
        c.close()


def _pack(rows, width, extra):
    cap = max(1, max(len(r) for r in rows)) + extra
    buf = np.full((len(rows), cap, width), np.nan, np.float32)      # what lies behind a frame's rows is never read: NaN would show
    for i, r in enumerate(rows):
        buf[i, :len(r)] = r
    return buf, np.array([len(r) for r in rows], np.int32), cap


def solve(ctx, scenes, build=0, lextra=0, aextra=0):
    """the scenes in slots 0.. of model 0 through ht_physics_update -> states [S,nb,13]"""
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lb, ln, lc = _pack([sc["lin"] for sc in scenes], 16, lextra); ab, an, ac = _pack([sc["ang"] for sc in scenes], 8, aextra)
    ctx.set_params(physics_use_collision=1 if scenes[0]["collide"] else 0)
    ctx.set_state(0, np.stack([sc["state"] for sc in scenes]))
    ctx.debug_solver_build(build)
    rc = ctx.L.ht_physics_update(ctx.h, 0, len(scenes), lb.ctypes.data_as(fp), lc, ln.ctypes.data_as(ip), ab.ctypes.data_as(fp), ac, an.ctypes.data_as(ip))
    if rc:      # every scene is one the call accepts: a status here is the device's, and nothing more is started on it
        pytest.exit("ht_physics_update: %s (status %d)" % (ctx.L.ht_last_error(ctx.h).decode(), rc), returncode=1)
    ctx.debug_solver_build(0)
    return ctx.get_state(0, len(scenes))


@pytest.fixture(scope="module")
def product(contexts):
    """the product build's answer to every family, computed once and left unchanged: {family: states}"""
    got = {}

    def get(family):
        if family not in got:
            ctx = contexts(family)
            if family == "chains_long":
                assert ctx.point_capacity() == ss.POINT_CAPACITY      # every prefix of the family is longer than what the context holds: the call grows it
            before = ctx.capacity_events()
            got[family] = solve(ctx, ss.scenes(family))
            if family == "chains_long":
                assert ctx.point_capacity() >= ss.POINT_CAPACITY + 65
            assert ctx.capacity_events() == before, "a capacity counter moved on %s" % family
            got[family].setflags(write=False)
        return got[family]
    return get


def _ratios(family, states, select=None):
    _, s64, _ = so.restated(family)
    keep = np.arange(len(s64)) if select is None else np.array(select)
    d, e = so.distance(states, s64[keep]), so.e_ref(family)
    return {q: float(d[q].max() / e[q]) for q in d}


@pytest.mark.parametrize("family", FAMILIES)
def test_against_float64(contexts, product, family):
    t0 = time.time()
    r = _ratios(family, product(family))
    print("solve fuzz %s: max |device - f64| / E_ref %s (%.2f s)" % (family, {q: "%.2f" % v for q, v in r.items()}, time.time() - t0))
    merge_report("device_ratio", family, r)
    assert np.all(np.isfinite(product(family)))
    assert all(v <= so.FACTOR for v in r.values()), r


@pytest.mark.parametrize("family", ["chains", "angular", "with_contacts"])
def test_level_schedule_for_every_frame(contexts, family):
    """build 7 takes the two-body and angular rows of every frame by the level schedule; on the frames the blocked form holds (no caller's two-body row, no angular row
    that RemoveBias switches on) that is another order of evaluation of the same rows, and meets the same bound"""
    scenes = ss.scenes(family)
    keep = [k for k, sc in enumerate(scenes) if not sc["tail"] and not sc["switched"]]
    assert len(keep) >= 16
    ctx = contexts(family)
    r = _ratios(family, solve(ctx, [scenes[k] for k in keep], build=7), keep)
    print("solve fuzz %s, build 7: %s" % (family, {q: "%.2f" % v for q, v in r.items()}))
    merge_report("device_ratio_build7", family, r)
    assert all(v <= so.FACTOR for v in r.values()), r


@pytest.mark.parametrize("family", FAMILIES)
def test_builds_return_the_same_bits(contexts, product, family):
    ctx = contexts(family)
    for build in BUILDS[1:]:
        assert np.array_equal(solve(ctx, ss.scenes(family), build=build), product(family)), "build %d" % build
    assert ctx.capacity_events() == (0, 0, 0)


@pytest.mark.parametrize("family", FAMILIES)
def test_slots_batch_and_strides_do_not_matter(contexts, product, family):
    scenes = ss.scenes(family); ctx = contexts(family)
    assert np.array_equal(solve(ctx, scenes[::-1]), product(family)[::-1]), "reversed slot order"
    for k in (0, len(scenes) - 1):
        assert np.array_equal(solve(ctx, [scenes[k]])[0], product(family)[k]), "scene %d alone" % k
    assert np.array_equal(solve(ctx, scenes, lextra=37, aextra=11), product(family)), "larger strides"


@pytest.mark.parametrize("family", FAMILIES)
def test_smallest_scene_after_the_largest(contexts, product, family):
    """nothing of a large solve is left where a small one reads it (LDS tables, the scratch slot's tail, d_user_pos, grown buffers): the scene with the fewest rows, run
    in the slots the scene with the most rows just used, gives the bits a context made for it gives"""
    scenes = ss.scenes(family)
    size = [len(sc["lin"]) + len(sc["ang"]) for sc in scenes]
    small, large = scenes[int(np.argmin(size))], scenes[int(np.argmax(size))]
    fresh = contexts(family, fresh=True)
    try:
        want = solve(fresh, [small, small])
    finally:
        fresh.close()
    ctx = contexts(family)
    solve(ctx, [large, large])
    assert np.array_equal(solve(ctx, [small, small]), want)
    assert np.array_equal(want[0], product(family)[int(np.argmin(size))])


def test_more_angular_runs_than_the_schedule_holds(contexts):
    """ht_fit_rows with the caller's angular rows in runs of one row: with the model's 16 joint runs behind them, 112 rows make the 128 runs the schedule holds, more rows
    make more.  Then the rows from run 128 on are dropped and the solve is counted: the result is the reference's on the rows that are kept, and the counter of solves over
    their angular capacity moves for exactly those scenes."""
    ctx = contexts("angular")
    callers, kept = ss.many_runs(), so.scenes("many_runs")
    assert [sc["runs"] for sc in kept] == [128, 129, 136, 142] and [sc["dropped"] for sc in kept] == [False, True, True, True]
    ctx.set_params(physics_use_collision=0)
    got = []
    for sc, k in zip(callers, kept):
        before = ctx.capacity_events()
        ctx.set_state(0, sc["state"][None])
        ctx.fit_rows(0, [np.zeros((0, 3), np.float32)], [np.zeros((0, 16), np.float32)], [sc["ang"]], microforce=1.0)
        got.append(ctx.get_state(0, 1)[0])
        assert tuple(np.subtract(ctx.capacity_events(), before)) == (0, 0, 1 if k["dropped"] else 0)
    r = _ratios("many_runs", np.stack(got))
    print("solve fuzz many_runs: %s" % {q: "%.2f" % v for q, v in r.items()})
    merge_report("e_ref", "many_runs", so.e_ref("many_runs")); merge_report("bound", "many_runs", so.bound("many_runs")); merge_report("device_ratio", "many_runs", r)
    assert all(v <= so.FACTOR for v in r.values()), r


def _refused(ctx, text, lin, ang, stride=None, build=0):
    from hand_tracking_samples_amd import native
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lin, ang = np.ascontiguousarray(lin, np.float32).reshape(-1, 16), np.ascontiguousarray(ang, np.float32).reshape(-1, 8)
    nl, na = np.array([len(lin)], np.int32), np.array([len(ang)], np.int32)
    lc, ac = stride if stride else (max(1, len(lin)), max(1, len(ang)))
    lb = np.zeros((max(lc, len(lin), 1), 16), np.float32); lb[:len(lin)] = lin
    ab = np.zeros((max(ac, len(ang), 1), 8), np.float32); ab[:len(ang)] = ang
    before, caps = ctx.get_state(0, 4), ctx.capacity_events()
    ctx.debug_solver_build(build)
    try:
        with pytest.raises(native.HTError, match=text):
            ctx._chk(ctx.L.ht_physics_update(ctx.h, 0, 1, lb.ctypes.data_as(fp), lc, nl.ctypes.data_as(ip), ab.ctypes.data_as(fp), ac, na.ctypes.data_as(ip)))
    finally:
        ctx.debug_solver_build(0)
    assert np.array_equal(ctx.get_state(0, 4).view(np.uint32), before.view(np.uint32)) and ctx.capacity_events() == caps


def test_refusals(contexts):
    """what ht_physics_update documents as refused: HTError with the documented text, and the slots' state as it was, bit for bit"""
    ctx = contexts("groups"); nb = ctx.nb
    rng = np.random.default_rng(ss.SEED + 9)
    ctx.set_params(physics_use_collision=0)
    ctx.set_state(0, np.stack([ss._state(rng, "hand17", k) for k in range(4)]))
    friction, index, count = "friction row must directly follow its master", "body index out of range", "row count is negative or exceeds the stride"
    ok_ang = ss._angular_rows(rng, [2, 3])
    one = lambda **kw: ss.lin_row(rng, 2, 5, **kw)
    # 33 groups: 32 pass (the groups family), one more does not
    _refused(ctx, "more than 32 groups", ss._tail(rng, "chain", 32) + ss._tail(rng, "star", 1), ok_ang)
    t = ss._triple(rng, 2, 5)
    _refused(ctx, friction, [t[0], t[2], t[1]], ok_ang)                                   # friction_master -2 directly behind the master
    other = ss._triple(rng, 2, 6)
    _refused(ctx, friction, [t[0], other[1], t[2]], ok_ang)                               # a friction row on another body pair
    _refused(ctx, friction, [t[1], t[2]] + ss._tail(rng, "chain", 2), ok_ang)             # a friction row as the first row
    _refused(ctx, friction, [ss.lin_row(rng, -1, 5, 0.0, 0.0, fm=-1)], ok_ang)            # ... acting from the world
    _refused(ctx, friction, t + [t[2]], ok_ang)                                           # a third friction row
    _refused(ctx, index, [one(), ss.lin_row(rng, -1, -1)], ok_ang)                        # both bodies NULL
    _refused(ctx, index, [one(), ss.lin_row(rng, 3, nb)], ok_ang)                         # body index = nb, linear: rb1, rb0
    _refused(ctx, index, [ss.lin_row(rng, nb, 3)], ok_ang)
    _refused(ctx, "angular rows: " + index, [one()], ok_ang + [ss.ang_row(rng, 1, nb)])   # ... angular
    _refused(ctx, "angular rows: " + index, [one()], [ss.ang_row(rng, nb, 1)])
    _refused(ctx, count, [one(), one(), one()], ok_ang, stride=(2, 8))                    # more rows than the stride
    _refused(ctx, "angular rows: a count is negative, exceeds the stride", [one()], ok_ang, stride=(4, 4))
    _refused(ctx, "exact-order instantiation", [one()], ok_ang, build=5)
    for sc in ss.too_many_angular():                                                      # more than 126 angular rows: refused, not dropped
        _refused(ctx, "angular rows: a count is negative, exceeds the stride, exceeds 126", sc["lin"], sc["ang"])
    # and the slots still solve: the context is as good as before
    scenes = ss.scenes("groups")[:4]
    assert np.array_equal(solve(ctx, scenes), solve(ctx, scenes))
