"""The head of an update: the launch tables made from the previous update's per-frame costs (k_contact_order, k_rank_desc: each over many blocks, every place of a
table written exactly once per launch) and the side branches beside the net (FitError and the reset decision on one stream, the tables and the boundary planes on the other).

First the tables alone, from cost arrays made here, against a NumPy restatement of the rule (the header comment of k_contact_order): a table that loses or repeats a
frame fails here, before any update uses it.  Then whole updates on the overlapped route against the serial route of the phase profile (profile_enable(2): every kernel
in order on one stream), three in a row so that the second and third run on tables made from history: equal bit for bit.
"""
import numpy as np
import pytest
import torch  # noqa: F401  -- at import time on purpose (tests/test_gpu_comm.py): torch's copy of the runtime finds no device once the library has initialised HIP first

import oracle_lib as ol

pytestmark = pytest.mark.gpu
NB = 17
SEG = 4096
# a share that is not full, a last int4 that is not full, one frame more than a segment (4095 frames with three per block), two segments and a remainder
TABLE_B = (2, 5, 64, 255, 256, 257, 1027, 4096, 4100, 8200)


def _ceil(a, b):
    return (a + b - 1) // b


def contact_order_rule(work, nfr, epb):
    """k_contact_order restated: [nfr, blocks] with table[round, block] = frame, B = no frame.  Segment by segment (the most whole blocks within 4096 frames): the frames
    sorted by min(runs, 1023) << 20 | pairs, largest first, ties by index; those with polytope runs dealt back and forth, epb to a block, over the first neb blocks;
    of the others the heaviest back and forth over the remaining blocks and the lightest into the places the first blocks have left."""
    Ball = len(work); seg = (SEG // nfr) * nfr; blocks_all = _ceil(Ball, nfr)
    table = np.full((nfr, blocks_all), Ball, np.int64)
    for f0 in range(0, Ball, seg):
        w = work[f0:f0 + seg].astype(np.int64); B = len(w); b0 = f0 // nfr; blocks = _ceil(B, nfr)
        runs = np.where(w < 0, 0, w >> 16); pairs = np.where(w < 0, 0, w & 0xffff)
        key = np.where(w < 0, -1, (np.minimum(runs, 1023) << 20) | pairs)
        frames = np.argsort(-key, kind="stable"); rank = np.arange(B)
        ne = int((runs > 0).sum()); ng = B - ne
        e = min(epb, nfr)
        if e * blocks < ne:
            e = _ceil(ne, blocks)
        neb = _ceil(ne, e); ngb = blocks - neb
        nfree = neb * nfr - ne; nheavy = max(ng - nfree, 0)
        first = rank < ne; second = ~first & (rank - ne < nheavy)
        nb_ = np.where(second, ngb, neb); base = np.where(second, neb, 0)
        r = np.where(first, rank, np.where(second, rank - ne, rank - nheavy))
        rnd = r // np.maximum(nb_, 1); pos = r - rnd * nb_
        col = np.where(rnd & 1, nb_ - 1 - pos, pos)
        assert (rnd < nfr).all() and (col >= 0).all() and (base + col < blocks).all()
        table[rnd, b0 + base + col] = f0 + frames
    return table


def rank_desc_rule(work):
    """k_rank_desc restated: every 4096-frame segment's frames by work, largest first, ties by index"""
    out = np.empty(len(work), np.int64)
    for f0 in range(0, len(work), SEG):
        out[f0:f0 + SEG] = f0 + np.argsort(-work[f0:f0 + SEG].astype(np.int64), kind="stable")
    return out


def _work_patterns(B):
    """{name: work[B]}, work = candidate pairs + 2 x patches | polytope runs << 16"""
    rng = np.random.default_rng(B)
    pairs = rng.integers(0, 300, B)      # many equal keys among them: the ties go by index
    few = np.where(rng.random(B) < 0.1, rng.integers(1, 12, B), 0)
    few[rng.integers(0, B)] = 3          # at least one frame with runs
    clamp = few.copy(); clamp[[0, B - 1]] = (1500, 2000); clamp[B // 2] = 1023      # above the clamp: one key, then pairs, then index
    return {"all keys equal": np.full(B, 57), "no frame with runs": pairs, "every frame with runs": pairs | (rng.integers(1, 9, B) << 16),
            "a tenth with runs": pairs | (few << 16), "runs above the clamp": pairs | (clamp << 16)}


@pytest.fixture(scope="module")
def small_ctx():
    from hand_tracking_samples_amd import native
    c = native.Context(ol.MODEL, 8)
    yield c
    c.close()


@pytest.mark.parametrize("B", TABLE_B)
def test_contact_order_tables_equal_the_rule(small_ctx, B):
    for name, work in _work_patterns(B).items():
        work = work.astype(np.int32)
        for nfr in (3, 4):
            for epb in (1, nfr):
                got = small_ctx.debug_contact_order(work, nfr, epb)
                what = "B = %d, %s, nfr = %d, epb = %d" % (B, name, nfr, epb)
                seen = np.bincount(got.reshape(-1).clip(0, B), minlength=B + 1)
                assert got.min() >= 0 and got.max() <= B, what + ": a place nobody wrote, or no frame"
                assert (seen[:B] == 1).all(), what + ": frames lost %s, repeated %s" % (np.flatnonzero(seen[:B] == 0)[:8], np.flatnonzero(seen[:B] > 1)[:8])
                assert seen[B] == got.size - B, what
                assert np.array_equal(got, contact_order_rule(work, nfr, epb)), what


@pytest.mark.parametrize("B", TABLE_B)
def test_rank_desc_tables_equal_the_rule(small_ctx, B):
    for name, work in _work_patterns(B).items():
        got = small_ctx.debug_rank_desc(work.astype(np.int32))
        what = "B = %d, %s" % (B, name)
        assert np.array_equal(np.sort(got), np.arange(B)), what + ": not a permutation of the frames"
        assert np.array_equal(got, rank_desc_rule(work)), what


def _three_updates(c, depth, cams, start, serial, call):
    """three consecutive updates without re-seeding; after each: what the call returned, both states, the tracker flags, the reset decision"""
    B = len(depth); out = []
    c.profile_enable(2 if serial else 0)
    try:
        c.tracker_reset(start)
        for _ in range(3):
            res = call(c, depth, cams)
            out.append(tuple(res) + (c.get_state(0, B), c.get_state(1, B), np.stack(c.tracker_flags(B), 1), c.debug_reset_flags(B)))
    finally:
        c.profile_enable(0)
    return out


def _assert_routes_equal(c, depth, cams, start, call, what):
    a = _three_updates(c, depth, cams, start, False, call); b = _three_updates(c, depth, cams, start, True, call)
    for u in range(3):
        names = ["result %d" % i for i in range(len(a[u]) - 4)] + ["handmodel", "othermodel", "tracker flags", "reset flags"]
        for x, y, n in zip(a[u], b[u], names):
            assert np.isfinite(x.astype(np.float64)).all() and np.array_equal(x, y), "%s, update %d: %s" % (what, u, n)
    assert c.capacity_events() == (0, 0, 0)
    return a


def _update(c, depth, cams):
    return (c.update_sync(depth, cams),)


def _kickstart(c, depth, cams):
    return c.update_cnn_model_sync(depth, cams, kickstart=True)


@pytest.fixture(scope="module")
def frames(golden):
    """eight frames: six golden ones, a frame with a 64-point cloud and an empty one; B = 3 takes a golden, the 64-point and the empty frame"""
    import test_gpu_pass_tail as pt
    L = ol.lib()
    depth = [np.ascontiguousarray(golden["f%d/depth" % f].reshape(-1)) for f in range(8)]
    cams = np.stack([golden["f%d/cam" % f] for f in range(8)]).astype(np.float32)
    start = np.stack([golden["f%d/startpose" % f] for f in range(8)]).astype(np.float32)
    depth[1] = pt._cut_to(L, depth[1], ol.camera(cams[1]), 64)
    depth[2] = np.zeros_like(depth[2])
    return np.stack(depth), cams, start


ONE_STEP = dict(steps=1, steps_cloudstart=1, steps_keypoints=1, steps_keyangles=1, steps_palmangle=1)
CASES = [("default", {}, _update, None), ("one step", ONE_STEP, _update, None), ("kickstart", {}, _kickstart, None),
         ("every frame resets", dict(full_reset_on_error=0.0), _update, True), ("no frame resets", dict(full_reset_on_error=1e30), _update, False)]


@pytest.mark.parametrize("name,params,call,resets", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_overlapped_update_equals_the_serial_route(frames, weights, name, params, call, resets):
    from hand_tracking_samples_amd import native
    depth, cams, start = frames
    c = native.Context(ol.MODEL, 8)
    try:
        c.load_weights(weights)
        c.set_params(microforce=3.0, mainthreadpasses=3, **params)
        for B in (3, 5, 8):
            got = _assert_routes_equal(c, depth[:B], cams[:B], start[:B], call, "%s, B = %d" % (name, B))
            if resets is not None:      # the state the case is about (the golden frames carry a cloud, so their error is above zero)
                for u in range(3):
                    flags = got[u][-1]
                    assert (flags[0] and flags[B - 1 if B > 3 else 0]) if resets else not flags.any(), "%s, B = %d, update %d: reset flags %s" % (name, B, u, flags.tolist())
    finally:
        c.close()


def test_overlapped_update_equals_the_serial_route_with_a_solve_history(golden, weights):
    """2056 frames (the golden frames over and over): the smallest batch above eight rounds per CU, from which on the solves keep a cost history -- the only way the
    product reaches k_rank_desc."""
    from hand_tracking_samples_amd import native
    B = 2056; idx = np.arange(B) % 8
    depth = np.stack([golden["f%d/depth" % f].reshape(-1) for f in range(8)])[idx]
    cams = np.stack([golden["f%d/cam" % f] for f in range(8)]).astype(np.float32)[idx]
    start = np.stack([golden["f%d/startpose" % f] for f in range(8)]).astype(np.float32)[idx]
    c = native.Context(ol.MODEL, B)
    try:
        c.load_weights(weights)
        c.set_params(microforce=3.0, mainthreadpasses=3)
        _assert_routes_equal(c, depth, cams, start, _update, "2056 frames")
    finally:
        c.close()
