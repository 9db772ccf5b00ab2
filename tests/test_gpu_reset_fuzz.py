"""k_reset (csrc/ht_cloud.hip: PoseFromScratch, then rounds of UnibodyFit) on the seeded scenes of tests/reset_scenes.py, against the fp32 restatement and the float64
statement of tests/reset_oracle.py.  Needs an MI355X: pytest -m gpu.

What is held to what:
    PoseFromScratch (n_unibody = 0), product build and exact-order build: the restatement's state bit for bit.
    The exact-order build (ht_debug_solver_build 5) after 1, 2, 3 rounds: the restatement bit for bit -- the stride-4 rows from the camera's position, UnibodyFit's limits,
        the re-expression on the proxy body and the pose move, over every edge of the row and point counts.
    The product build after round 1: within 8 x E_ref(1) of the float64 round; after rounds 2 and 3: within 8 x (E_ref(k) + S(k)) of the restatement's chain, on the scenes
        tests/test_reset_ref.py keeps.  Its three solve organisations round differently by design; nothing tighter holds across them.
    The model's momenta: zero after PoseFromScratch, and no round touches them.
    Slots, blocks that take several frames in turn, and the listed launch (ht_stage_scratch_unibody_listed: k_reset<1> and k_reset<2> through the flagged-frame list): bit
        for bit what the same scene gives in a batch of eight.

The float64 rounds of all scenes are one batched solve of some fifteen seconds, made once for the module; the device runs once per (build, rounds) and is shared.
HT_RESET_FUZZ_REPORT=<file>: the device's largest ratio to its bound per family and round is merged into that JSON (profiles/reset_fuzz.json)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch      # before the library is loaded, as the other GPU tests that use both have it

pytestmark = pytest.mark.gpu

import reset_oracle as ro
import reset_scenes as rs

BATCH = 8
POSE = ("position", "quaternion")


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------------------------
_ctx = {}


def context(model, slots=16):
    from hand_tracking_samples_amd import native
    if (model, slots) not in _ctx:
        _ctx[(model, slots)] = native.Context(rs.model_path(model), slots)
    return _ctx[(model, slots)]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def stage(ctx, scs, build=0):
    """the scenes' clouds, cameras and start poses into slots 0 .. len(scs) - 1; -> their analyses [B,84]"""
    from hand_tracking_samples_amd import native
    B = len(scs)
    assert len({(sc["model"], sc["unibody_force"]) for sc in scs}) == 1
    ctx.set_params(unibody_force=scs[0]["unibody_force"])
    ctx.debug_solver_build(build)
    ctx.stage_decode(np.full((B, native.CNN_OUT), 0.01, np.float32), np.stack([sc["cam"] for sc in scs]))      # uploads the cameras the pose-driven stages use
    ctx.set_points([sc["cloud"] for sc in scs])
    assert ctx.point_capacity() == rs.CAPACITY
    ctx.tracker_reset(np.stack([sc["start"] for sc in scs]))
    return np.stack([sc["analysis"] for sc in scs])


def run(ctx, scs, rounds, build=0):
    """-> states [B,nb,13] of the scenes after PoseFromScratch and `rounds` rounds of UnibodyFit, all slots in one unlisted call"""
    an = stage(ctx, scs, build)
    ctx.stage_scratch_unibody(an, len(scs), rounds)
    return ctx.get_state(1, len(scs))


@functools.lru_cache(None)
def device(build, rounds):
    """every scene through the device in batches of BATCH that share a model and a unibody_force -> [scene] states [nb,13]"""
    scs = rs.scenes()
    groups = {}
    for i, sc in enumerate(scs):
        groups.setdefault((sc["model"], sc["unibody_force"]), []).append(i)
    out = [None] * len(scs)
    for (model, _), idx in groups.items():
        for at in range(0, len(idx), BATCH):
            part = idx[at:at + BATCH]
            got = run(context(model), [scs[i] for i in part], rounds, build)
            for j, i in enumerate(part):
                out[i] = got[j].copy()
    return out


@pytest.fixture(scope="module")
def refs():
    ro.prepare((1, 2, 3))
    return ro.chain()


def _where(sc):
    return "%s (n %d, nr %d, path %s)" % (sc["name"], sc["n"], sc["nr"], sc["path"])


def _bits(got, ref, what):
    bad = [_where(sc) + ": max |d| %.2e" % np.abs(g.astype(np.float64) - r[:len(g)]).max() for sc, g, r in zip(rs.scenes(), got, ref) if not np.array_equal(g, r[:len(g)])]
    assert not bad, "%s differs from the restatement on %d scenes: %s" % (what, len(bad), "; ".join(bad[:8]))


def _within(got, ref, bounds, keep, what, section):
    """every kept scene within its family's bound, quantity by quantity; the family's largest ratio is printed, reported and returned"""
    scs = rs.scenes()
    ratio, bad = {f: 0.0 for f in rs.FAMILIES}, []
    same = sum(1 for i in keep if np.array_equal(got[i], ro.chain()[i][int(section[-1])][:len(got[i])]))
    print("%s: %d of %d scenes hold the restatement's bits" % (what, same, len(keep)))
    for i, sc in enumerate(scs):
        if i not in keep:
            continue
        d = ro.distance(got[i], np.asarray(ref[i])[:len(got[i])])
        assert not np.any(got[i][:, 7:13]), _where(sc) + ": the model's momenta are not zero"
        for q in POSE:
            r = d[q] / bounds[sc["family"]][q]
            ratio[sc["family"]] = max(ratio[sc["family"]], r)
            if r > 1.0:
                bad.append("%s: %s %.2e against %.2e" % (_where(sc), q, d[q], bounds[sc["family"]][q]))
    print("%s, largest |device - reference| / bound per family: %s" % (what, {f: "%.3f" % v for f, v in ratio.items()}))
    for f, v in ratio.items():
        ro.merge_report(f, "device_ratio", {section: v})
    assert not bad, "%s beyond the bound on %d scenes: %s" % (what, len(bad), "; ".join(bad[:8]))
    return ratio


# ---- 1, 2: bit for bit ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [0, 5])
def test_pose_from_scratch_bit_exact(refs, build):
    """every scene, product build and exact-order build: PoseFromScratch alone equals the restatement's bit for bit -- the weights of every pass of 256 points, the sums in
    the reference's order with their eight-term read-ahead and its tail, the curl by every clench angle, FixPositions"""
    _bits(device(build, 0), [r[0] for r in refs], "PoseFromScratch, build %d" % build)


@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_exact_order_build_bit_exact(refs, rounds):
    _bits(device(5, rounds), [r[rounds] for r in refs], "exact-order build, %d rounds" % rounds)


# ---- 3, 4, 5: the product build against its bounds -------------------------------------------------------------------------------------------------------------------
def test_paths_are_covered():
    counts = rs.path_counts()
    for f in rs.FAMILIES:
        print("%s: %s" % (f, counts[f]))
    for p in rs.PATHS:
        assert sum(counts[f][p] for f in rs.FAMILIES) >= 6, p


def test_product_build_round_1(refs):
    """within 8 x E_ref(1) of the float64 round from the restatement's PoseFromScratch state (which the device holds bit for bit, above)"""
    _within(device(0, 1), ro.f64(1), ro.bound(1), ro.kept(1), "product build, round 1", "round1")


@pytest.mark.parametrize("rounds", [2, 3])
def test_product_build_rounds_2_and_3(refs, rounds):
    """within 8 x (E_ref(k) + S(k)) of the restatement's chain, on the scenes no nudge of rounding size flips"""
    _within(device(0, rounds), [r[rounds] for r in refs], ro.bound(rounds), ro.kept(rounds), "product build, round %d" % rounds, "round%d" % rounds)


# ---- 6: the seams between the three organisations -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [(448, 449), (896, 897)])
def test_path_seams(refs, rows):
    """one cloud cut either side of a seam: each side obeys its own bound, and the device's step across the seam is the float64 statement's step to within the two bounds
    together.  (The cuts differ by a row, so the results differ by that row's doing; the organisations round differently by design, and nothing tighter holds.)"""
    scs = rs.scenes()
    a, b = [[i for i, sc in enumerate(scs) if sc["family"] == "edges" and sc["model"] == "hand17" and sc["nr"] == nr][0] for nr in rows]
    assert scs[a]["path"] != scs[b]["path"] and np.array_equal(scs[a]["cloud"], scs[b]["cloud"][:scs[a]["n"]])
    got, want, bound = device(0, 1), ro.f64(1), ro.bound(1)["edges"]
    nb = len(got[a])
    for q, sl in ro.QUANTITIES[:2]:
        da, db = np.abs(got[a][:, sl] - want[a][:nb, sl]).max(), np.abs(got[b][:, sl] - want[b][:nb, sl]).max()
        step = np.abs((got[b][:, sl].astype(np.float64) - got[a][:, sl]) - (want[b][:nb, sl] - want[a][:nb, sl])).max()
        print("seam %d | %d rows, %s: %.2e and %.2e of %.2e; the step across differs by %.2e" % (rows[0], rows[1], q, da, db, bound[q], step))
        assert da <= bound[q] and db <= bound[q] and step <= 2 * bound[q], (_where(scs[a]), _where(scs[b]), q)


# ---- 7, 8: slots and blocks -----------------------------------------------------------------------------------------------------------------------------------------------
def _edge(nr):
    return [sc for sc in rs.family("edges") if sc["model"] == "hand17" and sc["nr"] == nr][0]


def _index(sc):
    return [i for i, s in enumerate(rs.scenes()) if s is sc][0]


def test_slots_are_independent(refs):
    """one batch mixes the three organisations and an empty cloud; in three slot orders every scene gives the same bits (those of its batch of eight).  A batch of two
    afterwards leaves the slots behind it as they were."""
    mix = [_edge(nr) for nr in (1024, 0, 17, 449, 448, 897, 33, 896)]
    assert {sc["path"] for sc in mix} == set(rs.PATHS)
    want = device(0, 3)
    ctx = context("hand17")
    for order in (list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], [3, 0, 6, 1, 7, 4, 2, 5]):
        got = run(ctx, [mix[j] for j in order], 3)
        for slot, j in enumerate(order):
            assert np.array_equal(got[slot], want[_index(mix[j])]), "slot %d of order %s: %s" % (slot, order, _where(mix[j]))
    before = ctx.get_state(1, 8)
    two = run(ctx, [mix[2], mix[5]], 3)
    after = ctx.get_state(1, 8)
    assert np.array_equal(two[0], want[_index(mix[2])]) and np.array_equal(two[1], want[_index(mix[5])])
    assert np.array_equal(after[2:], before[2:])


def test_blocks_that_take_several_frames():
    """A context of 2 x CUs + 8 slots: the unlisted launch has 2 x CUs blocks, so eight of them take a second frame; the listed launch of few frames has one block per CU,
    so eight take three frames in turn and the others two (no launch shape gives a block four frames at this size).  Nearly every cloud is under 64 points; slots b,
    b + CUs and b + 2 CUs of the first blocks hold, block by block, every consecutive pair of the cycle HBM-path frame -> empty frame -> 17-row frame -> LDS-path frame
    -> HBM-path frame, so a block goes from planes to records to the next frame's weighted points across every change of organisation.  Every slot equals its scene's
    result from a batch of eight, bit for bit."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * cus + 8
    small = [_edge(nr) for nr in (0, 1, 2, 15)] + [sc for sc in rs.family("thin") if sc["model"] == "hand17" and sc["n"] in (2, 4)]
    assert all(sc["n"] < 64 for sc in small)
    cycle = [_edge(1024), _edge(0), _edge(17), _edge(449)]
    assert [sc["path"] for sc in cycle] == ["hbm", "blocked16", "blocked16", "lds"] and cycle[1]["n"] == 0 and cycle[2]["nr"] == 17
    slots = [small[s % len(small)] for s in range(B)]
    for b in range(4):
        for turn in range(3):      # the listed launch: block b takes entries b, b + CUs, b + 2 CUs
            slots[b + turn * cus] = cycle[(b + turn) % 4]
    for b in range(4, 8):          # the unlisted launch: block b takes slots b and b + 2 CUs
        slots[b] = cycle[b % 4]; slots[b + 2 * cus] = cycle[(b + 1) % 4]
    want = device(0, 3)
    ctx = context("hand17", B)
    got = run(ctx, slots, 3)
    for s in range(B):
        assert np.array_equal(got[s], want[_index(slots[s])]), "unlisted, slot %d: %s" % (s, _where(slots[s]))
    for many in (False, True):
        an = stage(ctx, slots)
        ctx.stage_scratch_unibody_listed(an, B, 3, np.arange(B), many_frames=many)
        got = ctx.get_state(1, B)
        for s in range(B):
            assert np.array_equal(got[s], want[_index(slots[s])]), "listed (many_frames %d), slot %d: %s" % (many, s, _where(slots[s]))


# ---- 9: the listed door ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listed():
    """eight scenes of the three organisations, their unlisted result, and their context"""
    mix = [_edge(nr) for nr in (449, 16, 1024, 0, 31, 895, 897, 2)]
    ctx = context("hand17")
    return ctx, mix, run(ctx, mix, 3)


def _start_state(ctx, mix):
    an = stage(ctx, mix)
    return an, ctx.get_state(1, len(mix))


@pytest.mark.parametrize("many", [False, True])
def test_listed_frames_equal_the_unlisted_call(listed, many):
    """the listed frames, in shuffled order, hold the unlisted call's bits (k_reset<1> for many_frames 0, k_reset<2> for 1); the others keep their state and row counts"""
    ctx, mix, want = listed
    run(ctx, mix, 1)                      # every slot's row count set by a launch
    rows_before = ctx.row_counts(8)
    assert rows_before.tolist() == [sc["nr"] for sc in mix]
    an, start = _start_state(ctx, mix)
    frames = [5, 2, 7, 0]
    ctx.set_points([sc["cloud"][:max(0, sc["n"] - 8)] if j not in frames else sc["cloud"] for j, sc in enumerate(mix)])      # a launch that touched an unlisted frame would leave another row count
    ctx.stage_scratch_unibody_listed(an, 8, 3, frames, many_frames=many)
    got, rows_after = ctx.get_state(1, 8), ctx.row_counts(8)
    for j in range(8):
        if j in frames:
            assert np.array_equal(got[j], want[j]), _where(mix[j])
            assert rows_after[j] == mix[j]["nr"]
        else:
            assert np.array_equal(got[j], start[j]) and rows_after[j] == rows_before[j], _where(mix[j])


@pytest.mark.parametrize("many", [False, True])
def test_listed_none_and_all(listed, many):
    ctx, mix, want = listed
    an, start = _start_state(ctx, mix)
    rows_before = ctx.row_counts(8)
    ctx.stage_scratch_unibody_listed(an, 8, 3, np.zeros(0, np.int32), many_frames=many)
    assert np.array_equal(ctx.get_state(1, 8), start) and np.array_equal(ctx.row_counts(8), rows_before)      # nlist = 0 changes nothing
    ctx.stage_scratch_unibody_listed(an, 8, 3, [6, 1, 3, 0, 7, 2, 5, 4], many_frames=many)
    assert np.array_equal(ctx.get_state(1, 8), want)                                                         # nlist = B equals the unlisted call


def test_listed_refusals(listed):
    """null pointers, nlist outside [0, B], an index outside [0, B) and an index given twice are refused: the state stays as it was, and the context goes on working"""
    HT_ERR_ARG = 1      # include/ht_mi355x.h
    ctx, mix, want = listed
    an, start = _start_state(ctx, mix)
    other = an + np.float32(0.25)                                                                # the analysis of the refused calls: never the one the frames are solved with
    ip = C.POINTER(C.c_int)

    def call(analysis, frames, nlist, B=8):
        fr = None if frames is None else np.ascontiguousarray(frames, np.int32)
        return ctx.L.ht_stage_scratch_unibody_listed(ctx.h, None if analysis is None else analysis.ctypes.data_as(C.POINTER(C.c_float)), B, 3,
                                                     None if fr is None else fr.ctypes.data_as(ip), nlist, 0)
    cases = {"no analysis": (None, [0, 1], 2), "no list": (other, None, 2), "nlist < 0": (other, [0, 1], -1), "nlist > B": (other, list(range(8)) + [0], 9),
             "index < 0": (other, [3, -1], 2), "index = B": (other, [3, 8], 2), "index twice": (other, [3, 5, 3], 3)}
    for what, (analysis, frames, nlist) in cases.items():
        assert call(analysis, frames, nlist) == HT_ERR_ARG, what
        assert np.array_equal(ctx.get_state(1, 8), start), what
    assert call(other, [0], 1, B=0) == HT_ERR_ARG and call(other, [0], 1, B=17) == HT_ERR_ARG      # the batch itself
    ctx.stage_scratch_unibody_listed(an, 8, 3, [4, 0, 6], many_frames=False)
    got = ctx.get_state(1, 8)
    for j in range(8):
        assert np.array_equal(got[j], want[j] if j in (4, 0, 6) else start[j]), _where(mix[j])
