"""What runs around the contact kernel of a main-thread pass: the boundary planes' rows are made by extra blocks of the cloud-row launch (k_cloud_rows, plane-row
role) on the pass's only side stream.  None of it may change a bit.  The same frames through FitError and the accept step that follows it, which sit between
MultiStepSim and the first pass (k_fit_error on two blocks per frame was measured and taken out again, profiles/r09_pass_tail.md: these are the checks it had to pass,
kept for whoever tries it again), and on two contexts at once.

Five frames (B = 1, 3 and 5 take the first so many; five is odd: the last frame's blocks have no partner frame):
  0  a golden frame with more than 400 points          boundary planes on, several 128-point chunks
  1  exactly 64 points                                 half a chunk; at or below min_point_num, so no plane rows: the plane-row block writes the count alone
  2  no point at all                                   nothing but the counts
  3  150 points                                        no multiple of 64, two chunks (128 + 22), at or below min_point_num
  4  another golden frame with more than 400 points
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  -- at import time on purpose (tests/test_gpu_comm.py): torch's copy of the runtime finds no device once the library has initialised HIP first

import oracle_lib as ol

pytestmark = pytest.mark.gpu
NB = 17
SHAPES = (1, 3, 5)


def _cloud(L, depth, cam):
    """the reference's cloud of a 64x64 frame as the tracker takes it (handtrack.h:703: every 4th in-range pixel)"""
    pts = np.zeros((4096, 3), np.float32); nfull = C.c_int(0)
    n = L.ho_pointcloud(ol.u16ptr(depth), C.byref(cam), 0.1, 0.7, 4, ol.f3ptr(pts), 4096, C.byref(nfull))
    return np.ascontiguousarray(pts[:n])


def _cut_to(L, depth, cam, target):
    """`depth` with only its first pixels (raster order) kept, as many as give a cloud of exactly `target` points"""
    nz = np.flatnonzero(depth)
    lo, hi = 0, len(nz)      # the cloud's size does not shrink with the number of pixels kept
    while lo < hi:
        mid = (lo + hi) // 2
        d = np.zeros_like(depth); d[nz[:mid]] = depth[nz[:mid]]
        if len(_cloud(L, d, cam)) < target:
            lo = mid + 1
        else:
            hi = mid
    d = np.zeros_like(depth); d[nz[:lo]] = depth[nz[:lo]]
    assert len(_cloud(L, d, cam)) == target
    return d


@pytest.fixture(scope="module")
def batch(golden):
    """the five frames, and what the reference makes of them at their start poses: clouds, FitError, cloud rows from the camera's origin, boundary-plane rows"""
    L = ol.lib()
    big = [f for f in range(8) if len(golden["f%d/vpts" % f]) > 400]
    assert len(big) >= 2
    src = [big[0], big[0], big[1], big[1], big[1]]
    cut = [None, 64, 0, 150, None]
    depth = []; cams = []; start = []
    for f, k in zip(src, cut):
        d = np.ascontiguousarray(golden["f%d/depth" % f].reshape(-1)); cam12 = golden["f%d/cam" % f]
        depth.append(d if k is None else np.zeros_like(d) if k == 0 else _cut_to(L, d, ol.camera(cam12), k))
        cams.append(cam12); start.append(golden["f%d/startpose" % f])
    depth = np.stack(depth); cams = np.stack(cams).astype(np.float32); start = np.stack(start).astype(np.float32)
    orc = ol.Oracle(None)
    ref = {"pts": [], "err": [], "cloud": [], "chamber": []}
    try:
        for i in range(5):
            cam = ol.camera(cams[i]); pts = _cloud(L, depth[i], cam); n = len(pts)
            orc.reset(start[i]); m = orc.model(0)
            ref["pts"].append(pts)
            ref["err"].append(np.float32(L.ho_fit_error(orc.h, m, ol.f3ptr(pts if n else np.zeros((1, 3), np.float32)), n, ol.u16ptr(depth[i]), C.byref(cam))))
            rows = (ol.Linear * max(n, 1))(); origin = ol.v3(cams[i][5:8])
            for k, v in enumerate(pts):
                rows[k] = L.ho_cloud_constraint(m, ol.v3(v), origin)
            ref["cloud"].append(ol.linears_to_array(rows, n))
            lin = (ol.Linear * (5 * NB))()
            nl = L.ho_cloud_chamber(m, ol.f3ptr(pts), n, lin, 10.0) if n > 400 else 0      # handtrack.h:774: only a frame with more than min_point_num points has them
            ref["chamber"].append(ol.linears_to_array(lin, nl))
    finally:
        orc.close()
    assert [len(p) for p in ref["pts"]][1:4] == [64, 0, 150] and len(ref["pts"][0]) > 400 and len(ref["pts"][4]) > 400
    assert len(ref["pts"][0]) % 64 and len(ref["pts"][4]) % 64
    return {"depth": depth, "cams": cams, "start": start, "ref": ref}


@pytest.fixture(scope="module")
def ctx(weights):
    from hand_tracking_samples_amd import native
    c = native.Context(ol.MODEL, 8)
    c.load_weights(weights)
    c.set_params(microforce=3.0, mainthreadpasses=1)
    yield c
    c.close()


def test_fused_launch_equals_the_stand_alone_kernels(ctx, batch):
    """One main pass with its plane rows inside the cloud-row launch (an update with one pass; ht_stage_fit, a pass outside an update, keeps k_chamber but shares the
    one side stream) against the same pass on the serial route of the phase profile, which takes the stand-alone k_chamber: equal bit for bit.  And the rows themselves,
    from the stage calls, equal the reference's on every frame."""
    depth, cams, start, ref = batch["depth"], batch["cams"], batch["start"], batch["ref"]
    for B in SHAPES:
        got = {}
        for serial in (0, 2):
            ctx.profile_enable(serial)
            try:
                ctx.tracker_reset(start[:B])
                poses = ctx.update_sync(depth[:B], cams[:B])
                hand = ctx.get_state(0, B)
                ctx.tracker_reset(start[:B]); ctx.stage_prepare(depth[:B], cams[:B])
                ctx.stage_fit(B)
                got[serial] = (poses, hand, ctx.get_state(0, B))
            finally:
                ctx.profile_enable(0)
        for a, b, what in zip(got[0], got[2], ("user poses of an update with one pass", "handmodel after it", "handmodel after ht_stage_fit")):
            assert np.isfinite(a).all() and np.array_equal(a, b), "B = %d: %s" % (B, what)
        assert ctx.capacity_events() == (0, 0, 0)
    ctx.tracker_reset(start); _, _, n = ctx.stage_prepare(depth, cams)
    assert n.tolist() == [len(p) for p in ref["pts"]]
    rows, nch = ctx.stage_chamber(0, 5)
    for i in range(5):
        assert nch[i] == len(ref["chamber"][i]) == (5 * NB if n[i] > 400 else 0)
        assert np.array_equal(rows[i, :nch[i]], ref["chamber"][i]), "boundary-plane rows, frame %d" % i
        assert not rows[i, nch[i]:].any(), "frame %d: rows written beyond the count" % i
    rows, nr = ctx.stage_cloud_rows(0, 1, True, 5)
    for i in range(5):
        assert nr[i] == n[i]
        assert np.array_equal(rows[i, :nr[i]], ref["cloud"][i]), "cloud rows, frame %d" % i


def test_fit_error_equals_the_reference(ctx, batch):
    """ht_stage_fit_error bit for bit against the reference's FitError on the five frames; twice in a row, then smaller batches and the frames in another order after
    the larger one (nothing of a launch may reach the next)."""
    depth, cams, start, ref = batch["depth"], batch["cams"], batch["start"], batch["ref"]
    want = np.array(ref["err"], np.float32)
    ctx.tracker_reset(start); ctx.stage_prepare(depth, cams)
    for run in range(2):
        err = ctx.stage_fit_error(0, 5)
        print("FitError, run %d: %s, reference %s" % (run, err.tolist(), want.tolist()))
        assert np.array_equal(err, want), "run %d" % run
    for order in ([4, 3, 2], [0], [3, 0, 4, 1, 2], [1, 2, 3]):
        ctx.tracker_reset(start[order]); ctx.stage_prepare(depth[order], cams[order])
        err = ctx.stage_fit_error(0, len(order))
        assert np.array_equal(err, want[order]), order
    assert np.array_equal(ctx.stage_fit_error(1, 3), want[[1, 2, 3]])      # othermodel holds the same poses after a tracker reset


@pytest.mark.parametrize("take", [0, 1], ids=["decides", "always_take_cnn"])
def test_accept_decision_on_the_edge_frames(batch, weights, take):
    """A whole update of the five frames with the exact-order sweeps under the product's launch sequence (ht_debug_solver_build 8): user poses, both models' states and the
    tracker flags equal the restatement's ho_update given the device's CNN output, as tests/test_gpu_exact_solver.py compares; the accept decision itself (accepted) from
    a kickstart call on the same frames equals ho_update_cnn_model's."""
    from hand_tracking_samples_amd import native
    depth, cams, start = batch["depth"], batch["cams"], batch["start"]
    c = native.Context(ol.MODEL, 5)
    try:
        c.load_weights(weights)
        c.set_params(microforce=3.0, mainthreadpasses=3, always_take_cnn=take)
        c.debug_solver_build(8)
        c.tracker_reset(start)
        dev = []
        for u in range(2):      # the second update carries prev_frame_error and `initializing`
            p, y = c.update_sync(depth, cams, want_cnn=True)
            dev.append((p, y, c.get_state(1, 5), c.get_state(0, 5), np.stack(c.tracker_flags(5), 1).astype(np.float32)))
        c.tracker_reset(start)
        kposes, acc = c.update_cnn_model_sync(depth, cams, kickstart=True)
        ky = c.cnn_results(5)[1]; khand = c.get_state(0, 5)
        assert c.capacity_events() == (0, 0, 0)
    finally:
        c.debug_solver_build(0)
        c.close()
    orc = ol.Oracle(weights)
    orc.head.par.microforce = 3.0; orc.head.par.mainthreadpasses = 3; orc.head.par.always_take_cnn = take
    orc.L.ho_set_round_once(1)
    try:
        for i in range(5):
            cam = ol.camera(cams[i]); d = ol.u16ptr(np.ascontiguousarray(depth[i]))
            orc.reset(start[i])
            for u in range(2):
                orc.L.ho_set_cnn_override(orc.h, ol.fptr(np.ascontiguousarray(dev[u][1][i])))
                user = np.zeros((NB, 7), np.float32)
                orc.L.ho_update(orc.h, d, C.byref(cam), ol.fptr(user))
                assert np.array_equal(dev[u][0][i], user), "frame %d update %d: user poses" % (i, u)
                assert np.array_equal(dev[u][2][i], orc.get_state(1)), "frame %d update %d: othermodel" % (i, u)
                assert np.array_equal(dev[u][3][i], orc.get_state(0)), "frame %d update %d: handmodel" % (i, u)
                assert np.array_equal(dev[u][4][i], np.array(orc.flags()[:2], np.float32)), "frame %d update %d: tracker flags" % (i, u)
            orc.reset(start[i])
            orc.L.ho_set_cnn_override(orc.h, ol.fptr(np.ascontiguousarray(ky[i])))
            pose = np.zeros((NB, 7), np.float32)
            n = orc.L.ho_update_cnn_model(orc.h, d, C.byref(cam), ol.fptr(pose))
            assert (n > 0) == bool(acc[i]), "frame %d: accepted" % i
            if n:      # kickstart (handtrack.h:743-746): handmodel takes the accepted pose, othermodel's
                other = orc.get_state(1)[:, :7]
                assert np.array_equal(kposes[i], other) and np.array_equal(khand[i][:, :7], other), "frame %d: kickstart" % i
            else:
                assert np.array_equal(khand[i][:, :7], start[i]), "frame %d: handmodel moved without an accepted pose" % i
        orc.L.ho_set_cnn_override(orc.h, None)
    finally:
        orc.L.ho_set_round_once(0)
        orc.close()
    print("always_take_cnn %d: accepted %s" % (take, acc.tolist()))
    if take:
        assert acc.all()


def test_two_contexts_on_two_streams_at_once(batch, weights):
    """The same five frames on two contexts, each on a stream of its own, enqueued alternately (the benchmark's two-in-flight leg): both give the single context's
    poses and states: everything a pass and the accept step keep between kernels belongs to the context."""
    from hand_tracking_samples_amd import native
    dev = torch.device("cuda:0")
    d_depth = torch.from_numpy(batch["depth"].view(np.int16)).to(dev); d_cams = torch.from_numpy(batch["cams"]).to(dev); d_start = torch.from_numpy(batch["start"]).to(dev)
    cs = [native.Context(ol.MODEL, 5) for _ in range(3)]
    try:
        for c in cs:
            c.load_weights(weights); c.set_params(microforce=3.0, mainthreadpasses=3)
        streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
        out = [torch.zeros((5, NB, 7), dtype=torch.float32, device=dev) for _ in range(3)]
        for _ in range(3):      # alone
            cs[2].update_dev(d_depth.data_ptr(), d_cams.data_ptr(), d_start.data_ptr(), 5, out[2].data_ptr(), streams[2].cuda_stream)
        torch.cuda.synchronize()
        for _ in range(3):      # two at once
            for k in range(2):
                cs[k].update_dev(d_depth.data_ptr(), d_cams.data_ptr(), d_start.data_ptr(), 5, out[k].data_ptr(), streams[k].cuda_stream)
        torch.cuda.synchronize()
        alone = (out[2].cpu().numpy(), cs[2].get_state(0, 5), cs[2].get_state(1, 5), np.stack(cs[2].tracker_flags(5), 1))
        assert np.isfinite(alone[0]).all()
        for k in range(2):
            got = (out[k].cpu().numpy(), cs[k].get_state(0, 5), cs[k].get_state(1, 5), np.stack(cs[k].tracker_flags(5), 1))
            for a, b, what in zip(got, alone, ("user poses", "handmodel", "othermodel", "tracker flags")):
                assert np.array_equal(a, b), "context %d: %s" % (k, what)
    finally:
        for c in cs:
            c.close()
