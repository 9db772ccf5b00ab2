"""GPU parity of the solver path against the golden vectors the reference produced (tests/golden/golden8.htfx) and against
the CPU oracle, stage by stage through the C-ABI.  Needs an MI355X: pytest -m gpu.

Tolerances.  Everything up to and including the constraint rows (prepare, FitError, cloud rows, contacts) evaluates the reference's IEEE fp32
operation sequence and is compared bit for bit.  The solver applies those rows in the reference's order but in Jacobian form with fused
multiply-adds (csrc/ht_quad.hpp), i.e. in another association order: poses after a fit step are required to agree to POS_TOL metres / QUAT_TOL
(observed: <= 2e-7 m / 6e-6; the reference's own IEEE and FMA-contracted builds differ by more, tests/golden/ref_flag_spread.py).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle_lib as ol

NF = 8
POS_TOL = 2e-5      # metres (hand is ~0.2 m; fp32 ulp at 0.5 m is 6e-8)
QUAT_TOL = 2e-4
MOM_TOL = 2e-4


@pytest.fixture(scope="module")
def ctx(weights):
    from hand_tracking_samples_amd import native
    c = native.Context(ol.MODEL, 64)
    c.load_weights(weights)
    c.set_params(microforce=3.0, mainthreadpasses=3)      # synthetic-tracker.cpp:91-93
    yield c
    c.close()


def _inputs(golden):
    depth = np.stack([golden["f%d/depth" % f].reshape(-1) for f in range(NF)])
    cams = np.stack([golden["f%d/cam" % f] for f in range(NF)])
    start = np.stack([golden["f%d/startpose" % f] for f in range(NF)])
    return depth, cams, start


def _analysis(golden):
    an = np.zeros((NF, 84), np.float32)
    for f in range(NF):
        pre = "f%d/" % f
        an[f, 0:32] = golden[pre + "an_crays"].reshape(-1)
        an[f, 32:48] = golden[pre + "an_image_points"].reshape(-1)
        an[f, 48:56] = golden[pre + "an_confidence"]
        an[f, 56:72] = golden[pre + "an_vals"]
        an[f, 72:79] = golden[pre + "an_angles"]
        an[f, 79:84] = golden[pre + "an_clenched"]
    return an


def _check_state(got, ref, what):
    dp = np.abs(got[:, 0:3] - ref[:, 0:3]).max()
    dq = np.abs(got[:, 3:7] - ref[:, 3:7]).max()
    dm = np.abs(got[:, 7:13] - ref[:, 7:13]).max()
    print("%s: |dpos| %.2e |dquat| %.2e |dmom| %.2e" % (what, dp, dq, dm))
    assert dp <= POS_TOL and dq <= QUAT_TOL and dm <= MOM_TOL, what
    return dp, dq


def test_fit_error_bit_exact(ctx, golden):
    depth, cams, start = _inputs(golden)
    ctx.stage_prepare(depth, cams)
    ctx.tracker_reset(start)
    err = ctx.stage_fit_error(0, NF)
    ref = np.array([golden["f%d/fiterror_start" % f][0] for f in range(NF)], np.float32)
    assert np.array_equal(err, ref)


def test_cloud_rows_bit_exact(ctx, golden):
    depth, cams, start = _inputs(golden)
    ctx.stage_prepare(depth, cams)
    ctx.tracker_reset(start)
    rows, n = ctx.stage_cloud_rows(0, 4, True, NF)
    for f in range(NF):
        ref = golden["f%d/cloud_rows_sub" % f]
        assert n[f] == len(ref)
        assert np.array_equal(rows[f, :n[f]], ref), "frame %d" % f
    rows, n = ctx.stage_cloud_rows(0, 1, True, NF)
    for f in range(2):
        ref = golden["f%d/cloud_rows_vpts" % f]
        assert n[f] == len(ref)
        assert np.array_equal(rows[f, :n[f]], ref), "frame %d" % f


def test_chamber_rows_bit_exact(ctx, golden):
    """cloud_chamber (physmodel.h:486-496): the five silhouette planes and one ConstrainUnderPlane row per (plane, body), against the rows the reference
    built for the start pose and the full cloud of each golden frame.  min_point_num = 0 switches the rows on for every frame (the reference dumped them
    for every frame); the gate itself (handtrack.h:774) is checked on the frames' real point counts."""
    depth, cams, start = _inputs(golden)
    ctx.stage_prepare(depth, cams)
    ctx.tracker_reset(start)
    ctx.set_params(min_point_num=0)
    try:
        rows, n = ctx.stage_chamber(0, NF)
    finally:
        ctx.set_params(min_point_num=400)
    for f in range(NF):
        ref = golden["f%d/chamber_rows" % f]
        assert n[f] == len(ref) == 85
        assert np.array_equal(rows[f, :n[f]], ref), "frame %d" % f
    rows, n = ctx.stage_chamber(0, NF)
    npts = [len(golden["f%d/vpts" % f]) for f in range(NF)]
    assert list(n) == [85 if p > 400 else 0 for p in npts] and 0 < sum(p > 400 for p in npts) < NF


def test_contacts_bit_exact(ctx, golden):
    depth, cams, start = _inputs(golden)
    ctx.tracker_reset(start)
    c, n = ctx.stage_contacts(0, NF)
    total = 0
    for f in range(NF):
        ref = golden["f%d/contacts_start" % f]
        assert n[f] == len(ref), "frame %d: %d contacts vs %d" % (f, n[f], len(ref))
        assert np.array_equal(c[f, :n[f]], ref[:, :12]), "frame %d" % f
        total += n[f]
    assert total >= 40      # the fist frames really produce contacts


def test_gjk_epa_cases(ctx, golden):
    """Hand-made pairs incl. penetrating ones (EPA): only pairs the model does not ignore can be observed through
    FindShapeShapeContacts; the others are covered by the oracle test."""
    cin, cout = golden["gjk_cases_in"], golden["gjk_cases_out"]
    rest = ctx.get_state(0, 1)[0]
    import htfx
    ign = htfx.load(ol.MODEL)["ignore"]
    checked = pen = 0
    states, expect = [], []
    for i in range(len(cin)):
        a, b = int(cin[i, 0]), int(cin[i, 1])
        lo, hi = min(a, b), max(a, b)
        if ign[lo, hi] or int(cout[i, 10]) < 1:
            continue
        s = np.zeros((17, 13), np.float32)
        s[:, 6] = 1.0
        s[:, 0] = 10.0 * (1 + np.arange(17))          # everything else far away
        s[a, :7] = cin[i, 2:9]
        s[b, :7] = cin[i, 9:16]
        states.append(s)
        expect.append((i, a, b))
    assert len(states) >= 6
    ctx.set_state(0, np.stack(states))
    c, n = ctx.stage_contacts(0, len(states))
    for k, (i, a, b) in enumerate(expect):
        assert n[k] == int(cout[i, 10])
        got = c[k, 0]
        # the reference evaluates Separated(A=a, B=b); FindShapeShapeContacts orders the pair by index
        if a < b:
            ref = np.concatenate([[a, b], cout[i, 0:3], cout[i, 11:17], [cout[i, 17]]]).astype(np.float32)
            assert np.array_equal(got, ref), "case %d" % i
            checked += 1
            pen += cout[i, 9] <= 0
    print("gjk cases checked through the ABI: %d (penetrating: %d)" % (checked, pen))
    assert checked >= 3 and pen >= 3      # the expanding-polytope path is really exercised through the ABI


def test_fit_two_passes(ctx, golden):
    depth, cams, start = _inputs(golden)
    ctx.stage_prepare(depth, cams)
    ctx.tracker_reset(start)
    ctx.set_params(boundary_planes=0)
    try:
        for p in range(2):
            ctx.stage_fit(NF)
            got = ctx.get_state(0, NF)
            for f in range(NF):
                _check_state(got[f], golden["f%d/fit_pass%d" % (f, p)], "fit pass %d frame %d" % (p, f))
    finally:
        ctx.set_params(boundary_planes=1)


@pytest.mark.parametrize("steps", [1, 2, 3, 5])
def test_multistep(ctx, golden, steps):
    depth, cams, start = _inputs(golden)
    ctx.stage_prepare(depth, cams)
    ctx.tracker_reset(start)
    ctx.set_params(steps=steps)
    try:
        ctx.stage_multistep(_analysis(golden), NF)
        got = ctx.get_state(1, NF)
        for f in range(NF):
            _check_state(got[f], golden["f%d/multistep%d" % (f, steps)], "multistep%d frame %d" % (steps, f))
    finally:
        ctx.set_params(steps=5)


def test_reset_path(ctx, golden):
    """PoseFromScratch and 0 to 3 rounds of UnibodyFit on the first three golden tiles: 1685, 944 and 1368 points, so 422, 236 and 342 rows per single-body solve -- all
    three on k_reset's sixteen-rows-at-a-time organisation (up to 448 rows), none on a multiple of sixteen, through the unlisted launch (k_reset<2>).  The row-by-row
    organisations (449 to 896 rows from LDS, more from HBM), the seams between the three and the listed launch are held by tests/test_gpu_reset_fuzz.py."""
    depth, cams, start = _inputs(golden)
    an = _analysis(golden)
    for k in range(4):
        ctx.stage_prepare(depth, cams)
        ctx.tracker_reset(start)
        ctx.stage_scratch_unibody(an, NF, k)
        got = ctx.get_state(1, NF)
        for f in range(3):
            ref = golden["f%d/%s" % (f, "scratch" if k == 0 else "unibody%d" % (k - 1))]
            _check_state(got[f], ref, "reset path k=%d frame %d" % (k, f))


# Whole-path tolerance: the CNN runs on MFMA (fused multiply-add, max |d cnn_out| ~2e-6), and when the tracker accepts the
# CNN-driven pose (after PoseFromScratch or MultiStepSim: five steps driven with force 10000) that difference is amplified.
# The reference itself moves by 3.5e-5 m / 4.5e-4 (quat) on that path between an FMA and a non-FMA build.
FULL_POS_TOL, FULL_QUAT_TOL = 2e-4, 2e-3


def test_unit_of_work_two_frames(ctx, golden):
    """The whole path (GPU CNN included) for two consecutive frames per tracker vs the reference's result."""
    depth, cams, start = _inputs(golden)
    ctx.tracker_reset(start)
    poses, cnn = ctx.update_sync(depth, cams, want_cnn=True)
    ref_cnn = np.stack([golden["f%d/cnn_output" % f] for f in range(NF)])
    assert np.abs(cnn - ref_cnn).max() <= 2e-5
    for f in range(NF):
        ref = golden["f%d/uw_pose_user" % f]
        accepted = golden["f%d/uw_accept" % f][0] > 0
        dp = np.abs(poses[f, :, :3] - ref[:, :3]).max(); dq = np.abs(poses[f, :, 3:] - ref[:, 3:]).max()
        print("unit of work frame %d (cnn pose %s): |dpos| %.2e |dquat| %.2e" % (f, "accepted" if accepted else "rejected", dp, dq))
        if accepted:
            assert dp <= FULL_POS_TOL and dq <= FULL_QUAT_TOL
        else:
            assert dp <= POS_TOL and dq <= QUAT_TOL      # hand model never saw the CNN: same arithmetic as the reference
    pfe, ini = ctx.tracker_flags(NF)
    for f in range(NF):
        assert ini[f] == int(golden["f%d/uw_final" % f][1])
        assert abs(pfe[f] - golden["f%d/uw_final" % f][0]) <= 1e-4
    # second frame of streaming use, teacher-forced from the reference's state after the first frame (free-running
    # sequences diverge through discrete closest-bone / GJK branch flips, SURVEY section 7 "discrete sensitivity")
    ctx.set_state(0, np.stack([golden["f%d/uw_hand_pass2" % f] for f in range(NF)]))
    ctx.set_tracker_flags([golden["f%d/uw_final" % f][0] for f in range(NF)], [int(golden["f%d/uw_final" % f][1]) for f in range(NF)])
    poses2 = ctx.update_sync(depth, cams)
    pfe, ini = ctx.tracker_flags(NF)
    for f in range(NF):
        ref = golden["f%d/uw2_pose_user" % f]
        dp = np.abs(poses2[f, :, :3] - ref[:, :3]).max(); dq = np.abs(poses2[f, :, 3:] - ref[:, 3:]).max()
        print("second frame %d: |dpos| %.2e |dquat| %.2e" % (f, dp, dq))
        assert dp <= FULL_POS_TOL and dq <= FULL_QUAT_TOL
        assert ini[f] == int(golden["f%d/uw2_final" % f][1])


@pytest.mark.parametrize("kick", [False, True])
def test_update_cnn_model_and_kickstart(ctx, golden, weights, kick):
    """HandTracker::update_cnn_model (handtrack.h:734-741) and kickstart (:743-746) against the C restatement: the CNN job alone.  othermodel starts
    from a pose that is NOT handmodel's, which the full update would overwrite (:757) and these calls must not; no main-thread passes; handmodel
    changes only in kickstart and only where the pose is accepted."""
    depth, cams, start = _inputs(golden)
    other = np.roll(start, 1, axis=0)
    ctx.tracker_reset(start)
    st = ctx.get_state(1, NF); st[:, :, :7] = other; st[:, :, 7:] = 0.0
    ctx.set_state(1, st)
    poses, acc = ctx.update_cnn_model_sync(depth, cams, kickstart=kick)
    hand = ctx.get_state(0, NF)
    pfe, ini = ctx.tracker_flags(NF)
    # The restatement is given the device's own heat-maps (the net accumulates on MFMA tiles: its parity is tests/test_gpu_cnn.py): what is compared here is the tracker's
    # logic and MultiStepSim on the same input.  (With its own net's output instead, golden frame 4 -- next to a discrete decision -- turns the 2.6e-6 of the heat-maps into
    # 2.5e-4 .. 6e-3 on othermodel depending on the solver's association order, where the reference's own FMA builds move that frame by 1.3e-5.)
    cnn_dev = ctx.cnn_results(NF)[1]
    orc = ol.Oracle(weights)
    orc.head.par.microforce = 3.0; orc.head.par.mainthreadpasses = 3
    n_acc = 0
    import parity_rule as pr
    trace = np.zeros((NF, 6, 17, 13), np.float32); an = np.zeros((NF, 84), np.float32)      # the restatement's othermodel before MultiStepSim's first step and after each of the five
    amplified = []
    for f in range(NF):
        orc.reset(start[f])
        so = orc.get_state(1); so[:, :7] = other[f]; orc.set_state(1, so)
        ref = np.zeros((17, 7), np.float32)
        cam = ol.camera(cams[f])
        y = np.ascontiguousarray(cnn_dev[f]); orc.L.ho_set_cnn_override(orc.h, ol.fptr(y))
        orc.L.ho_set_trace(orc.h, ol.fptr(trace[f]))
        n = orc.L.ho_update_cnn_model(orc.h, ol.u16ptr(np.ascontiguousarray(depth[f])), C.byref(cam), ol.fptr(ref))
        orc.L.ho_set_trace(orc.h, None); orc.L.ho_get_analysis(orc.h, ol.fptr(an[f]))
        orc.L.ho_set_cnn_override(orc.h, None)
        assert (n > 0) == bool(acc[f]), "frame %d: accept decision" % f
        ro = orc.get_state(1)
        dp = np.abs(poses[f][:, :3] - ro[:, :3]).max(); dq = np.abs(poses[f][:, 3:] - ro[:, 3:7]).max()
        print("update_cnn_model frame %d (%s): |dpos| %.2e |dquat| %.2e" % (f, "accepted" if acc[f] else "rejected", dp, dq))
        # Five free-running hard-driven steps: a frame that stays inside the bands is done.  One that does not (golden frame 4 from frame 3's pose sits next to a discrete
        # decision: tools/diag_frame4.py, 2.5e-7 after one step, 3.1e-3 after five, in either association order of the solver's sums) is a rounding difference amplified
        # or a defect -- which of the two is decided below, step by step from the restatement's state; free-running it only has to stay inside parity_rule's cap.
        if not (dp <= FULL_POS_TOL and dq <= FULL_QUAT_TOL):
            amplified.append(f)
            assert dp <= pr.CAP[0] and dq <= pr.CAP[1]
        if n:
            assert np.abs(poses[f] - ref).max() <= FULL_POS_TOL * 10      # the returned pose is othermodel.GetPose()
        expect_hand = ro[:, :7] if (kick and acc[f]) else start[f]
        tol = FULL_POS_TOL if (kick and acc[f]) else 0.0
        assert np.abs(hand[f][:, :3] - expect_hand[:, :3]).max() <= tol and np.abs(hand[f][:, 3:7] - expect_hand[:, 3:]).max() <= tol * 10
        assert np.all(hand[f][:, 7:] == 0.0)      # no main-thread pass ran
        e, i, _ = orc.flags()
        assert ini[f] == i and abs(pfe[f] - e) <= 1e-4
        n_acc += int(acc[f])
    orc.close()
    assert 0 < n_acc      # the case really covers accepted poses
    # every MultiStepSim step of every frame ALONE, from the restatement's state before it and the restatement's decode (single-step, teacher-forced)
    assert len(amplified) <= 1, amplified
    for s_ in range(5):
        ctx.set_state(1, trace[:, s_])
        ctx.stage_multistep_range(an, NF, s_, s_ + 1)
        got = ctx.get_state(1, NF)
        dps, dqs = pr.pose_diff(got[:, :, :7], trace[:, s_ + 1, :, :7])
        print("  step %d alone from the restatement's state: |dpos| max %.1e m, |dquat| max %.1e" % (s_, dps.max(), dqs.max()))
        assert dps.max() <= 1e-6 and dqs.max() <= 2e-5


def _scaled_cloud_rows(golden, f, microforce=3.0, weak=0.4):
    """CloudConstraints(vpts) of the start pose as the reference dumped them, with the limits PhysModel::FitPointCloud gives them (physmodel.h:347)"""
    rows = golden["f%d/cloud_rows_vpts" % f].copy()
    k = np.where(rows[:, 1] <= 2, weak, 1.0).astype(np.float32) * np.float32(microforce)
    rows[:, 13] = -1.0 * k; rows[:, 14] = 1.0 * k
    return rows


def test_physics_update_with_the_references_own_rows(ctx, golden):
    """void PhysicsUpdate(rigidbodies, Linears, Angulars, {}) (physics.h:543-587) through the C-ABI: the rows are the ones the REFERENCE built for the first
    FitPointCloud pass of each golden frame (cloud rows of every point, the 48 nailed joint rows, the 66 joint-range rows), handed over as caller-built
    rows; the state must be the reference's state after that pass.  Frames 0 and 1 carry the per-point rows in the fixture."""
    depth, cams, start = _inputs(golden)
    ctx.tracker_reset(start)
    frames = [0, 1]
    lin = [np.concatenate([_scaled_cloud_rows(golden, f), golden["f%d/joint_linears" % f]]) for f in frames]
    ang = [golden["f%d/joint_angulars" % f] for f in frames]
    st = ctx.get_state(0, NF)
    ctx.set_state(0, st[frames])
    ctx.physics_update(0, lin, ang)
    got = ctx.get_state(0, len(frames))
    for k, f in enumerate(frames):
        assert len(golden["f%d/contacts_start" % f]) == 0 or True
        _check_state(got[k], golden["f%d/fit_pass0" % f], "PhysicsUpdate with the reference's rows, frame %d" % f)
    # a row list PhysicsUpdate cannot have come from ConstrainContacts with: a friction row without its master in front of it
    bad = lin[0].copy(); bad[5, 15] = -1.0
    from hand_tracking_samples_amd import native
    with pytest.raises(native.HTError, match="friction row"):
        ctx.physics_update(0, [bad], [ang[0]])


def test_fit_rows_with_caller_rows(ctx, golden, weights):
    """void PhysModel::FitPointCloud(points, linears, angulars, microforce) (physmodel.h:345-356) through the C-ABI.  (1) Without caller rows it is the
    pass HandTracker::update runs with the boundary planes off: the reference's fit_pass0.  (2) With the reference's own boundary-plane rows
    (cloud_chamber, dumped as chamber_rows) as the caller's linear rows and one cone row as the caller's angular row: against the C restatement."""
    depth, cams, start = _inputs(golden)
    clouds = [golden["f%d/vpts" % f] for f in range(NF)]
    ctx.tracker_reset(start)
    ctx.fit_rows(0, clouds, [np.zeros((0, 16), np.float32)] * NF, [np.zeros((0, 8), np.float32)] * NF, microforce=3.0)
    got = ctx.get_state(0, NF)
    for f in range(NF):
        _check_state(got[f], golden["f%d/fit_pass0" % f], "FitPointCloud without caller rows, frame %d" % f)
    lin = [golden["f%d/chamber_rows" % f] for f in range(NF)]
    ang = [golden["f%d/enh_angulars" % f] for f in range(NF)]
    ctx.tracker_reset(start)
    ctx.fit_rows(0, clouds, lin, ang, microforce=3.0)
    got = ctx.get_state(0, NF)
    orc = ol.Oracle(weights)
    orc.head.par.microforce = 3.0
    for f in range(NF):
        orc.reset(start[f])
        m = orc.model(0)
        L = (ol.Linear * max(1, len(lin[f])))(); A = (ol.Angular * 16)()
        for i, r in enumerate(lin[f]):
            L[i].rb0 = int(r[0]); L[i].rb1 = int(r[1]); L[i].position0 = ol.v3(r[2:5]); L[i].position1 = ol.v3(r[5:8]); L[i].normal = ol.v3(r[8:11])
            L[i].targetdist = float(r[11]); L[i].targetspeednobias = float(r[12]); L[i].forcelimit = ol.F2(float(r[13]), float(r[14])); L[i].friction_master = int(r[15])
        n = C.c_int(0); z = ol.F3(0, 0, 0)
        orc.L.ho_enhancements(orc.h, m, A, C.byref(n), 0, z, z, 0)      # brings the joint ranges up to date (no rows of its own in this mode)
        assert n.value == 0
        for i, r in enumerate(ang[f]):
            A[i].rb0 = int(r[0]); A[i].rb1 = int(r[1]); A[i].axis = ol.v3(r[2:5]); A[i].torque = 0.0; A[i].targetspin = float(r[5]); A[i].mintorque = float(r[6]); A[i].maxtorque = float(r[7])
        orc.L.ho_fit_pointcloud(orc.h, m, ol.f3ptr(np.ascontiguousarray(clouds[f])), len(clouds[f]), L, len(lin[f]), A, len(ang[f]), 3.0)
        _check_state(got[f], orc.get_state(0), "FitPointCloud with boundary-plane rows, frame %d" % f)
    orc.close()
    from hand_tracking_samples_amd import native
    two_body = golden["f0/joint_linears"][:3]
    with pytest.raises(native.HTError, match="rb0 == NULL"):
        ctx.fit_rows(0, clouds[:1], [two_body], [np.zeros((0, 8), np.float32)], microforce=3.0)


def test_fit_rows_with_many_angular_runs(ctx, golden, weights):
    """More than 64 angular runs in one solve (the level schedule then works two groups per lane): 50 caller-built angular rows on changing body pairs in
    front of the model's own ~66, through PhysModel::FitPointCloud (physmodel.h:345-356), against the C restatement given the same rows."""
    depth, cams, start = _inputs(golden)
    clouds = [golden["f%d/vpts" % f] for f in range(NF)]
    rng = np.random.default_rng(7)
    ang = []
    for f in range(NF):
        rows = np.zeros((50, 8), np.float32)
        for i in range(50):
            a = int(rng.integers(0, 17)); b = (a + 1 + int(rng.integers(0, 15))) % 17
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            rows[i] = [a, b, ax[0], ax[1], ax[2], rng.uniform(-0.2, 0.2), -0.3, 0.3]
        ang.append(rows)
    lin = [np.zeros((0, 16), np.float32)] * NF
    ctx.tracker_reset(start)
    ctx.fit_rows(0, clouds, lin, ang, microforce=3.0)
    got = ctx.get_state(0, NF)
    orc = ol.Oracle(weights)
    orc.head.par.microforce = 3.0
    for f in range(NF):
        orc.reset(start[f])
        m = orc.model(0)
        A = (ol.Angular * 64)()
        n = C.c_int(0); z = ol.F3(0, 0, 0)
        orc.L.ho_enhancements(orc.h, m, A, C.byref(n), 0, z, z, 0)
        assert n.value == 0
        for i, r in enumerate(ang[f]):
            A[i].rb0 = int(r[0]); A[i].rb1 = int(r[1]); A[i].axis = ol.v3(r[2:5]); A[i].torque = 0.0; A[i].targetspin = float(r[5]); A[i].mintorque = float(r[6]); A[i].maxtorque = float(r[7])
        orc.L.ho_fit_pointcloud(orc.h, m, ol.f3ptr(np.ascontiguousarray(clouds[f])), len(clouds[f]), None, 0, A, len(ang[f]), 3.0)
        _check_state(got[f], orc.get_state(0), "FitPointCloud with 50 caller angular rows, frame %d" % f)
    orc.close()
    assert ctx.capacity_events()[2] == 0      # 116 rows: inside the 126 the kernel keeps


def test_solver_builds_agree_bit_for_bit(ctx, golden):
    """k_solve's builds differ only in which of a frame's arrays (two-body groups, impulse sums, angular records) fit their LDS and which go to the
    frame's scratch slot in HBM.  Build 4 holds nothing in LDS, so every frame takes every HBM path; all builds must return the same bits."""
    depth, cams, start = _inputs(golden)
    res = []
    try:
        for build in (0, 1, 2, 3, 4, 6):      # 6: four angular-row slots per lane (up to 252 rows: what a model with more than 18 joints takes)
            ctx.debug_solver_build(build)
            ctx.tracker_reset(start)
            res.append(ctx.update_sync(depth, cams))
    finally:
        ctx.debug_solver_build(0)
    for k, build in enumerate((1, 2, 3, 4, 6)):
        assert np.array_equal(res[0], res[k + 1]), "build %d" % build
    assert ctx.capacity_events() == (0, 0, 0)


def test_set_params_refuses_what_the_kernels_cannot_run(ctx):
    from hand_tracking_samples_amd import native
    for bad in ({"subsample_fraction": 0}, {"drangey": 0.05}, {"steps": -1}, {"physics_iterations": -2}):
        with pytest.raises(native.HTError, match="ht_set_params"):
            ctx.set_params(**bad)
    assert ctx.params.subsample_fraction == 4 and abs(ctx.params.drangey - 0.7) < 1e-7      # a refused call changes nothing
