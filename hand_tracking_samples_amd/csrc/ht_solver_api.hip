// ht_solver_api.hip -- tracker / solver entry points of the C-ABI: launch sequencing of the per-frame path
// (HandTracker::update / update_cnn_model / MultiStepSim / FitPointCloud, include/handtrack.h:642-785).
#include <string.h>
#include <stdlib.h>
#include "ht_device.hpp"
#include "ht_host.hpp"
#include "ht_launch.hpp"

#define CHECK_RANGE(ctx, first, n) do { if ((first) < 0 || (n) < 1 || (first) + (n) > (ctx)->B) { (ctx)->err = "slot range exceeds the capacity given to ht_create"; return HT_ERR_ARG; } } while (0)

static int scratch_stride(const ht_ctx *ctx) { return (int)ht_scratch_rows((size_t)ctx->model.pts_cap, (size_t)ctx->model.nb); }

// ---- building blocks ------------------------------------------------------------------------------------------------
static int dev_alloc_points(ht_ctx *ctx)      // the second cloud of a context that uses voxel sub-sampling
{
	const int r = dev_alloc(ctx, &ctx->d_ptsv, (size_t)ctx->B * ctx->model.pts_cap);
	return r || ctx->d_nptsv ? r : dev_alloc(ctx, &ctx->d_nptsv, (size_t)ctx->B);
}
static const cloud_take step_take = { /* stride */ 4, /* cam_origin */ 1, CLOUD_MULTISTEP };      // MultiStepSim: every 4th point, rays from the camera (handtrack.h:656, 681)
static cloud_take fit_take(int mode) { const cloud_take t = { /* stride */ 1, /* cam_origin */ 0, mode }; return t; }      // FitPointCloud's callers: every point, rays from the origin
static cloud_records cloud_rec(ht_ctx *ctx) { cloud_records r = { ctx->d_scratch, scratch_stride(ctx), ctx->d_rowbody, ctx->phys.deltaT }; return r; }
static const cloud_records *rec_or_rows(const ht_ctx *ctx, const cloud_records *cr) { return exact_solver(ctx) ? nullptr : cr; }
static void exact_args(ht_ctx *ctx, solve_args &a, bool cloud)
{
	a.force_build = exact_solver(ctx) ? 5 : ctx->solver_build;
	a.exact_lin = ctx->d_exact_lin; a.exact_ang = ctx->d_exact_ang;
	if (exact_solver(ctx) && cloud) { a.rows_cloud = ctx->d_rows; a.cloud_body = nullptr; }
}
// What every solve starts from: model `which` of the frames' slots, their scratch, the net's decoded output, the cameras, the capacity counters, the contact pool (if it takes contacts)
static solve_args solve_head(ht_ctx *ctx, int which, bool contacts)
{
	solve_args a; memset(&a, 0, sizeof a); a.sf_select = -1; a.caps = reinterpret_cast<int *>(ctx->d_epa_ws) + 2;
	a.contacts = contacts ? ctx->d_contacts : nullptr; a.ncontacts = ctx->d_ncontacts;
	a.analysis = ctx->d_analysis; a.cams = ctx->d_cams; a.state = ctx->d_state[which]; a.scratch = ctx->d_scratch; a.scratch_stride = scratch_stride(ctx); a.batch = ctx->B;
	return a;
}
// The row mix of a solve besides its contacts: MultiStepSim's step st (handtrack.h:660-688: CNN-driven angular rows, landmark rays, cloud rows, the palm drive) or a
// main-thread pass (:769-780: the boundary planes' rows and the cloud rows)
struct step_mix { bool angles, rays, cloud, chamber; float palm_drive; int arm_cone, zero_momenta; };
static step_mix mix_of_step(const ht_params &p, int st)
{
	const bool angles = (st < p.steps_keyangles) || p.angles_only, rays = (st < p.steps_keypoints) && !p.angles_only, cloud = (st >= p.steps_cloudstart) && !p.angles_only;
	step_mix m = { angles, rays, cloud, false, st < p.steps_palmangle ? 10000.0f : 0.0f, 1, 1 };
	return m;
}
static step_mix mix_of_pass() { step_mix m = { false, false, true, true, 0.0f, 0, 0 }; return m; }
static int step_slot(int st) { return st < 8 ? st : -1; }      // the launches of an update that keep a history, a contact launch its work and a solve its cost (HT_CONTACT_SLOTS): MultiStepSim step st -> st,
static int pass_slot(int pass) { return pass >= 0 && pass < 8 ? 8 + pass : -1; }      // main-thread pass i -> 8 + i; -1: none
// Batches that take several rounds per CU launch their block-per-frame kernels longest frame first, so that a launch ends on short frames instead of waiting for a long one
// that started last (results do not depend on the order): the cloud-row and FitError kernels by the frames' point counts (update_inputs), the solves by what every frame took
// in the same launch of the previous update (solve_hist: k_solve notes it, update_orders ranks it beside the net).
static bool several_rounds(const ht_ctx *ctx, int B) { return B > ctx->n_cu * 8; }
struct solve_opts { const int *active = nullptr; int hist_slot = -1; bool tables = false, shared_gpu = false; float *poses_out = nullptr; const int *out_npts = nullptr; bool fork_next = false; };      // active: only the frames whose flag is set; tables: solve_prep has made them for exactly this solve; poses_out: the solve also writes the user poses; fork_next: the stream's next operation is a fork (fork / fork1), so the launch may carry its event (forks_from)
// Tuning builds: a launch that takes a launch table while the tables are still being made on side stream 0 must be on that stream (update_resets)
static void table_read_on(const ht_ctx *ctx, hipStream_t s)
{
#ifdef HT_TUNING
	if (ctx->tables_out && s != ctx->side[0]) { fprintf(stderr, "a launch table read on a stream that has not joined side stream 0\n"); abort(); }
#endif
}
// The edges between an update's streams.  The row-producing kernels of one fit step only read the pose, so they run side by side with the contacts on a side stream and the
// solve waits for them (each is latency-bound on its slowest frame and leaves most of the chip idle).  An edge is an event of the context (ht_host.hpp: ht_edge_event --
// no system-scope fence: the consumer of every edge below is a kernel of this device) that the other stream waits for.  Who completes the event:
//   a hipEventRecord behind the producer                                       fork + join of a 100 us step: 7.9 us over the ideal, 20.4 us when the solve waits for the join
//   the producer's own launch (hipExtLaunchKernelGGL's stopEvent: `done`)      6.5 / 17.7 us: no marker between the solve and the contacts that follow it
// (tools/exp_stream_edges.hip, profiles/r30_stream_edges.md; with the events of rounds 1 to 29 a pair cost 10.0 / 24.5 us).  The launch form is taken where a solve is
// followed by the next step's fork (forks_from) and where the cloud rows are the last launch of their side stream before the join (joins_from), in updates that are not being
// captured into a HIP graph (run_update_: a stopEvent is not known to become a graph dependency) and not under ht_debug_stream_edges(ctx, 1).  The first fork of a loop,
// the forks and joins of the update's head and ev_lap follow other kernels and stay records.
// (side_open keeps track of the side streams that are out: an update ends by bringing back whichever still is, join_open)
#ifndef HT_EDGE_ON_LAUNCH
#define HT_EDGE_ON_LAUNCH 1
#endif
static hipEvent_t forks_from(ht_ctx *ctx, hipStream_t s) { if (!ctx->edges_on_launch) return nullptr; ctx->fork_carried = s; return ctx->ev_fork; }      // for the launch after which stream s forks next: the event it completes
static hipEvent_t joins_from(ht_ctx *ctx, int i) { if (!ctx->edges_on_launch) return nullptr; ctx->join_carried |= 1u << i; return ctx->ev_join[i]; }      // for the last launch of side stream i before its join
static void fork_event(ht_ctx *ctx, hipStream_t s) { if (ctx->fork_carried != s) (void)hipEventRecord(ctx->ev_fork, s); ctx->fork_carried = nullptr; }
static void fork(ht_ctx *ctx, hipStream_t s) { fork_event(ctx, s); for (int i = 0; i < 2; i++) (void)hipStreamWaitEvent(ctx->side[i], ctx->ev_fork, 0); ctx->side_open |= 3u; }
static void fork1(ht_ctx *ctx, hipStream_t s, int i) { fork_event(ctx, s); (void)hipStreamWaitEvent(ctx->side[i], ctx->ev_fork, 0); ctx->side_open |= 1u << i; }
static void join1(ht_ctx *ctx, hipStream_t s, int i)
{
	if (!((ctx->join_carried >> i) & 1u)) (void)hipEventRecord(ctx->ev_join[i], ctx->side[i]);
	(void)hipStreamWaitEvent(s, ctx->ev_join[i], 0); ctx->join_carried &= ~(1u << i); ctx->side_open &= ~(1u << i); if (i == 0) ctx->tables_out = false;
}
static void join(ht_ctx *ctx, hipStream_t s, int n) { for (int i = 0; i < n; i++) join1(ctx, s, i); }
static void join_open(ht_ctx *ctx, hipStream_t s) { for (int i = 0; i < 2; i++) if ((ctx->side_open >> i) & 1u) join1(ctx, s, i); }
static void solve_step(ht_ctx *ctx, int which, const step_mix &m, int B, hipStream_t s, const solve_opts &o)
{
	solve_args a = solve_head(ctx, which, ctx->phys.use_collision != 0);
	a.rows_pre = m.chamber ? ctx->d_chamber : nullptr; a.n_pre = m.chamber ? ctx->d_nchamber : nullptr; a.pre_stride = 5 * ctx->model.nb;
	a.cloud_body = m.cloud ? ctx->d_rowbody : nullptr; a.n_cloud = ctx->d_nrows;      // k_cloud_rows wrote the rows' records into the scratch slots (cloud_rec)
	a.active_flag = o.active; a.apply_angles = m.angles; a.drive_force = m.palm_drive; a.ray_rows = m.rays; a.arm_cone = m.arm_cone; a.zero_momenta = m.zero_momenta;
	a.steps_keyangles = ctx->par.steps_keyangles; a.min_cray_prob = ctx->par.min_cray_prob;
	a.dbg = ht_tuning_flags(); a.shared_gpu = o.shared_gpu ? 1 : 0; a.tables = o.tables ? ctx->d_tables : nullptr;
	exact_args(ctx, a, m.cloud);
	a.out_poses = o.poses_out; a.out_npts = o.out_npts; a.out_initializing = ctx->d_initializing; a.out_min_point_num = ctx->par.min_point_num;
	// (a solve on some of the frames -- o.active -- keeps no cost history and takes no order table: update_resets relies on it, as on launch_contacts' rule for the reset frames)
	if (!o.active && !exact_solver(ctx) && several_rounds(ctx, B)) { const ht_history::rows h = ctx->solve_hist.take(o.hist_slot, B); a.cost_out = h.work; a.frame_order = h.order; }
	if (a.frame_order) table_read_on(ctx, s);
	ht_launch_solve(ctx->model, ctx->phys, a, B, s, o.fork_next ? forks_from(ctx, s) : nullptr);
}
// Round 6: the tables of a solve (ht_solve_shared.hpp) are made by k_solve_prep on whichever stream runs the solve's row producers, behind the cloud rows (it lists them per
// body) and beside the contact kernel; the solve_step that follows is told to start from them.  Off for the exact-order builds (their sweeps take the rows as the reference
// lays them out) and under ht_debug_solve_tables(0).
// 0: off; 1: every table (pose-only and chain tables: one launch behind the cloud rows); 2: the pose-only tables alone, on the side stream the cloud rows do not use
static int solve_tables_mode(const ht_ctx *ctx)
{
	static const int env = ht_tuning_int("HT_TABLES", -1);      // timing experiments (-DHT_TUNING builds only): tools/exp_tables.sh
	const int m = env >= 0 ? env : ctx->solve_tables;
	return (m && ctx->d_tables && !exact_solver(ctx)) ? m : 0;
}
static bool solve_tables_on(const ht_ctx *ctx) { return solve_tables_mode(ctx) == 1; }
static void solve_prep(ht_ctx *ctx, int which, const step_mix &m, bool pose_only, const int *active, int B, hipStream_t s)      // pose_only: the tables that follow from the pose alone (mode 2); otherwise every table, the lists of the mix's cloud and boundary-plane rows among them
{
	prep_args a;
	memset(&a, 0, sizeof a);
	a.state = ctx->d_state[which]; a.analysis = ctx->d_analysis; a.cams = ctx->d_cams; a.active_flag = active;
	a.scratch = ctx->d_scratch; a.scratch_stride = scratch_stride(ctx); a.batch = ctx->B;
	a.cloud_body = m.cloud && !pose_only ? ctx->d_rowbody : nullptr; a.n_cloud = ctx->d_nrows;
	if (m.chamber && !pose_only) { a.ch_planes = ctx->d_chplanes; a.ch_on = ctx->d_chon; a.rows_pre = ctx->d_chamber; a.n_pre = ctx->d_nchamber; a.ch_maxforce = 10.0f; }
	a.apply_angles = m.angles; a.drive_force = m.palm_drive; a.ray_rows = m.rays; a.arm_cone = m.arm_cone;
	a.steps_keyangles = ctx->par.steps_keyangles; a.min_cray_prob = ctx->par.min_cray_prob;
	a.tables = ctx->d_tables; a.dbg = ht_tuning_flags(); a.parts = pose_only ? 1 : 3;
	ht_launch_solve_prep(ctx->model, ctx->phys, a, B, s);
}
// Tuning builds, HT_MARKS=1: events at named points of an update on whichever stream, printed (ms since the first) after the update -- the concurrent streams as
// they really ran (a kernel trace serialises them).
#ifdef HT_TUNING
static std::vector<std::pair<std::string, hipEvent_t>> g_marks;
static bool marks_on() { static const bool on = getenv("HT_MARKS") != nullptr; return on; }
static void mark(const char *name, hipStream_t s) { if (!marks_on()) return; hipEvent_t e; (void)hipEventCreate(&e); (void)hipEventRecord(e, s); g_marks.emplace_back(name, e); }
static void marks_dump()
{
	if (!marks_on() || g_marks.empty()) return;
	(void)hipDeviceSynchronize();
	for (auto &m : g_marks) { float ms = 0; (void)hipEventElapsedTime(&ms, g_marks[0].second, m.second); fprintf(stderr, "  mark %-28s %8.3f ms\n", m.first.c_str(), ms); }
	for (auto &m : g_marks) (void)hipEventDestroy(m.second);
	g_marks.clear();
}
#else
static inline void mark(const char *, hipStream_t) {}
static inline void marks_dump() {}
#endif
// The contact kernel on model `which`, with what varies from launch to launch: the frames (`active`: when given, only those whose flag is set -- the reset frames in their
// few-frames organisation unless many reset), the stream, whether cloud rows run beside it, the history slot (ht_launch.hpp: HT_CONTACT_SLOTS).  A launch on the reset frames
// alone keeps no history and takes the fixed assignment (update_resets relies on it: under resets_lap the tables are still being made on side stream 0 while this stream
// launches the reset frames' contacts).
static void launch_contacts(ht_ctx *ctx, int which, const int *active, int B, hipStream_t s, bool beside_cloud_rows = false, int slot = -1)
{
	const bool reset_frames = active && active == ctx->d_flags;
	const ht_history::rows h = ctx->contact_hist.take(reset_frames ? -1 : slot, B);
	if (h.order) table_read_on(ctx, s);
	ht_launch_contacts(ctx->model, ctx->d_state[which], ctx->phys.driftmax, ctx->phys.jiggle_sin, active, ctx->d_epa_ws, ctx->d_contacts, ctx->d_ncontacts, B, s, beside_cloud_rows, ctx->contact_kernel,
	                   reset_frames && !ctx->many_reset, h.order, h.work);
}
// At the head of an update, on a stream that has nothing to do while the net runs: this update's launch tables from the works of the last one
static void update_orders(ht_ctx *ctx, int B, hipStream_t t)
{
	const coop_plan plan = ht_contacts_coop_plan(ctx->model, B);      // the tables deal the frames over the blocks of the cooperative kernel's whole-batch form
	// frames with polytope runs per block: every block a CU of its own (the slowest block is the launch's time) -> one; several rounds per CU (the sum counts) -> all.
	// tools/exp_contact_epb.sh at 1024 frames, 1 / 2 / 3 / 4 per block: slowest block 329 / 339 / 355 / 369 k cycles, mean frame 2.13 / 2.11 / 2.05 / 2.01 M cycles per step
	static const int epb_env = ht_tuning_int("HT_CONTACT_EPB", 0);      // -DHT_TUNING builds: pins it
	const int blocks = plan.nfr > 0 ? (B + plan.nfr - 1) / plan.nfr : 0, epb = epb_env > 0 ? epb_env : blocks > ctx->n_cu ? plan.nfr : 1;
	ht_history &c = ctx->contact_hist, &v = ctx->solve_hist;
	c.begin(B, plan.nfr > 1 && ht_contacts_coop(ctx->model, B, ctx->contact_kernel, false), [&](unsigned slots) { ht_launch_contact_order(c.work, c.order, B, plan.nfr, c.stride, slots, HT_CONTACT_SLOTS, epb, t); });
	v.begin(B, several_rounds(ctx, B), [&](unsigned slots) { ht_launch_rank_desc(v.work, v.order, B, v.stride, slots, HT_CONTACT_SLOTS, t); });
}
// Which steps of MultiStepSim to run, where and how much of each: multistep(ctx, B, steps_on(stream).steps(0, 1).frames(ctx->d_flags).in_order().rows_only()).
// Unless told otherwise: every step of every frame, whole, bracketed for the profile, the cloud rows of a step on side stream 0 beside its contacts.
struct steps_on
{
	hipStream_t s; int from = 0, to = 1 << 30; const int *active = nullptr; int side = 0; bool prof = true, shared_gpu = false, rows = true, solve = true;
	explicit steps_on(hipStream_t stream) : s(stream) {}
	steps_on &steps(int first, int end = 1 << 30) { from = first; to = end; return *this; }      // [first, end), or from `first` to the last
	steps_on &frames(const int *flags) { active = flags; return *this; }               // only the frames whose flag is set
	steps_on &all_frames() { active = nullptr; return *this; }
	steps_on &rows_beside(int i) { side = i; return *this; }                            // the cloud rows on side stream i, beside the contacts on the steps' stream
	steps_on &in_order() { side = -1; return *this; }                                   // everything in order on the steps' stream
	steps_on &unprofiled() { prof = false; return *this; }                              // a concurrent second instance: not bracketed for the profile
	steps_on &shares_gpu() { shared_gpu = true; return *this; }                         // other kernels run beside the solves (solve_args::shared_gpu)
	steps_on &rows_only() { solve = false; return *this; }                              // only what precedes the solve (cloud rows, contacts)
	steps_on &solve_only() { rows = false; return *this; }
	bool fork_follows = false;
	steps_on &then_forks(bool yes = true) { fork_follows = yes; return *this; }         // the stream's next operation behind the last of these steps is a fork: its solve may carry the event (forks_from)
};
// What step st of MultiStepSim under `o` puts beside its contact kernel: the step's cloud rows, and (round 6) the solve's tables behind them -- a step without cloud rows
// forks for the tables alone.  The answer is whether the step forks at all
struct step_sides { bool par, pose_only, tables; };
static step_sides sides_of_step(ht_ctx *ctx, const steps_on &o, int st)
{
	const bool coll = ctx->phys.use_collision != 0, whole = o.rows && o.solve;
	static const bool no_side = ht_tuning_env("HT_NO_SIDE");      // timing experiments (-DHT_TUNING builds only)
	step_sides r;
	r.pose_only = solve_tables_mode(ctx) == 2 && o.side >= 0 && coll && !ctx->profile_phases && !no_side && whole && !o.active;      // the pose-only tables: on the OTHER side stream, beside the cloud rows
	r.tables = solve_tables_on(ctx) || r.pose_only;
	r.par = o.side >= 0 && (mix_of_step(ctx->par, st).cloud || r.tables) && coll && !ctx->profile_phases && !no_side;
	return r;
}
// HandTracker::MultiStepSim on othermodel (handtrack.h:642-690)
static void multistep(ht_ctx *ctx, int B, const steps_on &o)
{
	const ht_params &p = ctx->par;
	hipStream_t s = o.s; const int *active = o.active; const bool whole = o.rows && o.solve;
	for (int st = o.from; st < p.steps && st < o.to; st++)
	{
		const step_mix m = mix_of_step(p, st); const bool coll = ctx->phys.use_collision != 0;
		const step_sides sd = sides_of_step(ctx, o, st); const bool pose_only = sd.pose_only, tables = sd.tables, par = sd.par;
		if (o.rows)
		{
			hipStream_t rows_stream = par ? ctx->side[o.side] : s;
			if (par && pose_only) fork(ctx, s); else if (par) fork1(ctx, s, o.side);
			const cloud_records cr = cloud_rec(ctx);
			const bool rows_last = par && !tables;      // the cloud rows are the side stream's last launch before the join: the launch carries the join's event
			if (m.cloud) { ht_prof_scope ps(ctx, o.prof ? "cloud_rows" : nullptr, s, true); ht_launch_cloud_rows(ctx->model, ctx->d_state[1], ctx->d_pts, ctx->d_npts, ctx->d_cams, active, step_take, ht_cloud_limits(p, CLOUD_MULTISTEP), ctx->d_rows, ctx->d_nrows, B, rows_stream, rec_or_rows(ctx, &cr), nullptr, rows_last ? joins_from(ctx, o.side) : nullptr); }
			if (pose_only) solve_prep(ctx, 1, m, true, active, B, ctx->side[1 - o.side]);
			else if (tables) { ht_prof_scope ps(ctx, o.prof ? "solve_prep" : nullptr, s, true); solve_prep(ctx, 1, m, false, active, B, rows_stream); }
			if (coll) { ht_prof_scope ps(ctx, o.prof ? "contacts" : nullptr, s, true); launch_contacts(ctx, 1, active, B, s, false, step_slot(st)); }
			if (par && pose_only) join(ctx, s, 2); else if (par) join1(ctx, s, o.side);
			if (whole && !active) mark("  step: rows done", s);
		}
		if (!o.solve) continue;
		ht_prof_scope ps(ctx, o.prof ? "solve" : nullptr, s);
		solve_opts so; so.active = active; so.hist_slot = step_slot(st); so.tables = tables; so.shared_gpu = o.shared_gpu;
		const bool more = st + 1 < p.steps && st + 1 < o.to;      // behind this solve: the next step's fork, or what the caller says follows the last step
		so.fork_next = more ? o.rows && sides_of_step(ctx, o, st + 1).par : o.fork_follows;
		solve_step(ctx, 1, m, B, s, so);
	}
}
// one main-thread pass of HandTracker::update (handtrack.h:769-780).  Its row producers run beside the contact kernel on ONE side stream: a cross-stream edge costs about
// 10 us and the solve waited for the later of two joins; inside an update the boundary planes' rows are extra blocks of the cloud-row launch (k_cloud_rows: plane_rows), which
// fill that launch's tail instead of competing with it for the CUs the contact kernel frees.
static void main_pass(ht_ctx *ctx, int B, hipStream_t s, float *poses_out = nullptr, int pass = -1, bool pass_follows = false)      // poses_out: the update's last pass also writes the user poses; pass_follows: the stream's next operation is another pass of the same update
{
	const ht_params &p = ctx->par;
	const float4 *pts = p.subsample_voxel ? ctx->d_ptsv : ctx->d_pts;      // handtrack.h:751: the main-thread cloud
	const int *npts = p.subsample_voxel ? ctx->d_nptsv : ctx->d_npts;
	const step_mix m = mix_of_pass(); const bool coll = ctx->phys.use_collision != 0;
	static const bool no_side = ht_tuning_env("HT_NO_SIDE");
	const bool par = !ctx->profile_phases && !no_side;
	const bool pose_only = solve_tables_mode(ctx) == 2 && par;
	const bool tables = solve_tables_on(ctx);
	const bool fused = par && !tables && !pose_only && ctx->planes_valid;      // the plane rows ride in the cloud-row launch; otherwise k_chamber makes them (the serial route of the profile, a pass outside an update)
	hipStream_t rows_stream = par ? ctx->side[0] : s, chamber_stream = pose_only ? ctx->side[1] : rows_stream;      // side stream 1 is a pass's only with the pose-only tables
	// Round 6: the five boundary planes follow from the points alone, so an update makes them once (beside the net: update_planes) and every pass only their rows (k_chamber,
	// or k_solve_prep with the solve tables).  A pass outside an update (ht_stage_fit) makes them here.
	if (!ctx->planes_valid) { ht_prof_scope ps(ctx, "chamber", s, true); ht_launch_chamber_planes(ctx->model, pts, npts, p.min_point_num, p.boundary_planes, ctx->d_chplanes, ctx->d_chon, B, s); }
	if (par) { if (pose_only) fork(ctx, s); else fork1(ctx, s, 0); }
	if (pose_only) solve_prep(ctx, 0, m, true, nullptr, B, ctx->side[1]);      // the pose-only tables ahead of the boundary planes on their side stream: both beside the cloud rows
	if (!tables && !fused) { ht_prof_scope ps(ctx, "chamber", s, true); ht_launch_chamber(ctx->model, ctx->d_state[0], ctx->d_chplanes, ctx->d_chon, 10.0f, ctx->d_chamber, ctx->d_nchamber, B, chamber_stream); }
	const cloud_records cr = cloud_rec(ctx);
	const plane_rows pr = { ctx->d_chplanes, ctx->d_chon, 10.0f, ctx->d_chamber, ctx->d_nchamber };
	{ ht_prof_scope ps(ctx, "cloud_rows", s, true); ht_launch_cloud_rows(ctx->model, ctx->d_state[0], pts, npts, ctx->d_cams, nullptr, fit_take(CLOUD_FIT), ht_cloud_limits(p, CLOUD_FIT), ctx->d_rows, ctx->d_nrows, B, rows_stream, rec_or_rows(ctx, &cr), fused ? &pr : nullptr,
	                                                                         par && !tables && !pose_only ? joins_from(ctx, 0) : nullptr); }      // side stream 0's last launch before the join carries the join's event
	if (tables) { ht_prof_scope ps(ctx, "solve_prep", s, true); solve_prep(ctx, 0, m, false, nullptr, B, rows_stream); }
	if (coll) { ht_prof_scope ps(ctx, "contacts", s, true); launch_contacts(ctx, 0, nullptr, B, s, par, pass_slot(pass)); }
	mark("  pass: contacts done", s);
	if (par)
	{
		mark(fused ? "  pass: cloud + plane rows done" : "  pass: cloud rows done", ctx->side[0]);
		if (pose_only) { mark("  pass: chamber done", ctx->side[1]); join(ctx, s, 2); } else join1(ctx, s, 0);
	}
	mark("  pass: rows joined", s);
	ht_prof_scope ps(ctx, "solve", s);
	solve_opts so; so.hist_slot = pass_slot(pass); so.tables = tables || pose_only; so.poses_out = poses_out; so.out_npts = npts;
	so.fork_next = pass_follows && par && ctx->planes_valid;      // the next pass starts with its fork (its planes are the update's: no launch ahead of the fork)
	solve_step(ctx, 0, m, B, s, so);
}
// Behind the join of the side stream, so nothing of the step waits for it: the running counts of reset frames go to the host (ht_host.hpp: d_nreset).  The
// update's stream picks the copy up again at its very end (reset_tail_join: long finished by then) -- every stream of an update has to come back to the
// caller's, or the update could not be captured into a HIP graph.  The consumer of that last join is whatever the caller enqueues next; the host reads h_nreset without ever
// waiting, and what makes the two words visible to it is the copy itself (a copy engine or a blit kernel with its own system-scope release), not the event behind it.
// The same holds for a pose output in pinned host memory (zero copy): the update's last solve writes it on the caller's stream, and the caller's own event or
// synchronisation, which the library does not make, releases it to the host.
static void reset_tail(ht_ctx *ctx) { (void)hipMemcpyAsync(const_cast<unsigned *>(ctx->h_nreset), ctx->d_nreset, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->side[0]); ctx->tail_pending = true; }
static void reset_tail_join(ht_ctx *ctx, hipStream_t s) { if (ctx->tail_pending) { join(ctx, s, 1); ctx->tail_pending = false; } }
static void reset_path(ht_ctx *ctx, bool listed, int n_unibody, int B, hipStream_t s, hipStream_t prof_stream, bool many_frames = false)      // listed: the frames of d_flist; otherwise all
{
	ht_prof_scope ps(ctx, "reset_path", prof_stream, true);
	if (listed) ctx->last_reset_many = many_frames ? 1 : 0;
	ht_launch_reset(ctx->model, ctx->phys, ctx->d_state[1], ctx->d_pts, ctx->d_npts, ctx->d_analysis, ctx->d_cams, listed ? ctx->d_flist : nullptr, listed ? ctx->d_nflist : nullptr, n_unibody, ctx->par,
	                ctx->d_rows, ctx->d_nrows, ctx->d_scratch, scratch_stride(ctx), ctx->B, B, s, many_frames, ctx->n_cu, exact_solver(ctx));
}

// ---- the whole unit of work on device buffers --------------------------------------------------------------------------
// What an update call's d_depth / d_cams hold, by name (resolve_frames, below, makes it from an entry point's arguments and is the only place that compares sizes):
//   FRAME_TILE         the reference's 64x64 tile for the 64x64 net; the camera copy and the re-seeding from start poses ride on k_prepare
//   FRAME_OWN_SEGMENT  a side x side frame that is its own segment and feeds the net of that input size -- what HandSegmentVR returns for a frame of the net's size
//                      (handtrack.h:283-284), the stages of :693-729 called directly (BASELINE configs[4] end to end, SURVEY 8d config 5 i-iii); heat-map camera
//                      camsub(cam, side / 16).  Arises for side 128 only (at side 64 it is the tile)
//   FRAME_SEGMENTED    a full-size frame (handtrack.h:693-785 with dim != 64x64): the tracker segments it for the CNN (:697-698) at `side`, the tile side of the net that
//                      looks at it (64: the reference's; 128: the sized calls -- the segment camera of side 128 is that of side 64 with focal doubled and principal
//                      (64,64), its heat-map camera camsub(cam, 8) is camsub(cam64, 4), and the pose is the same pose).  From then on ctx->d_cams holds the SEGMENT
//                      cameras (CNN decode, landmark rays, PoseFromScratch, UnibodyFit and MultiStepSim take segment.cam.pose); the point cloud and FitError keep the
//                      full frame and its camera, whose cloud the point capacity can cut short (d_overflow counts such frames; the host forms report them)
// w x h: the image FitError looks at (a tile's 64 x 64).  `side`: the input side of the net (ht_net_of).  `px64`: the frame has a tile's pixels whatever its kind (a 64x64
// frame at side 128 is segmented like any other): the host forms upload such frames to d_depth / d_cams (stage_frames).
enum frame_kind { FRAME_TILE, FRAME_OWN_SEGMENT, FRAME_SEGMENTED };
struct frame_src { frame_kind kind; int w, h, side; float segment_scale; bool px64; };
// `mode`: UPD_FULL = HandTracker::update (handtrack.h:748-785); UPD_CNN_MODEL = update_cnn_model alone (:734-741): othermodel is NOT re-seeded from
// handmodel, no main-thread passes, no "initializing = 50" rule, the result is othermodel.GetPose() plus the accept decision, handmodel untouched;
// UPD_KICKSTART = kickstart (:743-746) = the same followed by handmodel.SetPose(pose) where the pose was accepted.
// UPD_PASSES = only the caller's part of update() (:751-753, 769-785): the cloud of the frame, the main-thread passes on handmodel, the user poses (the overlapped mode, ht_update_passes_sync)
enum { UPD_FULL = 0, UPD_CNN_MODEL = 1, UPD_KICKSTART = 2, UPD_PASSES = 3 };
struct update_call { const uint16_t *d_depth; const float *d_cams, *d_start; int B; float *d_poses_out, *d_cnn_out; hipStream_t s; frame_src fs; int mode; const float *img_cams; const ht_net *net; };      // one update call: what the caller gave, where FitError finds the image (update_inputs: the full-size frame and its cameras, or the tile), and the net that looks at it (run_update_)
static bool main_thread_cloud_voxel(const ht_ctx *ctx, const update_call &u) { return (u.mode == UPD_FULL || u.mode == UPD_PASSES) && ctx->par.subsample_voxel; }

// Input staging: the point capacity this frame size needs, the segment for the net (full-size frames), the net's input, the cloud(s), the launch order by point counts
static int update_inputs(ht_ctx *ctx, update_call &u)
{
	const ht_params &p = ctx->par;
	const frame_src &fs = u.fs; const uint16_t *d_depth = u.d_depth; const float *d_cams = u.d_cams; const int B = u.B, mode = u.mode; hipStream_t s = u.s;
	const bool tile = fs.kind == FRAME_TILE, own = fs.kind == FRAME_OWN_SEGMENT, segment = fs.kind == FRAME_SEGMENTED && mode != UPD_PASSES;      // (the caller's part of the overlapped update has no segment and no net)
	{ const int npx = fs.w * fs.h, fr = p.subsample_fraction > 0 ? p.subsample_fraction : 1, n = main_thread_cloud_voxel(ctx, u) ? npx : (npx + fr - 1) / fr; if (n > ctx->model.pts_cap) { const int r = ht_reserve_points_locked(ctx, n); if (r) return r; } ctx->model.pts_bound = (n + 63) & ~63; }
	u.img_cams = ctx->d_cams;
	if (!tile)
	{
		int r;      // the three buffers of the full-size path: the two of fixed size by the one this asks for last, the tiles following the largest side seen
		if (!ctx->d_overflow && ((r = dev_alloc(ctx, &ctx->d_frame_cams, (size_t)ctx->B * HT_CAM)) || (r = dev_alloc(ctx, &ctx->d_overflow, 1)))) return r;
		if ((r = dev_grow(ctx, &ctx->d_seg_tiles, &ctx->seg_tiles_cap, (size_t)ctx->B * (own ? 64 * 64 : fs.side * fs.side)))) return r;      // (a frame that is its own segment cuts no tile: the buffer comes with the first frame call, at the reference's side)
		HIPCHK(ctx, hipMemcpyAsync(ctx->d_frame_cams, d_cams, (size_t)B * HT_CAM * sizeof(float), hipMemcpyDeviceToDevice, s));
		HIPCHK(ctx, hipMemsetAsync(ctx->d_overflow, 0, sizeof(int), s));
		if (own) { if (d_cams != ctx->d_cams) HIPCHK(ctx, hipMemcpyAsync(ctx->d_cams, d_cams, (size_t)B * HT_CAM * sizeof(float), hipMemcpyDeviceToDevice, s)); }      // segment.cam = the frame's camera
		else if (segment) ht_launch_segment(d_depth, ctx->d_frame_cams, fs.w, fs.h, 0xF, p.drangey, fs.segment_scale, ctx->d_seg_tiles, ctx->d_cams, B, s, fs.side);
		u.img_cams = ctx->d_frame_cams;
	}
	if (u.d_start && !tile)      // full-size frames re-seed the trackers with their own small kernels; for 64x64 tiles that, and the camera copy, ride on k_prepare (below)
	{ for (int w = 0; w < 2; w++) ht_launch_set_pose(ctx->d_state[w], u.d_start, ctx->model.nb, B, 1, s); ht_launch_clear_flags(ctx->d_prev_err, ctx->d_initializing, B, s); }
	{
		ht_prof_scope ps(ctx, "prepare", s, true);
		if (!tile)
		{
			const ht_prepare_extra pz = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, ctx->d_nflist };
			const bool by_prepare = u.net->dims.in == HT_CNN_IN;      // k_prepare makes the input of the net that looks at the reference's tile; a larger net takes its own from the input transform, off the frame itself or off the segment's tile (handtrack.h:700)
			if (own || (segment && !by_prepare)) { HIPCHK(ctx, hipMemsetAsync(ctx->d_nflist, 0, sizeof(int), s)); ht_launch_cnn_input(own ? d_depth : ctx->d_seg_tiles, ctx->d_cams, fs.side * fs.side, p.drangey, u.net->d_in, B, s); }
			else if (segment) ht_launch_prepare(ctx->d_seg_tiles, ctx->d_cams, p.drangey, p.subsample_fraction, u.net->d_in, nullptr, nullptr, ctx->model.pts_cap, B, s, &pz);
			ht_launch_prepare_frame(d_depth, u.img_cams, fs.w, fs.h, p.drangey, p.subsample_fraction, ctx->d_pts, ctx->d_npts, ctx->d_overflow, ctx->model.pts_cap, B, s);
		}
		else
		{
			const ht_prepare_extra px = { d_cams != ctx->d_cams ? ctx->d_cams : nullptr, ctx->d_state[0], ctx->d_state[1], u.d_start, ctx->d_prev_err, ctx->d_initializing, ctx->model.nb, ctx->d_nflist };
			ht_launch_prepare(d_depth, d_cams, p.drangey, p.subsample_fraction, u.net->d_in, ctx->d_pts, ctx->d_npts, ctx->model.pts_cap, B, s, &px);
		}
		if (main_thread_cloud_voxel(ctx, u))      // UPD_PASSES: the caller's part of the overlapped update runs its passes on this very cloud (handtrack.h:753)
		{
			// the main-thread cloud of handtrack.h:751 with the voxel rule: ALL in-range points (taken once more, into the cloud-row array, which nothing
			// uses before the first fit step) go through the voxel table; the CNN job keeps the every-n-th cloud above (handtrack.h:703)
			if (!ctx->d_ptsv) { int r = dev_alloc_points(ctx); if (r) return r; }
			float4 *all = reinterpret_cast<float4 *>(ctx->d_rows);
			if (!tile) ht_launch_prepare_frame(d_depth, u.img_cams, fs.w, fs.h, p.drangey, 1, all, ctx->d_nrows, ctx->d_overflow, ctx->model.pts_cap, B, s);
			else ht_launch_prepare(d_depth, ctx->d_cams, p.drangey, 1, nullptr, all, ctx->d_nrows, ctx->model.pts_cap, B, s);
			ht_launch_voxel(all, ctx->d_nrows, ctx->model.pts_cap, p.subsample_size, p.subsample_fraction, ctx->d_ptsv, ctx->d_nptsv, B, s);
		}
	}
	// batches of several rounds per CU: the block-per-frame kernels take the frames with the most points first, so that a launch ends on short blocks
	if (ctx->d_porder && several_rounds(ctx, B) && !exact_solver(ctx)) { ht_launch_order_by_points(ctx->d_npts, ctx->d_porder, B, s); ctx->model.frame_order = ctx->d_porder; }
	return HT_OK;
}
static void update_planes(ht_ctx *ctx, const update_call &u, hipStream_t t)      // the boundary planes of the main-thread cloud (handtrack.h:751, 774-778), once per update
{
	const ht_params &p = ctx->par;
	if (u.mode == UPD_CNN_MODEL || u.mode == UPD_KICKSTART || p.angles_only || p.mainthreadpasses < 1) return;
	ht_launch_chamber_planes(ctx->model, p.subsample_voxel ? ctx->d_ptsv : ctx->d_pts, p.subsample_voxel ? ctx->d_nptsv : ctx->d_npts, p.min_point_num, p.boundary_planes, ctx->d_chplanes, ctx->d_chon, u.B, t); ctx->planes_valid = true;
}
static void update_fit_error_old(ht_ctx *ctx, const update_call &u, hipStream_t t)      // FitError of the carried pose (handtrack.h:704) and the reset decision it ends with (:706)
{
	const ht_params &p = ctx->par;
	ht_fit_after dec; memset(&dec, 0, sizeof dec);
	dec.mode = 1; dec.reset_thr = p.full_reset_on_error; dec.angles_only = p.angles_only; dec.flags = ctx->d_flags; dec.nflags = ctx->d_nflags; dec.list = ctx->d_flist; dec.nlist = ctx->d_nflist; dec.nreset = ctx->d_nreset;
	ht_launch_fit_error(ctx->model, ctx->d_state[0], ctx->d_pts, ctx->d_npts, u.d_depth, u.img_cams, u.fs.w, u.fs.h, p.bone_sum_error_scale, ctx->d_err_old, u.B, t, &dec);
}
// The side branches beside the net, in dependency order.  Nothing on them needs the CNN.  What the update's stream waits for behind the net is the reset decision alone,
// so the carried pose's FitError (with the set_pose it reads behind) has side stream 1 to itself from the fork on and runs under the convolutions (ht_cnn.hip: ht_launch_cnn).
// The launch tables and the boundary planes have later consumers -- the batch's first contact launch and first solve, the first main pass -- and go to side stream 0, which
// has nothing else to do beside the net: ahead of FitError on its stream (rounds 5 to 10) they made it start 0.2 ms late, and the reset kernel waited for it 0.1 ms behind the net.
// Measured (profiles/r11_update_head.md): the reset kernel starts 46 us earlier in a 1024-frame step, 4.459 -> 4.412 and 4.474 -> 4.434 ms per step in two sessions, 19.54 -> 19.15 ms
// at 8192 frames.  Everything on side stream 1 with FitError first and one join was measured beside it: the same at 1024 frames (4.848 against 4.849 ms, tuning build), 0.05 ms slower at 8192.
// update_resets says when stream 0 comes back.  (The contacts of MultiStepSim's first step do not need the net either, but the contact kernel
// owns whole CUs and the FC layers want one block per CU: beside each other they took 0.78 ms, one after the other 0.46.)
static void update_beside_net(ht_ctx *ctx, const update_call &u)
{
	hipStream_t fit = ctx->side[1], rest = ctx->side[0];
	mark("update start", u.s);
	fork(ctx, u.s);
	if (u.mode == UPD_FULL && !(u.d_start && u.fs.kind == FRAME_TILE)) ht_launch_set_pose(ctx->d_state[1], ctx->d_state[0], ctx->model.nb, u.B, 2, fit);     // othermodel.SetPose(handmodel.GetPose()) handtrack.h:757 (both were just seeded with the same pose otherwise)
	update_fit_error_old(ctx, u, fit); mark("carried FitError done", fit);
	update_orders(ctx, u.B, rest); mark("orders done", rest);
	update_planes(ctx, u, rest); mark("planes done", rest);
	ctx->tables_out = true;      // until side stream 0 is joined (join1)
}
static void update_net(ht_ctx *ctx, const update_call &u, bool overlap)      // the net and its decode.  overlap: the side branch's FitError runs beside the net
{
	const ht_net &net = *u.net; hipStream_t s = u.s;
	ht_prof_scope ps(ctx, net.prof, s, true);
	ht_launch_cnn(net, net.d_in, ctx->d_act3, ctx->d_logits, u.B, s, overlap);
	ht_launch_softmax_decode(ctx->d_logits, u.d_cnn_out ? u.d_cnn_out : ctx->d_cnn_out, ctx->d_cams, ctx->d_analysis, 1, u.B, s, net.dims.sub);
}
// The three organisations of the full-reset frames beside the batch's MultiStepSim (update_resets picks one).
// The full-reset path touches few frames but is long (3 sequential single-body solves): it runs on a side stream while step 0 of
// MultiStepSim (which uses no cloud rows) proceeds for all other frames; the reset frames then do their step 0 on their own.
// (Taking the reset frames through ALL their steps on the side stream was measured: their five few-frame steps are pure latency and end
// later than the main stream's full-batch steps plus this one extra step, 4.6 against 4.5 ms.)
static void resets_short(ht_ctx *ctx, int B, hipStream_t s)      // p.steps < 2, or HT_NO_STEP1_LAP
{
	reset_path(ctx, true, ctx->par.steps_unibody, B, ctx->side[0], s, ctx->many_reset);
	multistep(ctx, B, steps_on(s).steps(0, 1).frames(ctx->d_nflags).rows_beside(0).shares_gpu());
	join(ctx, s, 1); reset_tail(ctx);
	multistep(ctx, B, steps_on(s).steps(0, 1).frames(ctx->d_flags).rows_beside(0));
	multistep(ctx, B, steps_on(s).steps(1).all_frames().rows_beside(0));
}
static void resets_joined_late(ht_ctx *ctx, int B, hipStream_t s, int join_step)      // experiment (HT_RESET_JOIN): the reset frames take steps [0, join_step) on the side stream
{
	reset_path(ctx, true, ctx->par.steps_unibody, B, ctx->side[0], s, ctx->many_reset);
	multistep(ctx, B, steps_on(ctx->side[0]).steps(0, join_step).frames(ctx->d_flags).in_order().unprofiled().shares_gpu());
	multistep(ctx, B, steps_on(s).steps(0, join_step).frames(ctx->d_nflags).rows_beside(1).shares_gpu());
	join(ctx, s, 1); reset_tail(ctx);
	multistep(ctx, B, steps_on(s).steps(join_step).all_frames().rows_beside(0));
}
static void resets_lap(ht_ctx *ctx, int B, hipStream_t s)      // p.steps >= 2
{
	// The reset frames' chain -- the reset kernel, then their own first step (eight frames: pure latency) -- is what the batch ends up waiting for, and its
	// few long blocks must find CUs although the batch's kernels ask for all of them (a cooperative contact block for a whole CU's LDS).  So the chain
	// stays on THIS stream, where it is dispatched the moment the CNN ends, and the batch's first step goes to the side stream, which only starts
	// after a cross-queue wait: launched the other way round the reset blocks often found no CU until the batch's contact kernel had finished.
	// While the reset frames take their first step the batch prepares its second (cloud rows and contacts of the other frames: a frame's rows and
	// contacts are its own), after the reset frames' contact blocks are in (same reason); the reset frames' rows for step 1 follow their solve on this
	// stream, beside the batch's.  Then ONE solve for all frames.  (The reset frames any further behind the batch was measured and does not pay:
	// DESIGN.md section 4.)  What the reset frames' contact blocks wait for (event marks): the batch's first solve -- both contact kernels want more
	// registers than a SIMD has left beside a solver wave (256 and 410 against 512 - 168), so they start when that solve ends, 0.55 ms after the fork,
	// however early the reset kernel is through (0.25 ms); making the batch's solve wait for them instead was measured: 5.39 against 5.31 ms.
	hipStream_t u = ctx->side[0];
	const int *reset_frames = ctx->d_flags, *batch_frames = ctx->d_nflags;
	mark("fork", s);
	reset_path(ctx, true, ctx->par.steps_unibody, B, s, s, ctx->many_reset); mark("reset kernel done", s);
	multistep(ctx, B, steps_on(u).steps(0, 1).frames(batch_frames).in_order().unprofiled().shares_gpu()); mark("batch step 0 done", u);
	multistep(ctx, B, steps_on(s).steps(0, 1).frames(reset_frames).in_order().rows_only()); mark("reset frames contacts done", s);
	(void)hipEventRecord(ctx->ev_lap, s); (void)hipStreamWaitEvent(u, ctx->ev_lap, 0);      // (consumer: the batch's step-1 kernels on the side stream; a record, it follows a contact launch)
	multistep(ctx, B, steps_on(s).steps(0, 1).frames(reset_frames).in_order().solve_only()); mark("reset frames step 0 done", s);
	multistep(ctx, B, steps_on(u).steps(1, 2).frames(batch_frames).in_order().unprofiled().rows_only()); mark("batch step 1 rows done", u);      // in order on the side stream: there is time (0.76 against 0.82 ms), and a fork out of a forked stream does not survive a HIP graph capture
	multistep(ctx, B, steps_on(s).steps(1, 2).frames(reset_frames).rows_beside(1).rows_only()); mark("reset frames step 1 rows done", s);      // the reset frames' rows for step 1, beside the batch's
	join(ctx, s, 1); mark("side branch back", s); reset_tail(ctx);      // the batch's steps so far, and ahead of them the tables and the planes of the update's head
	const steps_on rest = steps_on(s).steps(2).all_frames().rows_beside(0);
	multistep(ctx, B, steps_on(s).steps(1, 2).all_frames().solve_only().then_forks(ctx->par.steps > 2 && sides_of_step(ctx, rest, 2).par)); mark("step 1 done", s);
	multistep(ctx, B, rest); mark("MultiStepSim done", s);
}
// The overlapped update behind the net: the side branch comes back, then the reset frames and MultiStepSim in one of the organisations above
static void update_resets(ht_ctx *ctx, const update_call &u)
{
	hipStream_t s = u.s; mark("net done", s);
	static const int join_step = ht_tuning_int("HT_RESET_JOIN", 0);      // experiment (-DHT_TUNING): the reset frames take steps [0, join_step) on the side stream
	static const bool no_lap = ht_tuning_env("HT_NO_STEP1_LAP");      // experiment (-DHT_TUNING)
	const bool lap = join_step <= 0 && ctx->par.steps >= 2 && !no_lap;
	join1(ctx, s, 1);      // the reset decision comes back
	// The tables and the planes (side stream 0).  resets_lap runs the batch's first step in order on that very stream, behind them, and this stream launches nothing that
	// reads a table or the planes before it takes that stream back; the other organisations launch the batch's first contacts here, so the stream comes back first.
	if (!lap) join1(ctx, s, 0);
	mark(lap ? "reset decision back" : "side branch back", s);      // under resets_lap side stream 0 is still out
	fork(ctx, s);
	const unsigned frames = ctx->h_nreset[0], updates = ctx->h_nreset[1];      // few or many reset frames (ht_host.hpp: d_nreset): the average over the updates whose counts have arrived since the last look
	if (updates != ctx->nreset_seen[1])
	{
		ctx->many_reset = (frames - ctx->nreset_seen[0]) / (updates - ctx->nreset_seen[1]) > (unsigned)ctx->n_cu;
		ctx->nreset_seen[0] = frames; ctx->nreset_seen[1] = updates;
	}
	if (join_step > 0) resets_joined_late(ctx, u.B, s, join_step);
	else if (lap) resets_lap(ctx, u.B, s);
	else resets_short(ctx, u.B, s);
}
// FitError of the CNN-driven pose, and on its last thread the accept step (handtrack.h:713-731)
static void update_accept(ht_ctx *ctx, const update_call &u)
{
	const ht_params &p = ctx->par;
	ht_fit_after acc; memset(&acc, 0, sizeof acc);
	acc.mode = 2; acc.hand = u.mode == UPD_CNN_MODEL ? nullptr : ctx->d_state[0]; acc.other = ctx->d_state[1]; acc.err_old = ctx->d_err_old; acc.prev_err = ctx->d_prev_err;
	acc.initializing = ctx->d_initializing; acc.accepted = ctx->d_accepted; acc.nb = ctx->model.nb; acc.min_point_num = p.min_point_num; acc.always_take_cnn = p.always_take_cnn;
	acc.angles_only = p.angles_only; acc.accum_thr = p.accum_error_threshold; ht_prof_scope ps(ctx, "fit_error", u.s, true);
	ht_launch_fit_error(ctx->model, ctx->d_state[1], ctx->d_pts, ctx->d_npts, u.d_depth, u.img_cams, u.fs.w, u.fs.h, p.bone_sum_error_scale, ctx->d_err_new, u.B, u.s, &acc);
}
static void update_passes(ht_ctx *ctx, const update_call &u)      // the main-thread passes on handmodel and the user poses: the last pass's solve writes them, k_output when there is no pass
{
	const ht_params &p = ctx->par;
	const int passes = p.angles_only ? 0 : p.mainthreadpasses;
	for (int i = 0; i < passes; i++) { main_pass(ctx, u.B, u.s, i + 1 == passes ? u.d_poses_out : nullptr, i, i + 1 < passes); mark("pass done", u.s); }
	if (passes < 1) ht_launch_output(ctx->model, ctx->d_state[0], p.subsample_voxel ? ctx->d_nptsv : ctx->d_npts, ctx->d_initializing, p.min_point_num, u.d_poses_out, u.B, u.s);
}
static int run_update_(ht_ctx *ctx, update_call &u)
{
	const ht_params &p = ctx->par; hipStream_t s = u.s;
	u.net = ht_net_of(ctx, u.fs.side);      // (resolve_frames has checked the side)
	if (u.mode != UPD_PASSES && !u.net->have) { ctx->err = u.net->missing; return HT_ERR_STATE; }      // (no net in the caller's part of the overlapped update)
	{      // the launches of this update may carry its edges' events unless the caller is capturing its stream: every edge of a captured update is a record and a wait.
		// Nor under the profile (ht_profile_enable): its timing events bracket the very solves that would carry a fork, and a launch with a completion event between two
		// timing records costs more than the record it saves (bench.py --full, 1024 frames: 4.53 against 4.41 ms per step with a record per edge; the parent 4.46)
		hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
		const bool capturing = hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
		ctx->edges_on_launch = HT_EDGE_ON_LAUNCH && ctx->edge_mode == 0 && !capturing && !ctx->profile; ctx->fork_carried = nullptr; ctx->join_carried = 0;
	}
	{ const int r = update_inputs(ctx, u); if (r) return r; }
	if (u.mode == UPD_PASSES) { update_planes(ctx, u, s); update_passes(ctx, u); return HT_OK; }
	static const bool no_overlap = ht_tuning_env("HT_NO_OVERLAP");      // timing experiments (-DHT_TUNING builds only)
	const bool overlap = !no_overlap && !ctx->profile_phases && p.steps >= 1 && p.steps_cloudstart >= 1 && !p.angles_only && ctx->solver_build != 5;
	if (overlap) update_beside_net(ctx, u);
	else { update_orders(ctx, u.B, s); update_planes(ctx, u, s); }
	update_net(ctx, u, overlap);
	if (overlap) update_resets(ctx, u);
	else      // the same on one stream, in the reference's order
	{
		if (u.mode == UPD_FULL) ht_launch_set_pose(ctx->d_state[1], ctx->d_state[0], ctx->model.nb, u.B, 2, s);     // othermodel.SetPose(handmodel.GetPose()) handtrack.h:757
		{ ht_prof_scope ps(ctx, "fit_error", s, true); update_fit_error_old(ctx, u, s); }
		reset_path(ctx, true, p.steps_unibody, u.B, s, s);
		multistep(ctx, u.B, steps_on(s).all_frames().rows_beside(0));
	}
	update_accept(ctx, u);
	if (u.mode != UPD_FULL) { ht_launch_output(ctx->model, ctx->d_state[1], ctx->d_npts, ctx->d_initializing, p.min_point_num, u.d_poses_out, u.B, s, 1); reset_tail_join(ctx, s); join_open(ctx, s); return HT_OK; }      // othermodel.GetPose()
	mark("accept done", s);
	update_passes(ctx, u);
	reset_tail_join(ctx, s); join_open(ctx, s); mark("update done", s);
	marks_dump();
	return HT_OK;
}
static int run_update(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_start, int B, float *d_poses_out, float *d_cnn_out, hipStream_t s, const frame_src &fs, int mode = UPD_FULL)
{
	update_call u = { d_depth, d_cams, d_start, B, d_poses_out, d_cnn_out, s, fs, mode, nullptr, nullptr };
	const int r = run_update_(ctx, u);
	ctx->model.frame_order = nullptr; ctx->model.pts_bound = 0;      // the per-call hints of update_inputs (launch order of the block-per-frame kernels, largest cloud) belong to the update that set them
	ctx->planes_valid = false;                                       // and so do the boundary planes of its cloud
	ctx->edges_on_launch = false; ctx->fork_carried = nullptr; ctx->join_carried = 0;      // and the launch form of its edges (a fit step outside an update records its events)
	return r;
}
static int update_dev_end(ht_ctx *ctx, int r) { if (r) return r; HIPCHK(ctx, hipGetLastError()); return HT_OK; }      // what a *_dev update ends with: nothing is waited for, a launch that failed is reported

// ---- public entry points ----------------------------------------------------------------------------------------------
extern "C" int ht_tracker_reset(ht_ctx *ctx, int first, int n, const float *poses)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_RANGE(ctx, first, n);
	if (!poses) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	const int nb = ctx->model.nb;
	HIPCHK(ctx, hipMemcpyAsync(ctx->d_stage, poses, (size_t)n * nb * HT_POSE * sizeof(float), hipMemcpyHostToDevice, s));
	for (int w = 0; w < 2; w++) ht_launch_set_pose(ctx->d_state[w] + (size_t)first * nb * HT_STATE_STRIDE, ctx->d_stage, nb, n, 1, s);
	ht_launch_clear_flags(ctx->d_prev_err + first, ctx->d_initializing + first, n, s);
	return ht_sync_check(ctx, s);
}
extern "C" int ht_get_state(ht_ctx *ctx, int which, int first, int n, float *state)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_RANGE(ctx, first, n);
	if (!state || which < 0 || which > 1) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	const int nb = ctx->model.nb;
	ht_launch_get_state(ctx->d_state[which] + (size_t)first * nb * HT_STATE_STRIDE, ctx->d_stage, nb, n, s);
	HIPCHK(ctx, hipMemcpyAsync(state, ctx->d_stage, (size_t)n * nb * HT_STATE * sizeof(float), hipMemcpyDeviceToHost, s));
	return ht_sync_check(ctx, s);
}
extern "C" int ht_set_state(ht_ctx *ctx, int which, int first, int n, const float *state)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_RANGE(ctx, first, n);
	if (!state || which < 0 || which > 1) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	const int nb = ctx->model.nb;
	HIPCHK(ctx, hipMemcpyAsync(ctx->d_stage, state, (size_t)n * nb * HT_STATE * sizeof(float), hipMemcpyHostToDevice, s));
	ht_launch_set_pose(ctx->d_state[which] + (size_t)first * nb * HT_STATE_STRIDE, ctx->d_stage, nb, n, 3, s);
	return ht_sync_check(ctx, s);
}
extern "C" int ht_get_tracker_flags(ht_ctx *ctx, int first, int n, float *prev_frame_error, int *initializing)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_RANGE(ctx, first, n);
	HIPCHK(ctx, ht_sync_all(ctx));
	if (prev_frame_error) HIPCHK(ctx, hipMemcpy(prev_frame_error, ctx->d_prev_err + first, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
	if (initializing) HIPCHK(ctx, hipMemcpy(initializing, ctx->d_initializing + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
	return HT_OK;
}
extern "C" int ht_set_tracker_flags(ht_ctx *ctx, int first, int n, const float *prev_frame_error, const int *initializing)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_RANGE(ctx, first, n);
	if (prev_frame_error) HIPCHK(ctx, hipMemcpy(ctx->d_prev_err + first, prev_frame_error, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
	if (initializing) HIPCHK(ctx, hipMemcpy(ctx->d_initializing + first, initializing, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
	return HT_OK;
}
// Capacities of the contact kernel that the reference does not have: expanding-polytope runs cut short (128 iterations, 96 vertices, 192
// triangles in LDS; hull.h:246 loops without bound), touching samples beyond the 192 of a frame's pool, and solves whose angular rows exceed the 126
// the solver keeps (a model with many ranged joints).  Counted since ht_create; 0 on every
// workload of the test suite and the benches, so no result there depends on them.
extern "C" int ht_capacity_events(ht_ctx *ctx, int *epa_cut_short, int *contacts_dropped, int *angular_rows_over)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx);
	int v[3] = { 0, 0, 0 };
	HIPCHK(ctx, ht_sync_all(ctx));
	HIPCHK(ctx, hipMemcpy(v, ctx->d_epa_ws, sizeof v, hipMemcpyDeviceToHost));
	if (epa_cut_short) *epa_cut_short = v[0];
	if (contacts_dropped) *contacts_dropped = v[1];
	if (angular_rows_over) *angular_rows_over = v[2];
	return HT_OK;
}
// What the contact kernel's per-frame pool can be asked to hold AT MOST, from the model alone: FindShapeShapeContacts (physics.h:451-462) visits every pair of colliding bodies
// that do not ignore each other, and ContactPatch (gjk.h:607-643) returns one sample for a pair -- five only when neither body is smaller than the 0.05 m of its proximity test
// (the kernel's exact shortcut: DESIGN.md section 4).  samples_bound <= pool and patches_bound <= patch_slots is a PROOF that no touching sample can be dropped for this model
// (the stock hand: 91 pairs, none of them between two large bodies that do not ignore each other: 91 <= 192, 0 <= 40); otherwise the pool is a counted capacity
// (ht_capacity_events).  Follows ht_scale (the diameters grow with the model).
extern "C" int ht_contact_capacity(ht_ctx *ctx, int *samples_bound, int *patches_bound, int *pool, int *patch_slots)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx);
	const int nb = ctx->model.nb;
	int pairs = 0, big = 0;
	for (int i = 0; i < nb; i++) for (int j = i + 1; j < nb; j++)
	{
		if (!(ctx->model.collide[i] & ctx->model.collide[j] & 2)) continue;
		if (ctx->model.ignore[i] & (1u << j)) continue;
		pairs++;
		const float di = ctx->h_bodyc[(size_t)i * HT_BC + HT_BC_DIAM], dj = ctx->h_bodyc[(size_t)j * HT_BC + HT_BC_DIAM];
		if (!((di < dj ? di : dj) < 0.049f)) big++;
	}
	if (samples_bound) *samples_bound = pairs + 4 * big;
	if (patches_bound) *patches_bound = big;
	if (pool) *pool = HT_MAXCONTACT;
	if (patch_slots) *patch_slots = 40;      // GJK_JMAX (csrc/ht_gjk.hip)
	return HT_OK;
}
extern "C" int ht_frames_overflow(ht_ctx *ctx, int *frames_over)
{
	CHECK_READY(ctx);
	if (!frames_over) return HT_ERR_ARG;
	*frames_over = 0;
	HIPCHK(ctx, ht_sync_all(ctx));
	if (ctx->d_overflow) HIPCHK(ctx, hipMemcpy(frames_over, ctx->d_overflow, sizeof(int), hipMemcpyDeviceToHost));
	return HT_OK;
}
// ---- the update entry points: one frame source, one request ------------------------------------------------------------------------------------------------------
// The rules of the three families of entry points, stated once.  resolve_frames makes an entry's (family, side, w, h, segment_scale) into a frame_src and makes every
// argument check of the family, in this order; it is the only place that compares w, h and side with each other or with 64.
//   FRAMES_PLAIN   ht_update_*, ht_update_frames_*, ht_update_cnn_model_sync, ht_update_passes_sync, ht_job_start: HandTracker::update on frames of any size up to 320x240
//                  (handtrack.h:693-785) for the reference's net.  64x64 is the tile; anything else must pass ht_segment_supported and is segmented at 64.  No point limit.
//   FRAMES_SIZED   ht_update_frames_sized_*, ht_update_hands_*, ht_update_two_hands*: the same on frames up to 640x480 and for either net: HandSegmentVR (:280-344) cuts the
//                  segment at `side` (dstcam :338-340 is the only place the side enters), the net is the one of that input size, the decode camera camsub(segment.cam,
//                  side / 16) (:218-241); everything behind the net takes the segment's pose, which does not depend on the side.  The net of `side` must exist; the size
//                  must be side x side or pass ht_segment_supported_sized; the net's weights must be there; the cloud a frame can carry, as update_inputs counts it, must
//                  fit HT_POINTS_LIMIT.  side x side is the frame that is its own segment (:283-284; at side 64: the tile); a 64x64 frame at side 128 is segmented.
//   FRAMES_DIRECT  ht_update_direct_*: side x side frames that are their own segment (BASELINE configs[4] end to end, SURVEY 8d "config 5 (i)-(iii)"), no HandSegmentVR.
//                  Only the side is checked (missing weights are run_update_'s to report, behind the alignment rule of update_check).
enum frame_family { FRAMES_PLAIN, FRAMES_SIZED, FRAMES_DIRECT };
static int resolve_frames(ht_ctx *ctx, frame_family family, int side, int w, int h, float segment_scale, frame_src &fs)
{
	const frame_src tile = { FRAME_TILE, 64, 64, 64, 0.0f, true };
	const bool px64 = w == 64 && h == 64;
	if (family == FRAMES_PLAIN)
	{
		if (!px64 && !ht_segment_supported(w, h)) { ctx->err = "ht_update_frames: frame size must be a multiple of 4 and at most 320x240 pixels"; return HT_ERR_ARG; }
		fs = px64 ? tile : frame_src{ FRAME_SEGMENTED, w, h, 64, segment_scale, false };
		return HT_OK;
	}
	const ht_net *net = ht_net_of(ctx, side);
	if (!net) { ctx->err = (family == FRAMES_DIRECT ? "ht_update_direct: " : "ht_update_frames_sized: ") + ctx->err; return HT_ERR_ARG; }
	const bool own = family == FRAMES_DIRECT || (w == side && h == side);
	if (family == FRAMES_SIZED)
	{
		if (!own && !ht_segment_supported_sized(w, h, side)) { ctx->err = "ht_update_frames_sized: frame size must be a multiple of 4, at least 8x8 and at most 640x480 pixels (19200 quarter-size pixels)"; return HT_ERR_ARG; }
		if (!net->have) { ctx->err = net->missing; return HT_ERR_STATE; }
		const ht_params &p = ctx->par;
		const long long npx = (long long)w * h, fr = p.subsample_fraction > 0 ? p.subsample_fraction : 1, n = p.subsample_voxel ? npx : (npx + fr - 1) / fr;
		if (n > HT_POINTS_LIMIT) { ctx->err = "ht_update_frames_sized: these frames can carry " + std::to_string(n) + " points each, the per-point arrays hold at most 76800 (ht_reserve_points): raise subsample_fraction, and leave the voxel rule off"; return HT_ERR_ARG; }
	}
	if (!own) fs = frame_src{ FRAME_SEGMENTED, w, h, side, segment_scale, px64 };
	else fs = side == 64 ? tile : frame_src{ FRAME_OWN_SEGMENT, side, side, side, 0.0f, false };
	return HT_OK;
}

// ---- host forms: frames up ---------------------------------------------------------------------------------------------------------------------------
// Upload: a frame of a tile's pixels goes to d_depth / d_cams, a frame of any other size to d_frames (which follows the largest frame size seen) / d_frame_cams_in.
// *d_in, *d_cin: what run_update takes.  `depth`, `cams`: host memory (ht_job_start: its pinned copy).
static int stage_frames(ht_ctx *ctx, const uint16_t *depth, const float *cams, const frame_src &fs, int B, hipStream_t s, const uint16_t **d_in, const float **d_cin)
{
	uint16_t *dd = ctx->d_depth; float *dc = ctx->d_cams;
	const size_t npx = (size_t)fs.w * fs.h;
	if (!fs.px64)
	{
		int r;
		if ((r = dev_grow(ctx, &ctx->d_frames, &ctx->frames_cap, (size_t)ctx->B * npx))) return r;
		if (!ctx->d_frame_cams_in && (r = dev_alloc(ctx, &ctx->d_frame_cams_in, (size_t)ctx->B * HT_CAM))) return r;
		dd = ctx->d_frames; dc = ctx->d_frame_cams_in;
	}
	HIPCHK(ctx, hipMemcpyAsync(dd, depth, (size_t)B * npx * sizeof(uint16_t), hipMemcpyHostToDevice, s));
	HIPCHK(ctx, hipMemcpyAsync(dc, cams, (size_t)B * HT_CAM * sizeof(float), hipMemcpyHostToDevice, s));
	*d_in = dd; *d_cin = dc;
	return HT_OK;
}

// ---- the staging of the left-hand and two-hand calls (additions; DESIGN sections 26, 27, 31) ---------------------------------------------------------------------------
// A left-hand update is the existing update on the mirror image: frames, cameras and start poses of the flagged frames mirrored into a staging of the context
// (ht_mirror.hip), the update on that staging, the poses that come out mirrored in place.  The slots' state stays the right hand's.
// Two hands in one frame: B frames become 2B hand frames: the split (ht_split.hip) writes frame i's right hand into slot 2i of the same staging and its left hand,
// mirrored, into slot 2i + 1, with their cameras; the update runs on the staging; the odd slots' poses are mirrored back.  Slot state stays canonical.
// The staging: max_batch frames of `px` pixels, cameras and start poses, and the host form's flags.  Never smaller; growing is one synchronising re-allocation, the
// replacement made first (dev_grow), so a failure leaves what was there.
static int hands_reserve(ht_ctx *ctx, size_t px)
{
	int r;
	if (!ctx->d_hands_cams && ((r = dev_alloc(ctx, &ctx->d_hands_start, (size_t)ctx->B * ctx->model.nb * HT_POSE)) || (r = dev_alloc(ctx, &ctx->d_hands_flags, (size_t)ctx->B)) ||
	                           (r = dev_alloc(ctx, &ctx->d_hands_cams, (size_t)ctx->B * HT_CAM)))) return r;
	if (px <= ctx->hands_px) return HT_OK;
	HIPCHK(ctx, ht_sync_all(ctx));
	return dev_grow(ctx, &ctx->d_hands_frames, &ctx->hands_px, px, (size_t)ctx->B);
}
extern "C" int ht_reserve_hands(ht_ctx *ctx, int w, int h)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx);
	if (w < 1 || h < 1 || (long long)w * h > 640LL * 480) { ctx->err = "ht_reserve_hands: a frame of 1 to 640x480 pixels"; return HT_ERR_ARG; }
	return hands_reserve(ctx, (size_t)w * h);
}
extern "C" int ht_hands_capacity(ht_ctx *ctx, size_t *frame_pixels)
{
	CHECK_READY(ctx);
	if (!frame_pixels) return HT_ERR_ARG;
	*frame_pixels = ctx->hands_px;
	return HT_OK;
}
// model_mode: -1 the blob split; HT_SPLIT_MODEL_ALWAYS / _MERGED: the cells go to the nearer tracked model (ht_split_model.hip), priors the start poses
// where given, else the slots' own hand-model state (the left one canonical already)
struct two_hands_args { uint16_t lo, hi, step, far; int min_pixels, flags; float max_dist; int model_mode; };
static int two_hands_reserve(ht_ctx *ctx, int w, int h, bool model)
{
	int r = hands_reserve(ctx, (size_t)w * h);
	if (r) return r;
	if (!ctx->d_two_flags)
	{
		unsigned char *f = nullptr;
		if ((r = dev_alloc(ctx, &ctx->d_two_info, (size_t)ctx->B * 8)) || (r = dev_alloc(ctx, &f, (size_t)ctx->B))) return r;
		std::vector<unsigned char> pat((size_t)ctx->B);
		for (size_t i = 0; i < pat.size(); i++) pat[i] = (unsigned char)(i & 1);
		HIPCHK(ctx, hipMemcpy(f, pat.data(), pat.size(), hipMemcpyHostToDevice));
		ctx->d_two_flags = f;
	}
	if (model && (size_t)ctx->B > ctx->model_ncomp_cap)      // the blob split's counts [B / 2] and, behind them, the frames' sources [B / 2]
	{
		HIPCHK(ctx, ht_sync_all(ctx));
		if ((r = dev_grow(ctx, &ctx->d_model_ncomp, &ctx->model_ncomp_cap, (size_t)ctx->B))) return r;
	}
	const size_t cells = (size_t)(ctx->B / 2) * (w / 4) * (h / 4);
	if (cells > ctx->split_labels_cap) HIPCHK(ctx, ht_sync_all(ctx));
	return dev_grow(ctx, &ctx->d_split_labels, &ctx->split_labels_cap, cells);
}

// ---- one request -----------------------------------------------------------------------------------------------------------------------------------------------------
// Any update call: `entry` names it in the overflow report; (family, side, w, h, segment_scale) are the caller's, `fs` what update_check resolved them into; B frames in
// B slots, or with `two` in 2B; `hands`: a handedness flag per frame (null: none, nothing is staged); depth / cams / start / poses / info / source are host pointers in
// the host form's record and device pointers in the one update_enqueue takes.
struct update_req
{
	const char *entry; frame_family family; int side, w, h; float segment_scale; int mode, B; const uint16_t *depth; const float *cams; float *poses;      // what every entry gives, in this order
	const float *start; float *cnn; int *accepted; bool poses_optional; const unsigned char *hands; const two_hands_args *two; int32_t *info, *source;      // null / false unless the entry sets them
	frame_src fs;
	int slots() const { return two ? 2 * B : B; }
	bool staged() const { return hands || two; }
};
// Everything a call can be refused for, in the order the faults are reported; complete before anything is uploaded, grown or launched.  (The context itself: CHECK_READY,
// in update_dev / update_host, whose device guard has to outlive the call.)  dev: depth is the caller's device pointer.
static int update_check(ht_ctx *ctx, update_req &q, bool dev)
{
	CHECK_MODEL(ctx);
	const int B = q.B;      // (CHECK_BATCH's parameter is also the name of the context's capacity)
	if (!q.two) CHECK_BATCH(ctx, B);
	if (!q.depth || !q.cams || (!q.poses && !q.poses_optional)) return HT_ERR_ARG;
	if (q.two && (q.B < 1 || 2 * (long long)q.B > ctx->B)) { ctx->err = "ht_update_two_hands: two slots per frame: 2 * B exceeds the capacity given to ht_create"; return HT_ERR_ARG; }
	{ const int r = resolve_frames(ctx, q.family, q.side, q.w, q.h, q.segment_scale, q.fs); if (r) return r; }
	if (q.two)
	{
		const two_hands_args &a = *q.two;
		if (a.model_mode >= 0) { const int r = ht_split_model_check(ctx, "ht_update_two_hands_model", a.max_dist, a.model_mode, a.flags); if (r) return r; }
		const int r = ht_split_check(ctx, "ht_update_two_hands", q.w, q.h, a.lo, a.hi, a.min_pixels, a.far, a.flags); if (r) return r;
	}
	// the input transform of the larger net reads eight pixels per load off the frame that is its own segment: the caller's, unless the call stages (the context's staging is aligned)
	if (dev && q.fs.kind == FRAME_OWN_SEGMENT && !q.staged() && ((uintptr_t)q.depth & 15) != 0) { ctx->err = "ht_update_direct_dev: d_depth must be 16-byte aligned (the input transform reads eight pixels per 128-bit load)"; return HT_ERR_ARG; }
	return HT_OK;
}
static int update_reserve(ht_ctx *ctx, const update_req &q)      // the staging of a flagged or split call; may wait for the context's streams when it grows
{
	if (!q.staged()) return HT_OK;
	return q.two ? two_hands_reserve(ctx, q.w, q.h, q.two->model_mode >= 0) : hands_reserve(ctx, (size_t)q.w * q.h);
}
// A checked request on device pointers, all enqueued on s: mirror in or split where the call stages, the update, the poses of left hands mirrored back in place
static int update_enqueue(ht_ctx *ctx, const update_req &q, hipStream_t s)
{
	{ const int r = update_reserve(ctx, q); if (r) return r; }      // (nothing left to do behind the host form, which reserves before it uploads)
	const int nb = ctx->model.nb, n = q.slots();
	const uint16_t *d_depth = q.depth; const float *d_cams = q.cams, *d_start = q.start;
	const unsigned char *left = q.two ? ctx->d_two_flags : q.hands;      // the slots whose poses are a left hand's
	if (q.two)
	{
		const two_hands_args &a = *q.two; const int flags = a.flags | HT_SPLIT_MIRROR_LEFT; int32_t *d_info = q.info ? q.info : ctx->d_two_info;
		if (a.model_mode < 0) { ht_prof_scope ps(ctx, "k_split_label", s); ht_launch_split_label(d_depth, q.w, q.h, q.B, a.lo, a.hi, a.step, a.min_pixels, flags, d_info, nullptr, ctx->d_split_labels, s); }
		else ht_launch_split_model(ctx, d_depth, d_cams, d_start ? d_start : ctx->d_state[0], d_start ? HT_POSE : HT_STATE_STRIDE, d_start ? 0 : 1, q.w, q.h, q.B, a.lo, a.hi, a.step, a.min_pixels, a.max_dist, a.model_mode, flags,
		                           d_info, ctx->d_model_ncomp, q.source, nullptr, ctx->d_split_labels, s);
		{ ht_prof_scope ps(ctx, "k_split_write", s); ht_launch_split_write(d_depth, ctx->d_split_labels, d_info, q.w, q.h, q.B, a.far, flags, ctx->d_hands_frames, s); }
		{ ht_prof_scope ps(ctx, "k_split_cams", s); ht_launch_split_cams(d_cams, q.w, q.B, flags, ctx->d_hands_cams, s); }
	}
	else if (q.hands)
	{
		{ ht_prof_scope ps(ctx, "k_mirror_frames", s); ht_launch_mirror_frames(d_depth, q.w, q.h, q.B, left, ctx->d_hands_frames, s); }
		{ ht_prof_scope ps(ctx, "k_mirror_cams", s); ht_launch_mirror_cams(d_cams, q.w, q.B, left, ctx->d_hands_cams, s); }
	}
	if (q.staged())
	{
		if (d_start) { ht_prof_scope ps(ctx, "k_mirror_poses", s); ht_launch_mirror_poses(d_start, nb, n, left, ctx->d_hands_start, s); d_start = ctx->d_hands_start; }
		d_depth = ctx->d_hands_frames; d_cams = ctx->d_hands_cams;
	}
	{ const int r = run_update(ctx, d_depth, d_cams, d_start, n, q.poses, nullptr, s, q.fs, q.mode); if (r) return r; }
	if (q.staged()) { ht_prof_scope ps(ctx, "k_mirror_poses", s); ht_launch_mirror_poses(q.poses, nb, n, left, q.poses, s); }
	return HT_OK;
}
// The device form of every entry: nothing is waited for, a launch that failed is reported (update_dev_end)
static int update_dev(ht_ctx *ctx, update_req &q, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = update_check(ctx, q, true); if (r) return r; }
	return update_dev_end(ctx, update_enqueue(ctx, q, ht_user_stream(ctx, stream)));
}
// The host form: the staging reserved first (it may wait for the stream, and the uploads below are already on it), frames and flags up, the request on the context's
// own buffers, the split's records and the results the caller asked for down (accepted as 0 / 1), the stream drained.  Segmented frames whose clouds the point capacity
// cut short (d_overflow counts them) are an error, reported under the entry point's name.
static int update_host(ht_ctx *ctx, update_req &q)
{
	CHECK_READY(ctx);
	{ const int r = update_check(ctx, q, false); if (r) return r; }
	hipStream_t s = ctx->stream;
	update_req d = q;
	int r = update_reserve(ctx, q);
	if (!r) r = stage_frames(ctx, q.depth, q.cams, q.fs, q.B, s, &d.depth, &d.cams);
	if (r) return r;
	d.start = nullptr; d.poses = ctx->d_poses_out;
	if (q.hands) { HIPCHK(ctx, hipMemcpyAsync(ctx->d_hands_flags, q.hands, (size_t)q.B, hipMemcpyHostToDevice, s)); d.hands = ctx->d_hands_flags; }
	if (q.two) { d.info = ctx->d_two_info; d.source = q.two->model_mode >= 0 ? ctx->d_model_ncomp + ctx->B / 2 : nullptr; }
	if ((r = update_enqueue(ctx, d, s))) return r;
	if (q.two && q.info) HIPCHK(ctx, hipMemcpyAsync(q.info, d.info, (size_t)q.B * 16 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
	if (q.two && q.source && d.source) HIPCHK(ctx, hipMemcpyAsync(q.source, d.source, (size_t)q.B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
	const int n = q.slots();
	if (q.poses) HIPCHK(ctx, hipMemcpyAsync(q.poses, ctx->d_poses_out, (size_t)n * ctx->model.nb * HT_POSE * sizeof(float), hipMemcpyDeviceToHost, s));
	if (q.accepted) HIPCHK(ctx, hipMemcpyAsync(q.accepted, ctx->d_accepted, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
	if (q.cnn) HIPCHK(ctx, hipMemcpyAsync(q.cnn, ctx->d_cnn_out, (size_t)n * HT_CNN_OUT * sizeof(float), hipMemcpyDeviceToHost, s));
	if ((r = ht_sync_check(ctx, s))) return r;
	if (q.accepted) for (int b = 0; b < n; b++) q.accepted[b] = q.accepted[b] != 0;
	int over = 0;
	if (q.fs.kind == FRAME_SEGMENTED) HIPCHK(ctx, hipMemcpy(&over, ctx->d_overflow, sizeof(int), hipMemcpyDeviceToHost));
	if (over) { ctx->err = std::string(q.entry) + ": " + std::to_string(over) + " frame(s) have more in-range points than the context's point capacity holds; their result is not the reference's"; return HT_ERR_ARG; }
	return HT_OK;
}

// ---- the entries: fill the record, hand it to the device or the host form ----------------------------------------------------------------------------------------------
extern "C" int ht_update_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_start_poses, int B, float *d_poses_out, void *stream)
{
	update_req q = { "ht_update", FRAMES_PLAIN, 64, 64, 64, 0.0f, UPD_FULL, B, d_depth, d_cams, d_poses_out }; q.start = d_start_poses;
	return update_dev(ctx, q, stream);
}
extern "C" int ht_update_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int B, float *poses_out, float *cnn_out)
{
	update_req q = { "ht_update", FRAMES_PLAIN, 64, 64, 64, 0.0f, UPD_FULL, B, depth, cams, poses_out }; q.cnn = cnn_out;
	return update_host(ctx, q);
}
extern "C" int ht_update_frames_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, const float *d_start_poses, int B, float *d_poses_out, void *stream)
{
	update_req q = { "ht_update_frames", FRAMES_PLAIN, 64, w, h, segment_scale, UPD_FULL, B, d_depth, d_cams, d_poses_out }; q.start = d_start_poses;
	return update_dev(ctx, q, stream);
}
extern "C" int ht_update_frames_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, int B, float *poses_out, float *cnn_out)
{
	update_req q = { "ht_update_frames", FRAMES_PLAIN, 64, w, h, segment_scale, UPD_FULL, B, depth, cams, poses_out }; q.cnn = cnn_out;
	return update_host(ctx, q);
}
extern "C" int ht_update_frames_sized_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, const float *d_start_poses, int B, float *d_poses_out, void *stream)
{
	update_req q = { "ht_update_frames_sized", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, d_depth, d_cams, d_poses_out }; q.start = d_start_poses;
	return update_dev(ctx, q, stream);
}
extern "C" int ht_update_frames_sized_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, int B, float *poses_out, float *cnn_out)
{
	update_req q = { "ht_update_frames_sized", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, depth, cams, poses_out }; q.cnn = cnn_out;
	return update_host(ctx, q);
}
// ---- several views (ht_views.hip): ht_update_frames_sized_* on view 0, the existing request unchanged, then the fused cloud of all views and `passes`
// fits of the handmodel against it; the last of them writes the poses the caller gets.  The net, the segmentation, FitError and MultiStepSim see view 0 only.
struct views_req { const float *planes; int V; const ht_views *opt; int passes; };
// everything the call can be refused for or has to grow, before anything runs: the view-0 request, the fused cloud, the fit, the contiguous copy of view 0
static int update_views_prepare(ht_ctx *ctx, update_req &q, const views_req &v, bool dev)
{
	{ const int r = update_check(ctx, q, dev); if (r) return r; }
	{ const int r = ht_fuse_views_reserve(ctx, "ht_update_views", q.depth, q.cams, q.w, q.h, v.V, q.B, v.opt); if (r) return r; }
	if (v.passes < 1 || v.passes > 64) { ctx->err = "ht_update_views: passes between 1 and 64"; return HT_ERR_ARG; }
	REFUSE_EXACT_SOLVER(ctx);
	if (v.V > 1)
	{
		const size_t px = (size_t)q.w * q.h;
		if (px > ctx->view0_cap) HIPCHK(ctx, ht_sync_all(ctx));
		int r;
		if ((r = dev_grow(ctx, &ctx->d_view0, &ctx->view0_cap, px, (size_t)ctx->B)) || (!ctx->d_view0_cams && (r = dev_alloc(ctx, &ctx->d_view0_cams, (size_t)ctx->B * HT_CAM)))) return r;
	}
	return HT_OK;
}
// q: the request on device pointers, depth [B][V][h][w] and cams [B][V][12]
static int update_views_enqueue(ht_ctx *ctx, const update_req &q, const views_req &v, hipStream_t s)
{
	update_req q0 = q;
	const size_t px = (size_t)q.w * q.h;
	if (v.V > 1)      // view 0 of every slot, contiguous, as the update takes its frames
	{
		HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_view0, px * sizeof(uint16_t), q.depth, v.V * px * sizeof(uint16_t), px * sizeof(uint16_t), q.B, hipMemcpyDeviceToDevice, s));
		HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_view0_cams, HT_CAM * sizeof(float), q.cams, (size_t)v.V * HT_CAM * sizeof(float), HT_CAM * sizeof(float), q.B, hipMemcpyDeviceToDevice, s));
		q0.depth = ctx->d_view0; q0.cams = ctx->d_view0_cams;
	}
	int r;
	if ((r = update_enqueue(ctx, q0, s))) return r;
	if ((r = ht_fuse_views_enqueue(ctx, q.depth, q.cams, v.planes, q.w, q.h, v.V, q.B, v.opt, nullptr, nullptr, nullptr, nullptr, s))) return r;
	return ht_fit_views_enqueue(ctx, 0, q.B, v.passes, q.poses, s);
}
extern "C" int ht_update_views_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, float segment_scale, const float *d_start_poses, int B,
                                   const ht_views *o, int passes, float *d_poses_out, void *stream)
{
	update_req q = { "ht_update_views", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, d_depth, d_cams, d_poses_out }; q.start = d_start_poses;
	const views_req v = { d_planes, V, o, passes };
	CHECK_READY(ctx);
	{ const int r = update_views_prepare(ctx, q, v, true); if (r) return r; }
	return update_dev_end(ctx, update_views_enqueue(ctx, q, v, ht_user_stream(ctx, stream)));
}
extern "C" int ht_update_views_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, const float *planes, int w, int h, int V, float segment_scale, int B, const ht_views *o, int passes,
                                    float *poses_out, float *cnn_out)
{
	update_req q = { "ht_update_views", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, depth, cams, poses_out };
	const views_req v = { planes, V, o, passes };
	CHECK_READY(ctx);
	{ const int r = update_views_prepare(ctx, q, v, false); if (r) return r; }
	const size_t n = (size_t)B, nv = n * V;
	for (size_t b = 0; b < n; b++)      // the reference's PointCloud is camera-local (handtrack.h:703): view 0 is the tracking space
	{
		const float *c = cams + b * V * HT_CAM;
		if (!(c[5] == 0.0f && c[6] == 0.0f && c[7] == 0.0f && c[8] == 0.0f && c[9] == 0.0f && c[10] == 0.0f && c[11] == 1.0f)) { ctx->err = "ht_update_views: view 0's camera pose must be identity (the other views are posed in its space)"; return HT_ERR_ARG; }
	}
	{ const int r = ht_views_planes_ok(ctx, "ht_update_views", planes, nv); if (r) return r; }
	ht_seg seg[4] = { { (void *)depth, nv * w * h * sizeof(uint16_t), false }, { (void *)cams, nv * HT_CAM * sizeof(float), false }, { (void *)planes, nv * 4 * sizeof(float), false },
	                  { poses_out, n * ctx->model.nb * HT_POSE * sizeof(float), true } };
	const int r = ht_staged_call(ctx, seg, 4, [&](hipStream_t s)
	                             {
		                             update_req d = q; d.depth = (const uint16_t *)seg[0].dev; d.cams = (const float *)seg[1].dev; d.poses = (float *)seg[3].dev;
		                             const views_req dv = { (const float *)seg[2].dev, V, o, passes };
		                             return update_views_enqueue(ctx, d, dv, s);
	                             });
	if (r) return r;
	HIPCHK(ctx, hipGetLastError());
	if (cnn_out) HIPCHK(ctx, hipMemcpy(cnn_out, ctx->d_cnn_out, n * HT_CNN_OUT * sizeof(float), hipMemcpyDeviceToHost));
	int over = 0;
	if (q.fs.kind == FRAME_SEGMENTED) HIPCHK(ctx, hipMemcpy(&over, ctx->d_overflow, sizeof(int), hipMemcpyDeviceToHost));
	if (over) { ctx->err = "ht_update_views: " + std::to_string(over) + " frame(s) have more in-range points than the context's point capacity holds; their result is not the reference's"; return HT_ERR_ARG; }
	return HT_OK;
}
extern "C" int ht_update_direct_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int side, const float *d_start_poses, int B, float *d_poses_out, void *stream)
{
	update_req q = { "ht_update_direct", FRAMES_DIRECT, side, side, side, 0.0f, UPD_FULL, B, d_depth, d_cams, d_poses_out }; q.start = d_start_poses;
	return update_dev(ctx, q, stream);
}
extern "C" int ht_update_direct_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int side, int B, float *poses_out, float *cnn_out)
{
	update_req q = { "ht_update_direct", FRAMES_DIRECT, side, side, side, 0.0f, UPD_FULL, B, depth, cams, poses_out }; q.cnn = cnn_out;
	return update_host(ctx, q);
}
// Without flags the call IS ht_update_frames_sized_*, on the caller's own pointers: no mirror launch, no staging, that call's name and alignment rule
extern "C" int ht_update_hands_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, const unsigned char *d_hands, const float *d_start_poses, int B, float *d_poses_out, void *stream)
{
	update_req q = { d_hands ? "ht_update_hands" : "ht_update_frames_sized", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, d_depth, d_cams, d_poses_out }; q.start = d_start_poses; q.hands = d_hands;
	return update_dev(ctx, q, stream);
}
extern "C" int ht_update_hands_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, const unsigned char *hands, int B, float *poses_out, float *cnn_out)
{
	update_req q = { hands ? "ht_update_hands" : "ht_update_frames_sized", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, depth, cams, poses_out }; q.cnn = cnn_out; q.hands = hands;
	return update_host(ctx, q);
}
extern "C" int ht_update_two_hands_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, uint16_t range_lo, uint16_t range_hi, uint16_t max_step,
                                       int min_pixels, uint16_t far, int flags, const float *d_start_poses, int B, float *d_poses_out, int32_t *d_info, void *stream)
{
	const two_hands_args a = { range_lo, range_hi, max_step, far, min_pixels, flags, 0.0f, -1 };
	update_req q = { "ht_update_two_hands", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, d_depth, d_cams, d_poses_out }; q.start = d_start_poses; q.two = &a; q.info = d_info;
	return update_dev(ctx, q, stream);
}
extern "C" int ht_update_two_hands_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, uint16_t range_lo, uint16_t range_hi, uint16_t max_step,
                                        int min_pixels, uint16_t far, int flags, int B, float *poses_out, int32_t *info, float *cnn_out)
{
	const two_hands_args a = { range_lo, range_hi, max_step, far, min_pixels, flags, 0.0f, -1 };
	update_req q = { "ht_update_two_hands", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, depth, cams, poses_out }; q.cnn = cnn_out; q.two = &a; q.info = info;
	return update_host(ctx, q);
}
// The same calls with the model split in front.  mode below 0 would name the blob split: refused with every other unknown mode.  HT_SPLIT_USER_POSES
// is the split calls' alone: d_start_poses also seed the slots, as centre-of-mass poses
extern "C" int ht_update_two_hands_model_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, uint16_t range_lo, uint16_t range_hi, uint16_t max_step,
                                             int min_pixels, uint16_t far, float max_dist, int mode, int flags, const float *d_start_poses, int B, float *d_poses_out, int32_t *d_info, int32_t *d_source, void *stream)
{
	const two_hands_args a = { range_lo, range_hi, max_step, far, min_pixels, flags, max_dist, mode < 0 ? 0x7fffffff : mode };
	update_req q = { "ht_update_two_hands", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, d_depth, d_cams, d_poses_out }; q.start = d_start_poses; q.two = &a; q.info = d_info; q.source = d_source;
	return update_dev(ctx, q, stream);
}
extern "C" int ht_update_two_hands_model_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, uint16_t range_lo, uint16_t range_hi, uint16_t max_step,
                                              int min_pixels, uint16_t far, float max_dist, int mode, int flags, int B, float *poses_out, int32_t *info, int32_t *source, float *cnn_out)
{
	const two_hands_args a = { range_lo, range_hi, max_step, far, min_pixels, flags, max_dist, mode < 0 ? 0x7fffffff : mode };
	update_req q = { "ht_update_two_hands", FRAMES_SIZED, side, w, h, segment_scale, UPD_FULL, B, depth, cams, poses_out }; q.cnn = cnn_out; q.two = &a; q.info = info; q.source = source;
	return update_host(ctx, q);
}
// HandTracker::update_cnn_model (handtrack.h:734-741) and kickstart (:743-746) for B trackers; every output is optional
extern "C" int ht_update_cnn_model_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, int B, int apply_to_handmodel,
                                        float *poses_out, int *accepted_out, float *cnn_out)
{
	update_req q = { "ht_update_cnn_model", FRAMES_PLAIN, 64, w, h, segment_scale, apply_to_handmodel ? UPD_KICKSTART : UPD_CNN_MODEL, B, depth, cams, poses_out };
	q.cnn = cnn_out; q.accepted = accepted_out; q.poses_optional = true;
	return update_host(ctx, q);
}
// ---- the reference's OVERLAPPED update() (handtrack.h:748-785) on two contexts of one device ----------------------------------------------------------------
// The reference runs the CNN job (update_cnn_model_threadsafe: net, decode, FitError, reset, MultiStepSim, accept decision) on a background thread and lets the caller go
// on with the main-thread passes; the job's pose is taken over by a later call, when the job is through (:760-768).  Here the job runs on a second context `job` (its own
// streams, buffers and othermodel) beside the caller's context `main`, whose update call does the cloud, the passes and the user poses only:
//   ht_job_start    othermodel.SetPose(handmodel.GetPose()) (:757) -- main's handmodel and tracker flags are copied to `job` --, the frame goes to pinned staging and the
//                   job is enqueued on job's stream; returns without waiting (what std::async does, :758)
//   ht_job_poll     pose_estimator.wait_for(...) == ready (:760) as a hipEventQuery
//   ht_job_collect  handmodel.SetPose(results.pose) (:767) where the job accepted its pose (an empty pose changes nothing); prev_frame_error as the job left it, and the
//                   job's `initializing = max(initializing - 1, 0)` (:726) applied to main's CURRENT value (the caller's own `initializing = 50` (:781) may have intervened:
//                   the reference shares the variable between the threads)
//   ht_update_passes_sync   the caller's part: points, mainthreadpasses x (HandModelEnhancements, cloud_chamber, FitPointCloud), the initializing rule, GetPoseUser
__global__ void k_job_collect(float *__restrict__ hand, const float *__restrict__ other, const int *__restrict__ accepted, float *__restrict__ prev_err, const float *__restrict__ job_prev_err, int *__restrict__ initializing, int nb, int n)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * nb) return;
	const int f = i / nb;
	if (accepted[f]) { float *s = hand + (size_t)i * HT_STATE_STRIDE; const float *o = other + (size_t)i * HT_STATE_STRIDE; for (int k = 0; k < 7; k++) s[k] = o[k]; }
	if (i == f * nb) { prev_err[f] = job_prev_err[f]; const int v = initializing[f] - 1; initializing[f] = v < 0 ? 0 : v; }
}
extern "C" int ht_update_passes_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, int B, float *poses_out)
{
	update_req q = { "ht_update_passes", FRAMES_PLAIN, 64, w, h, 0.17f, UPD_PASSES, B, depth, cams, poses_out };
	return update_host(ctx, q);
}
extern "C" int ht_job_start(ht_ctx *job, ht_ctx *main, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, int B)
{
	CHECK_READY(job); CHECK_MODEL(job); CHECK_BATCH(job, B);
	if (!main || !depth || !cams || main == job || main->device != job->device || main->model.nb != job->model.nb || B > main->B) { job->err = "ht_job_start: the two contexts must be different ones of one device with the same model"; return HT_ERR_ARG; }
	if (job->job_pending) { job->err = "ht_job_start: a job is in flight on this context (ht_job_collect takes it over)"; return HT_ERR_STATE; }
	frame_src fs;
	{ const int r = resolve_frames(job, FRAMES_PLAIN, 64, w, h, segment_scale, fs); if (r) return r; }
	hipStream_t s = job->stream;
	const int nb = job->model.nb;
	const size_t npx = (size_t)w * h, in_bytes = (size_t)B * npx * sizeof(uint16_t), cam_bytes = (size_t)B * HT_CAM * sizeof(float);
	if (!job->ev_job) HIPCHK(job, hipEventCreateWithFlags(&job->ev_job, hipEventDisableTiming));      // (the host queries and waits for this one: the ordinary fence, not ht_edge_event)
	if (job->h_job_cap < in_bytes + cam_bytes) { if (job->h_job_in) (void)hipHostFree(job->h_job_in); job->h_job_in = nullptr; HIPCHK(job, hipHostMalloc(&job->h_job_in, in_bytes + cam_bytes, hipHostMallocDefault)); job->h_job_cap = in_bytes + cam_bytes; }
	HIPCHK(job, hipStreamSynchronize(main->stream));      // the caller's context is between two of its (synchronous) calls: its handmodel is final
	memcpy(job->h_job_in, depth, in_bytes); memcpy((char *)job->h_job_in + in_bytes, cams, cam_bytes);      // the caller's image need not outlive this call (the reference moves it into the task)
	const uint16_t *d_in; const float *d_cin;
	{ const int r = stage_frames(job, (const uint16_t *)job->h_job_in, (const float *)((const char *)job->h_job_in + in_bytes), fs, B, s, &d_in, &d_cin); if (r) return r; }
	// the job looks at handmodel (FitError of the carried pose, :704) and starts othermodel from its pose (:757); prev_frame_error and initializing as they stand
	HIPCHK(job, hipMemcpyAsync(job->d_state[0], main->d_state[0], (size_t)B * nb * HT_STATE_STRIDE * sizeof(float), hipMemcpyDeviceToDevice, s));
	ht_launch_set_pose(job->d_state[1], main->d_state[0], nb, B, 2, s);
	HIPCHK(job, hipMemcpyAsync(job->d_prev_err, main->d_prev_err, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
	HIPCHK(job, hipMemcpyAsync(job->d_initializing, main->d_initializing, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
	// othermodel's seed is taken BEFORE the caller goes on (the reference copies synchronously in front of std::async, :757): the caller's stream waits for these copies, so its
	// next passes cannot overwrite handmodel under them
	if (!job->ev_seed) HIPCHK(job, ht_edge_event(job, &job->ev_seed));      // (consumer: the kernels of the caller's next passes on main's stream, same device)
	HIPCHK(job, hipEventRecord(job->ev_seed, s));
	HIPCHK(job, hipStreamWaitEvent(main->stream, job->ev_seed, 0));
	int r = run_update(job, d_in, d_cin, nullptr, B, job->d_poses_out, nullptr, s, fs, UPD_CNN_MODEL);
	if (r) { (void)hipStreamSynchronize(s); return r; }      // the queued uploads read h_job_in: nothing may be in flight when the caller frees or reuses it
	HIPCHK(job, hipEventRecord(job->ev_job, s));
	job->job_pending = true;
	return HT_OK;
}
extern "C" int ht_job_poll(ht_ctx *job, int *ready)
{
	if (!job || !ready) return HT_ERR_ARG;
	ht_device_guard dev_guard_(job->device);
	*ready = 0;
	if (!job->job_pending) return HT_OK;
	const hipError_t e = hipEventQuery(job->ev_job);
	if (e == hipSuccess) *ready = 1;
	else if (e != hipErrorNotReady) { job->err = std::string("ht_job_poll: ") + hipGetErrorString(e); return HT_ERR_HIP; }
	return HT_OK;
}
extern "C" int ht_job_wait(ht_ctx *job)
{
	if (!job) return HT_ERR_ARG;
	ht_device_guard dev_guard_(job->device);
	if (job->job_pending) HIPCHK(job, hipEventSynchronize(job->ev_job));
	return HT_OK;
}
extern "C" int ht_job_collect(ht_ctx *job, ht_ctx *main, int B, int *accepted_out)
{
	CHECK_READY(job); CHECK_MODEL(job); CHECK_BATCH(job, B);
	if (!main || main == job || main->device != job->device || main->model.nb != job->model.nb || B > main->B) return HT_ERR_ARG;
	if (!job->job_pending) { job->err = "ht_job_collect: no job in flight"; return HT_ERR_STATE; }
	HIPCHK(job, hipEventSynchronize(job->ev_job));
	const int nb = job->model.nb;
	hipLaunchKernelGGL(k_job_collect, dim3((B * nb + 255) / 256), dim3(256), 0, main->stream, main->d_state[0], job->d_state[1], job->d_accepted, main->d_prev_err, job->d_prev_err, main->d_initializing, nb, B);
	if (accepted_out) { HIPCHK(job, hipMemcpyAsync(accepted_out, job->d_accepted, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, main->stream)); }
	HIPCHK(job, hipStreamSynchronize(main->stream));
	if (accepted_out) for (int b = 0; b < B; b++) accepted_out[b] = accepted_out[b] != 0;
	job->job_pending = false;
	return HT_OK;
}
// Results of the CNN job of the latest update call of slots [first, first + n): HandTracker::cnn_input / cnn_output (handtrack.h:583-584) and the
// decoded CNNOutputAnalysis (:182-242; layout as ht_stage_decode).  Any pointer may be NULL.
extern "C" int ht_get_cnn_results(ht_ctx *ctx, int first, int n, float *cnn_input, float *cnn_output, float *analysis)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_RANGE(ctx, first, n);
	HIPCHK(ctx, ht_sync_all(ctx));
	const ht_net &tile = *ht_net_of(ctx, 64);
	if (cnn_input) HIPCHK(ctx, hipMemcpy(cnn_input, tile.d_in + (size_t)first * tile.dims.in, (size_t)n * tile.dims.in * sizeof(float), hipMemcpyDeviceToHost));
	if (cnn_output) HIPCHK(ctx, hipMemcpy(cnn_output, ctx->d_cnn_out + (size_t)first * HT_CNN_OUT, (size_t)n * HT_CNN_OUT * sizeof(float), hipMemcpyDeviceToHost));
	if (analysis) HIPCHK(ctx, hipMemcpy(analysis, ctx->d_analysis + (size_t)first * HT_ANALYSIS, (size_t)n * HT_ANALYSIS * sizeof(float), hipMemcpyDeviceToHost));
	return HT_OK;
}

// The CNN's intermediate layers of the latest evaluation (ht_cnn_eval, an update call) of slots [first, first + n), for per-layer parity tests:
// act1 [n][3600] = layer 3 of the reference's list (conv 5x5, tanh, two 2x2 max-pools: 16 x 15 x 15), act2 [n][2304] = layer 6 (conv 4x4, tanh, pool: 64 x 6 x 6),
// act3 [n][2048] = layer 8 (first fully connected layer + tanh), logits [n][2304] = layer 9 (second fully connected layer, before the chunked soft-max).
// The net's own convolution buffers (act1 [n][dims.act1], act2 [n][dims.act2]) exist once it has any: the 64x64-input net's from the start, the larger net's with its
// weights; act3 and the logits are the one pair both nets write.
static int get_cnn_layers(ht_ctx *ctx, const ht_net *net, int first, int n, float *act1, float *act2, float *act3, float *logits)
{
	if (!net) return HT_ERR_ARG;
	CHECK_RANGE(ctx, first, n);
	if (!net->d_act1) { ctx->err = net->missing; return HT_ERR_STATE; }
	const size_t n1 = net->dims.act1, n2 = net->dims.act2;
	HIPCHK(ctx, ht_sync_all(ctx));
	if (act1) HIPCHK(ctx, hipMemcpy(act1, net->d_act1 + (size_t)first * n1, (size_t)n * n1 * sizeof(float), hipMemcpyDeviceToHost));
	if (act2) HIPCHK(ctx, hipMemcpy(act2, net->d_act2 + (size_t)first * n2, (size_t)n * n2 * sizeof(float), hipMemcpyDeviceToHost));
	if (act3)      // the device holds the layer in the column order the last layer's kernel reads (k_fc<PACK16>): position (c & ~15) | (c & 3) << 2 | (c >> 2) & 3 holds column c
	{
		std::vector<float> packed((size_t)n * 2048);
		HIPCHK(ctx, hipMemcpy(packed.data(), ctx->d_act3 + (size_t)first * 2048, (size_t)n * 2048 * sizeof(float), hipMemcpyDeviceToHost));
		for (int r = 0; r < n; r++) for (int c = 0; c < 2048; c++) act3[(size_t)r * 2048 + c] = packed[(size_t)r * 2048 + ((c & ~15) | ((c & 3) << 2) | ((c >> 2) & 3))];
	}
	if (logits) HIPCHK(ctx, hipMemcpy(logits, ctx->d_logits + (size_t)first * HT_CNN_OUT, (size_t)n * HT_CNN_OUT * sizeof(float), hipMemcpyDeviceToHost));
	return HT_OK;
}
extern "C" int ht_get_cnn_layers(ht_ctx *ctx, int first, int n, float *act1, float *act2, float *act3, float *logits) { CHECK_READY(ctx); return get_cnn_layers(ctx, ht_net_of(ctx, 64), first, n, act1, act2, act3, logits); }
// the same of the net with a side x side input
extern "C" int ht_get_cnn_layers_sized(ht_ctx *ctx, int side, int first, int n, float *act1, float *act2, float *act3, float *logits) { CHECK_READY(ctx); return get_cnn_layers(ctx, ht_net_of(ctx, side), first, n, act1, act2, act3, logits); }

// ---- stage entry points (operate on the buffers ht_stage_prepare filled and on the tracker state of slots [0,B)) -------------
extern "C" int ht_stage_fit_error(ht_ctx *ctx, int which, int B, float *err)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (!err || which < 0 || which > 1) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	ht_launch_fit_error(ctx->model, ctx->d_state[which], ctx->d_pts, ctx->d_npts, ctx->d_depth, ctx->d_cams, 64, 64, ctx->par.bone_sum_error_scale, ctx->d_err_old, B, s);
	HIPCHK(ctx, hipMemcpyAsync(err, ctx->d_err_old, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
	return ht_sync_check(ctx, s);
}
extern "C" int ht_stage_cloud_rows(ht_ctx *ctx, int which, int stride, int use_cam_origin, int B, float *rows, int *nrows)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (!rows || !nrows || which < 0 || which > 1 || stride < 1) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	HIPCHK(ctx, hipMemsetAsync(ctx->d_rows, 0, (size_t)B * ctx->model.pts_cap * HT_ROW * sizeof(float), s));
	const cloud_take take = { stride, use_cam_origin, CLOUD_UNIT };
	ht_launch_cloud_rows(ctx->model, ctx->d_state[which], ctx->d_pts, ctx->d_npts, ctx->d_cams, nullptr, take, ht_cloud_limits(ctx->par, CLOUD_UNIT), ctx->d_rows, ctx->d_nrows, B, s);
	HIPCHK(ctx, hipMemcpy2DAsync(rows, HT_MAXPTS * HT_ROW * sizeof(float), ctx->d_rows, (size_t)ctx->model.pts_cap * HT_ROW * sizeof(float), HT_MAXPTS * HT_ROW * sizeof(float), B, hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipMemcpyAsync(nrows, ctx->d_nrows, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
	return ht_sync_check(ctx, s);
}
// cloud_chamber (physmodel.h:486-496) as HandTracker::update calls it (handtrack.h:774-778): rows [B][5*nb][16], nrows [B] (0 where the frame has no more than
// min_point_num points or boundary_planes is off)
extern "C" int ht_stage_chamber(ht_ctx *ctx, int which, int B, float *rows, int *nrows)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (!rows || !nrows || which < 0 || which > 1) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	const size_t per = (size_t)5 * ctx->model.nb * HT_ROW;
	HIPCHK(ctx, hipMemsetAsync(ctx->d_chamber, 0, (size_t)B * per * sizeof(float), s));
	ht_launch_chamber_planes(ctx->model, ctx->d_pts, ctx->d_npts, ctx->par.min_point_num, ctx->par.boundary_planes, ctx->d_chplanes, ctx->d_chon, B, s);
	ht_launch_chamber(ctx->model, ctx->d_state[which], ctx->d_chplanes, ctx->d_chon, 10.0f, ctx->d_chamber, ctx->d_nchamber, B, s);
	HIPCHK(ctx, hipMemcpyAsync(rows, ctx->d_chamber, (size_t)B * per * sizeof(float), hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipMemcpyAsync(nrows, ctx->d_nchamber, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
	return ht_sync_check(ctx, s);
}
extern "C" int ht_stage_contacts(ht_ctx *ctx, int which, int B, int cap, float *contacts, int *ncontacts)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (!contacts || !ncontacts || which < 0 || which > 1 || cap < 1) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	launch_contacts(ctx, which, nullptr, B, s);
	std::vector<float> tmp((size_t)B * HT_MAXCONTACT * HT_CONTACT);
	HIPCHK(ctx, hipMemcpyAsync(tmp.data(), ctx->d_contacts, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipMemcpyAsync(ncontacts, ctx->d_ncontacts, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
	{ const int r = ht_sync_check(ctx, s); if (r) return r; }
	const int ncopy = cap < HT_MAXCONTACT ? cap : HT_MAXCONTACT;
	for (int b = 0; b < B; b++) memcpy(contacts + (size_t)b * cap * HT_CONTACT, tmp.data() + (size_t)b * HT_MAXCONTACT * HT_CONTACT, (size_t)ncopy * HT_CONTACT * sizeof(float));
	return HT_OK;
}
extern "C" int ht_stage_fit(ht_ctx *ctx, int B)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	main_pass(ctx, B, ctx->stream);
	return ht_sync_check(ctx, ctx->stream);
}
// The stage calls that start from a decoded CNN output of the caller's: MultiStepSim, its steps [from_step, to_step) alone (handtrack.h:660-688: every step has its own
// mix of CNN-driven angular rows, landmark rays and cloud rows; teacher-forced single-step tests start a step from a given state), PoseFromScratch + UnibodyFit.
template <class F> static int stage_on_analysis(ht_ctx *ctx, const float *analysis, int B, F launch)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (!analysis) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	HIPCHK(ctx, hipMemcpyAsync(ctx->d_analysis, analysis, (size_t)B * HT_ANALYSIS * sizeof(float), hipMemcpyHostToDevice, s));
	launch(s);
	return ht_sync_check(ctx, s);
}
extern "C" int ht_stage_multistep(ht_ctx *ctx, const float *analysis, int B) { return stage_on_analysis(ctx, analysis, B, [&](hipStream_t s) { multistep(ctx, B, steps_on(s).all_frames()); }); }
extern "C" int ht_stage_multistep_range(ht_ctx *ctx, const float *analysis, int B, int from_step, int to_step)
{
	const bool range_ok = from_step >= 0 && to_step >= from_step;
	return stage_on_analysis(ctx, range_ok ? analysis : nullptr, B, [&](hipStream_t s) { multistep(ctx, B, steps_on(s).steps(from_step, to_step).all_frames()); });
}
extern "C" int ht_stage_scratch_unibody(ht_ctx *ctx, const float *analysis, int B, int n_unibody) { return stage_on_analysis(ctx, analysis, B, [&](hipStream_t s) { reset_path(ctx, false, n_unibody, B, s, s); }); }
// Tests only: the same for the frames list[0 .. nlist) alone, through the flagged-frame list as an update launches it (many_frames 0: k_reset<1>, one block per CU;
// 1: k_reset<2>) -- the listed launch without a whole update around it.  The other frames keep their state and their row counts.  Refused before anything is
// uploaded: a null pointer, nlist outside [0, B], an index outside [0, B), an index given twice.  Leaves the list empty, as an update's head does.
extern "C" int ht_stage_scratch_unibody_listed(ht_ctx *ctx, const float *analysis, int B, int n_unibody, const int *list, int nlist, int many_frames)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (!analysis || !list || nlist < 0 || nlist > B) return HT_ERR_ARG;
	std::vector<char> seen((size_t)B, 0);
	for (int i = 0; i < nlist; i++)
	{
		if (list[i] < 0 || list[i] >= B || seen[list[i]]) return HT_ERR_ARG;
		seen[list[i]] = 1;
	}
	const int organisation = ctx->last_reset_many;      // what the latest update chose stays on record (ht_debug_reset_organisation)
	const int r = stage_on_analysis(ctx, analysis, B, [&](hipStream_t s) {
		if (nlist > 0) (void)hipMemcpyAsync(ctx->d_flist, list, (size_t)nlist * sizeof(int), hipMemcpyHostToDevice, s);
		(void)hipMemcpyAsync(ctx->d_nflist, &nlist, sizeof(int), hipMemcpyHostToDevice, s);
		reset_path(ctx, true, n_unibody, B, s, s, many_frames != 0);
		(void)hipMemsetAsync(ctx->d_nflist, 0, sizeof(int), s);
	});
	ctx->last_reset_many = organisation;
	return r;
}

// Timing experiments only (HT_DEBUG_SKIP & 2048): per-frame k_solve statistics accumulated in the last scratch record of each frame:
// launches, cycles in chains / two-body linear / angular, cycles in all sweeps, steps (linear, angular), longest chain, row counts.
extern "C" int ht_debug_solve_stats(ht_ctx *ctx, int B, float *out, int reset)
{
	if (!ctx || !ctx->ready || B < 1 || B > ctx->B) return HT_ERR_ARG;
	ht_device_guard dev_guard_(ctx->device);
	const int stride = scratch_stride(ctx);
	if (ht_sync_all(ctx) != hipSuccess) return HT_ERR_HIP;
	for (int b = 0; b < B; b++)
	{
		float *src = ctx->d_scratch + ((size_t)b * stride + (stride - 1)) * HT_CREC;
		if (out && hipMemcpy(out + (size_t)b * 16, src, 16 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return HT_ERR_HIP;
		if (reset && hipMemset(src, 0, 16 * sizeof(float)) != hipSuccess) return HT_ERR_HIP;
	}
	return HT_OK;
}
// Tests only: pins the build of k_solve (0 = the launcher's choice by batch and frame size; 1 small, 2 only, 3 mid, 4 tiny = a build whose LDS arrays hold
// nothing, so that every frame takes the HBM placement of its two-body groups, impulse sums and angular records).  The builds differ in where a
// frame's arrays live, never in arithmetic: results must agree bit for bit (tests/test_gpu_solver.py).
// 5 = the EXACT-ORDER instantiation: the same rows, swept by the reference's own Iter functions in the reference's row order (physics.h:251-265, 289-307, 556-581) on one
// lane per frame, the single-body solves of UnibodyFit too.  With it an update equals the CPU restatement bit for bit (tests/test_gpu_exact_solver.py), which
// pins the Jacobian-form arithmetic of the product's sweeps as the solver's only difference from the reference.  Far slower; never chosen by a launcher.
extern "C" int ht_debug_solver_build(ht_ctx *ctx, int which)
{
	if (!ctx || which < 0 || which > 8) return HT_ERR_ARG;      // 6: the build with four angular-row slots per lane (up to 252 rows), otherwise chosen by the model's joint count; 7: the launcher's choice of build, with the two-body rows of EVERY frame taken by the level schedule (round 4's sweeps; otherwise only frames the blocked form of round 5 does not hold): another rounding of the same sweeps
	if ((which == 5 || which == 8) && !ctx->d_exact_lin)
	{
		ht_device_guard dev_guard_(ctx->device);
		int r;
		if ((r = dev_alloc(ctx, &ctx->d_exact_ang, (size_t)ctx->B * 256 * 8)) || (r = dev_alloc(ctx, &ctx->d_exact_lin, (size_t)ctx->B * HT_EX_LIN * HT_ROW))) return r;
	}
	ctx->solver_build = which;
	return HT_OK;
}
// Tests only: how the edges between an update's streams are made.  0 = the product's choice (ht_host.hpp: ht_edge_event; fork / join1 above); 1 = as up to round 29: events
// with hipEventDisableTiming alone, every edge a hipEventRecord and a hipStreamWaitEvent.  Waits for the context's work and makes its events anew, so that a test can run
// both paths in one process; the results must be the same bits (tests/test_gpu_stream_edges.py).
extern "C" int ht_debug_stream_edges(ht_ctx *ctx, int mode)
{
	if (!ctx || mode < 0 || mode > 1) return HT_ERR_ARG;
	ht_device_guard dev_guard_(ctx->device);
	HIPCHK(ctx, ht_sync_all(ctx));
	for (int i = 0; i < 2; i++) HIPCHK(ctx, hipStreamSynchronize(ctx->side[i]));
	ctx->edge_mode = mode;
	hipEvent_t *ev[] = { &ctx->ev_fork, &ctx->ev_join[0], &ctx->ev_join[1], &ctx->ev_lap };
	for (hipEvent_t *e : ev) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; HIPCHK(ctx, ht_edge_event(ctx, e)); }
	if (ctx->ev_seed && !ctx->job_pending) { (void)hipEventDestroy(ctx->ev_seed); ctx->ev_seed = nullptr; }      // made again by the next ht_job_start
	return HT_OK;
}
// Tests only: which organisation the latest update launched the full-reset branch in (0 = few frames: one k_reset block per CU, a contact block per reset frame;
// 1 = many frames: two blocks per CU, four frames per contact block; -1 = no update yet).  The choice follows the count of reset frames of earlier updates.
extern "C" int ht_debug_reset_organisation(ht_ctx *ctx, int *many)
{
	if (!ctx || !many) return HT_ERR_ARG;
	*many = ctx->last_reset_many;
	return HT_OK;
}
// Tests only: which frames of the latest update took the full-reset branch (handtrack.h:706-711): flags[i] = 1 for tracker slot i (the decision kernel's own array)
extern "C" int ht_debug_reset_flags(ht_ctx *ctx, int *flags, int n)
{
	if (!ctx || !flags || n < 0 || n > ctx->B) return HT_ERR_ARG;
	ht_device_guard dev_guard_(ctx->device);
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	HIPCHK(ctx, hipMemcpy(flags, ctx->d_flags, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
	return HT_OK;
}
// Tests only: the cloud-row counts of slots [0, B) as the latest launch that wrote them left them (the cloud-row kernels, k_reset)
extern "C" int ht_debug_row_counts(ht_ctx *ctx, int B, int *nrows)
{
	CHECK_READY(ctx); CHECK_BATCH(ctx, B);
	if (!nrows) return HT_ERR_ARG;
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	HIPCHK(ctx, hipMemcpy(nrows, ctx->d_nrows, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
	return HT_OK;
}
// Tests only: pins the organisation of the contact kernel (0 = the launcher's choice; 1 cooperative, 2 lane-per-pair).  Same arithmetic, same contacts in the same order.
extern "C" int ht_debug_contact_kernel(ht_ctx *ctx, int which)
{
	if (!ctx || which < 0 || which > 2) return HT_ERR_ARG;
	ctx->contact_kernel = which;
	return HT_OK;
}
// Tests only: which kernel a contact launch on B frames takes under the current pin, from the launcher's own functions: the cooperative kernel's frames per block
// (0 = not taken, e.g. because a frame of the model does not fit its LDS) and the lane-per-pair kernel's waves per frame (0 = not taken; 2 = k_contacts<2>).
extern "C" int ht_debug_contact_plan(ht_ctx *ctx, int B, int *coop_frames, int *lane_waves)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	const bool coop = ht_contacts_coop(ctx->model, B, ctx->contact_kernel, false);
	if (coop_frames) *coop_frames = coop ? ht_contacts_coop_plan(ctx->model, B).nfr : 0;
	if (lane_waves) *lane_waves = coop ? 0 : ht_contacts_lane_waves(ctx->model);
	return HT_OK;
}
// Tests only: the launch tables of one slot from a work array the caller gives.  The product's launchers on the context's stream, over buffers of the call's own
// (stride as the context lays its histories out: B + 8), preset to -1 so that a place no block wrote shows.
//   ht_debug_contact_order: order_out[ceil(B / nfr) * nfr] = k_contact_order's table (order_out[round * blocks + block] = frame, B = no frame); 1 <= nfr <= 8, epb >= 1
//   ht_debug_rank_desc:     order_out[B] = k_rank_desc's
template <class F> static int debug_order_table(ht_ctx *ctx, const int *work, int B, int n_out, int *order_out, F launch)      // launch(work, order, stride, stream)
{
	const int stride = ht_history::stride_for(B);
	int *d = nullptr;
	HIPCHK(ctx, hipMalloc(&d, (size_t)2 * stride * sizeof(int)));
	hipStream_t s = ctx->stream;
	hipError_t e = hipMemcpyAsync(d, work, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s);
	if (e == hipSuccess) e = hipMemsetAsync(d + stride, 0xff, (size_t)stride * sizeof(int), s);
	if (e == hipSuccess) { launch(d, d + stride, stride, s); e = hipGetLastError(); }
	if (e == hipSuccess) e = hipMemcpyAsync(order_out, d + stride, (size_t)n_out * sizeof(int), hipMemcpyDeviceToHost, s);
	if (e == hipSuccess) e = hipStreamSynchronize(s); else (void)hipStreamSynchronize(s);
	(void)hipFree(d);
	HIPCHK(ctx, e);
	return HT_OK;
}
extern "C" int ht_debug_contact_order(ht_ctx *ctx, const int *work, int B, int nfr, int epb, int *order_out)
{
	CHECK_READY(ctx);
	if (!work || !order_out || B < 1 || nfr < 1 || nfr > 8 || epb < 1) return HT_ERR_ARG;
	return debug_order_table(ctx, work, B, (B + nfr - 1) / nfr * nfr, order_out, [&](const int *w, int *o, int stride, hipStream_t s) { ht_launch_contact_order(w, o, B, nfr, stride, 1u, 1, epb, s); });
}
extern "C" int ht_debug_rank_desc(ht_ctx *ctx, const int *work, int B, int *order_out)
{
	CHECK_READY(ctx);
	if (!work || !order_out || B < 1) return HT_ERR_ARG;
	return debug_order_table(ctx, work, B, B, order_out, [&](const int *w, int *o, int stride, hipStream_t s) { ht_launch_rank_desc(w, o, B, stride, 1u, 1, s); });
}
extern "C" int ht_debug_solve_tables(ht_ctx *ctx, int on)
{
	if (!ctx || !ctx->ready) return HT_ERR_ARG;
	ht_device_guard dev_guard_(ctx->device);
	if (on < 0 || on > 2) return HT_ERR_ARG;
	if (on) { const int r = ht_alloc_solve_tables(ctx); if (r) return r; }
	ctx->solve_tables = on;
	return HT_OK;
}
extern "C" int ht_debug_solve_tables_header(ht_ctx *ctx, int B, int *hdr)
{
	if (!ctx || !ctx->ready || !hdr || B < 1 || B > ctx->B || !ctx->d_tables) return HT_ERR_ARG;
	ht_device_guard dev_guard_(ctx->device);
	if (ht_sync_all(ctx) != hipSuccess) return HT_ERR_HIP;
	if (hipMemcpy2D(hdr, 32 * sizeof(int), ctx->d_tables, (size_t)TB_WORDS * sizeof(float), 32 * sizeof(int), B, hipMemcpyDeviceToHost) != hipSuccess) return HT_ERR_HIP;
	return HT_OK;
}
// Same for k_contacts (last contact slot of each frame): launches, cycles in GJK / polytope runs, polytope runs, polytope cycles in
// face scoring / support scans / mesh surgery, total cycles, candidate pairs, pairs that jiggle, contacts, polytope iterations.
extern "C" int ht_debug_contact_stats(ht_ctx *ctx, int B, float *out, int reset)
{
	if (!ctx || !ctx->ready || B < 1 || B > ctx->B) return HT_ERR_ARG;
	ht_device_guard dev_guard_(ctx->device);
	if (hipDeviceSynchronize() != hipSuccess) return HT_ERR_HIP;
	for (int b = 0; b < B; b++)
	{
		float *src = ctx->d_contacts + ((size_t)b * HT_MAXCONTACT + HT_MAXCONTACT - 2) * HT_CONTACT;      // the last two contact slots: [1] the frame's record, [0] its wave's polytope runs
		if (out && hipMemcpy(out + (size_t)b * 24, src, 24 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return HT_ERR_HIP;
		if (reset && hipMemset(src, 0, 24 * sizeof(float)) != hipSuccess) return HT_ERR_HIP;
	}
	return HT_OK;
}

// ------------------------------------------------------------------------------------------------- segmentation (before the tracker)
// One implementation for both forms: `sized` = the *_sized entry points (either tile side, frames up to 640x480), otherwise the unsized ones with their own limit and message.
static int segment_dev(ht_ctx *ctx, bool sized, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, int entry_options, float wrange_hi, float diam,
                       uint16_t *d_tiles, float *d_cams_out, void *stream)
{
	if (!d_depth || !d_cams || !d_tiles || !d_cams_out || B < 1) return HT_ERR_ARG;
	if (side != 64 && side != 128) { ctx->err = "ht_segment_vr_sized: the tile side must be 64 or 128"; return HT_ERR_ARG; }
	hipStream_t s = ht_user_stream(ctx, stream);
	if (w == side && h == side)      // handtrack.h:283-284: a frame of the net's own size is returned as it is
	{
		HIPCHK(ctx, hipMemcpyAsync(d_tiles, d_depth, (size_t)B * side * side * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
		HIPCHK(ctx, hipMemcpyAsync(d_cams_out, d_cams, (size_t)B * HT_CAM * sizeof(float), hipMemcpyDeviceToDevice, s));
		return HT_OK;
	}
	if (!sized && !ht_segment_supported(w, h)) { ctx->err = "ht_segment_vr: frame size must be a multiple of 4 and at most 320x240 pixels"; return HT_ERR_ARG; }
	if (sized && !ht_segment_supported_sized(w, h, side)) { ctx->err = "ht_segment_vr_sized: frame size must be a multiple of 4, at least 8x8 and at most 640x480 pixels (19200 quarter-size pixels)"; return HT_ERR_ARG; }
	ht_launch_segment(d_depth, d_cams, w, h, entry_options, wrange_hi, diam, d_tiles, d_cams_out, B, s, side);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
static int segment_host(ht_ctx *ctx, bool sized, int side, const uint16_t *depth, const float *cams, int w, int h, int B, int entry_options, float wrange_hi, float diam, uint16_t *tiles, float *cams_out)
{
	if (!depth || !cams || !tiles || !cams_out || B < 1 || w < 1 || h < 1) return HT_ERR_ARG;
	if (sized && !(w == side && h == side) && !ht_segment_supported_sized(w, h, side)) return segment_dev(ctx, true, side, depth, cams, w, h, B, entry_options, wrange_hi, diam, tiles, cams_out, nullptr);      // refused before the staging buffer grows
	const size_t n = (size_t)B;      // staged through the context's buffer (ht_staged_call; no tracker slot: B is not bounded by max_batch)
	ht_seg seg[4] = { { (void *)depth, n * w * h * sizeof(uint16_t), false }, { (void *)cams, n * HT_CAM * sizeof(float), false }, { tiles, n * side * side * sizeof(uint16_t), true }, { cams_out, n * HT_CAM * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 4, [&](hipStream_t s)
	                      { return segment_dev(ctx, sized, side, (const uint16_t *)seg[0].dev, (const float *)seg[1].dev, w, h, B, entry_options, wrange_hi, diam, (uint16_t *)seg[2].dev, (float *)seg[3].dev, s); });
}
extern "C" int ht_segment_vr_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, int entry_options, float wrange_lo, float wrange_hi, float diam,
                                 uint16_t *d_tiles, float *d_cams_out, void *stream)
{
	CHECK_READY(ctx);
	(void)wrange_lo;      // the reference's lower bound is commented out (handtrack.h:288)
	return segment_dev(ctx, false, 64, d_depth, d_cams, w, h, B, entry_options, wrange_hi, diam, d_tiles, d_cams_out, stream);
}
extern "C" int ht_segment_vr(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, int B, int entry_options, float wrange_lo, float wrange_hi, float diam,
                             uint16_t *tiles, float *cams_out)
{
	CHECK_READY(ctx);
	(void)wrange_lo;
	return segment_host(ctx, false, 64, depth, cams, w, h, B, entry_options, wrange_hi, diam, tiles, cams_out);
}
// HandSegmentVR (handtrack.h:280-344) with the tile side of dstcam (:338-340) a parameter, on frames up to 640x480: the one place the size rule lives
extern "C" int ht_segment_vr_supported(int w, int h, int side) { return ht_segment_supported_sized(w, h, side) || ((side == 64 || side == 128) && w == side && h == side) ? HT_OK : HT_ERR_ARG; }
extern "C" int ht_segment_vr_sized_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, int entry_options, float wrange_lo, float wrange_hi, float diam,
                                       uint16_t *d_tiles, float *d_cams_out, void *stream)
{
	CHECK_READY(ctx);
	(void)wrange_lo;
	return segment_dev(ctx, true, side, d_depth, d_cams, w, h, B, entry_options, wrange_hi, diam, d_tiles, d_cams_out, stream);
}
extern "C" int ht_segment_vr_sized(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, int B, int entry_options, float wrange_lo, float wrange_hi, float diam,
                                   uint16_t *tiles, float *cams_out)
{
	CHECK_READY(ctx);
	(void)wrange_lo;
	if (side != 64 && side != 128) { ctx->err = "ht_segment_vr_sized: the tile side must be 64 or 128"; return HT_ERR_ARG; }
	return segment_host(ctx, true, side, depth, cams, w, h, B, entry_options, wrange_hi, diam, tiles, cams_out);
}

// ------------------------------------------------------------------------------------------------- caller-built constraint rows
// PhysModel::FitPointCloud(points, linears, angulars, microforce) (physmodel.h:345-356) and the free PhysicsUpdate(bodies, Linears, Angulars, wgeom)
// (physics.h:543-587) take rows the CALLER built.  Row layouts are those of the stage calls: a linear row is 16 floats (rb0 rb1 position0[3]
// position1[3] normal[3] targetdist targetspeednobias forcelimit.x forcelimit.y friction_master), an angular row 8 (rb0 rb1 axis[3] targetspin
// mintorque maxtorque); a body is its index in PhysModel::rigidbodies, -1 = NULL.
int ht_user_rows_reserve(ht_ctx *ctx, int lin_cap, int ang_cap)
{
	const size_t B = (size_t)ctx->B;
	int r, pos_cap = ctx->user_lin_cap;      // the two arrays of the linear rows share a capacity: it is raised by the second to grow
	if ((r = dev_grow(ctx, &ctx->d_user_pos, &pos_cap, lin_cap, B)) || (r = dev_grow(ctx, &ctx->d_user_lin, &ctx->user_lin_cap, lin_cap, B * HT_ROW))) return r;
	if ((r = dev_grow(ctx, &ctx->d_user_ang, &ctx->user_ang_cap, ang_cap, B * HT_AROW))) return r;
	return ctx->d_user_n ? HT_OK : dev_alloc(ctx, &ctx->d_user_n, 4 * B);
}
static int upload_angulars(ht_ctx *ctx, int B, const float *angulars, int acap, const int *nangulars, std::vector<int> &na)
{
	na.assign(B, 0);
	for (int b = 0; b < B; b++)
	{
		na[b] = (angulars && nangulars) ? nangulars[b] : 0;
		if (na[b] < 0 || na[b] > acap || na[b] > 126 || 13 + 6 * ctx->model.nj + na[b] > 252) { ctx->err = "caller-built angular rows: a count is negative, exceeds the stride, exceeds 126 or leaves no room for the model's own rows among the 252 angular rows a solve keeps"; return HT_ERR_ARG; }
		for (int i = 0; i < na[b]; i++) { const float *r = angulars + ((size_t)b * acap + i) * HT_AROW; if ((int)r[0] >= ctx->model.nb || (int)r[1] >= ctx->model.nb) { ctx->err = "caller-built angular rows: body index out of range"; return HT_ERR_ARG; } }
	}
	if (acap > 0 && angulars) HIPCHK(ctx, hipMemcpy2D(ctx->d_user_ang, (size_t)ctx->user_ang_cap * HT_AROW * sizeof(float), angulars, (size_t)acap * HT_AROW * sizeof(float), (size_t)acap * HT_AROW * sizeof(float), B, hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(ctx->d_user_n + 3 * (size_t)ctx->B, na.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
	return HT_OK;
}
// the solve of ht_fit_rows / ht_physics_update / ht_fit_keypoints: the caller's angular rows (upload_angulars; ang_bound: the largest count of a frame) join
static void enqueue_caller_rows(ht_ctx *ctx, solve_args &a, int ang_bound, int B, hipStream_t s)
{
	a.ang_user = ctx->d_user_ang; a.n_ang_user = ctx->d_user_n + 3 * (size_t)ctx->B; a.ang_user_stride = ctx->user_ang_cap;
	a.ang_extra_bound = ang_bound;
	a.force_build = ctx->solver_build;
	ctx->model.pts_bound = 0;
	ht_launch_solve(ctx->model, ctx->phys, a, B, s);
}
// ... then the stream is waited for
static int solve_caller_rows(ht_ctx *ctx, solve_args &a, const std::vector<int> &na, int B, hipStream_t s)
{
	int mx = 0; for (int v : na) mx = v > mx ? v : mx;
	enqueue_caller_rows(ctx, a, mx, B, s);
	return ht_sync_check(ctx, s);
}
// One FitPointCloud step on what the context's buffers hold (ht_fit_rows' launch sequence; ht_fit_keypoints runs it once per step with rows its kernel wrote): the cloud
// rows of the prepared points, the contacts if physics_use_collision, and k_solve with the caller's linear rows (d_user_lin / d_user_n) ahead of them.  k_solve brings the
// joint ranges up to date itself.  Enqueued on s, not waited for
void ht_fit_rows_enqueue(ht_ctx *ctx, int which, int B, float microforce, int ang_bound, int zero_momenta, hipStream_t s)
{
	const bool coll = ctx->phys.use_collision != 0;
	cloud_limits lim = ht_cloud_limits(ctx->par, CLOUD_FIT); lim.microforce = microforce;
	const cloud_records cr = cloud_rec(ctx);
	ht_launch_cloud_rows(ctx->model, ctx->d_state[which], ctx->d_pts, ctx->d_npts, ctx->d_cams, nullptr, fit_take(CLOUD_FIT), lim, ctx->d_rows, ctx->d_nrows, B, s, &cr);
	if (coll) launch_contacts(ctx, which, nullptr, B, s);
	solve_args a = solve_head(ctx, which, coll);
	a.rows_pre = ctx->d_user_lin; a.n_pre = ctx->d_user_n; a.pre_stride = ctx->user_lin_cap;
	a.cloud_body = ctx->d_rowbody; a.n_cloud = ctx->d_nrows;
	a.zero_momenta = zero_momenta;
	enqueue_caller_rows(ctx, a, ang_bound, B, s);
}
// ht_fit_views (ht_views.hip): `passes` times the sequence above on the slots' fused cloud, with the cloud-row launch that takes every point's ray from its own origin
// and without caller rows or boundary planes; the momenta are kept from pass to pass as in update()'s main passes, and the last solve writes the user poses (d_poses may
// be null).  All on s, nothing copied or waited for between the passes
int ht_fit_views_enqueue(ht_ctx *ctx, int which, int B, int passes, float *d_poses, hipStream_t s)
{
	const bool coll = ctx->phys.use_collision != 0;
	const cloud_records cr = cloud_rec(ctx);
	for (int pass = 0; pass < passes; pass++)
	{
		ht_launch_cloud_rows_views(ctx->model, ctx->d_state[which], ctx->d_pts, ctx->d_npts, ctx->d_view_origins, ht_cloud_limits(ctx->par, CLOUD_FIT), ctx->d_rows, ctx->d_nrows, B, s, &cr);
		if (coll) launch_contacts(ctx, which, nullptr, B, s);
		solve_args a = solve_head(ctx, which, coll);
		a.cloud_body = ctx->d_rowbody; a.n_cloud = ctx->d_nrows;
		a.force_build = ctx->solver_build;
		if (d_poses && pass + 1 == passes) { a.out_poses = d_poses; a.out_npts = ctx->d_npts; a.out_initializing = ctx->d_initializing; a.out_min_point_num = 0; }      // (no point count is below 0: the tracker's flags are not touched)
		ctx->model.pts_bound = 0;
		ht_launch_solve(ctx->model, ctx->phys, a, B, s);
	}
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
// void PhysModel::FitPointCloud(const std::vector<float3> &points, std::vector<LimitLinear> linears, std::vector<LimitAngular> angulars, float microforce)
// on model `which` of slots [0,B): the caller's linear rows, then CloudConstraints(points) with the +-microforce limits (x physics_weak_force on
// bodies 0-2), then the joints' nailed rows; the caller's angular rows, then the joints' range rows; PhysicsUpdate with collision; SanityCheck.  As
// at every call site of the reference (handtrack.h:672-685, 773-779, 803-819) the joint ranges are first brought up to date from the pose
// (HandModelEnhancements, :417-420, 434-440).  The caller's linear rows must be anchored in the world (rb0 == NULL), as the rows of every such call
// site are (landmark rays, boundary planes, the annotator's nail): they join the per-body row chains ahead of the cloud rows.
extern "C" int ht_fit_rows(ht_ctx *ctx, int which, int B, const float *points, int pcap, const int *npoints, const float *linears, int lcap, const int *nlinears,
                           const float *angulars, int acap, const int *nangulars, float microforce)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (which < 0 || which > 1 || pcap < 0 || lcap < 0 || acap < 0) return HT_ERR_ARG;
	const int nb = ctx->model.nb;
	std::vector<int> nl(B, 0), na;
	for (int b = 0; b < B; b++)
	{
		nl[b] = (linears && nlinears) ? nlinears[b] : 0;
		if (nl[b] < 0 || nl[b] > lcap || nl[b] > 5 * nb + 128) { ctx->err = "ht_fit_rows: a linear row count is negative, exceeds the stride or exceeds the 5 * bodies + 128 caller rows a frame's scratch slot holds"; return HT_ERR_ARG; }
		for (int i = 0; i < nl[b]; i++)
		{
			const float *r = linears + ((size_t)b * lcap + i) * HT_ROW;
			if ((int)r[0] >= 0 || (int)r[1] < 0 || (int)r[1] >= nb || r[15] != 0.0f) { ctx->err = "ht_fit_rows: the caller's linear rows must act on one body from the world (rb0 == NULL, no friction master); use ht_physics_update for general rows"; return HT_ERR_ARG; }
		}
	}
	REFUSE_EXACT_SOLVER(ctx);
	{ const int r = ht_user_rows_reserve(ctx, lcap > 1 ? lcap : 1, acap > 1 ? acap : 1); if (r) return r; }
	{ const int r = upload_angulars(ctx, B, angulars, acap, nangulars, na); if (r) return r; }
	// the points (ht_set_points grows the point capacity when it has to)
	{
		static const float none[3] = { 0, 0, 0 }; std::vector<int> zero(B, 0);
		const int r = (points && npoints && pcap > 0) ? ht_set_points(ctx, B, points, pcap, npoints) : ht_set_points(ctx, 1, none, 1, zero.data());
		if (r) return r;
		if (!(points && npoints && pcap > 0)) HIPCHK(ctx, hipMemset(ctx->d_npts, 0, (size_t)B * sizeof(int)));
	}
	if (lcap > 0 && linears) HIPCHK(ctx, hipMemcpy2D(ctx->d_user_lin, (size_t)ctx->user_lin_cap * HT_ROW * sizeof(float), linears, (size_t)lcap * HT_ROW * sizeof(float), (size_t)lcap * HT_ROW * sizeof(float), B, hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(ctx->d_user_n, nl.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
	int most_ang = 0; for (int v : na) most_ang = v > most_ang ? v : most_ang;
	ht_fit_rows_enqueue(ctx, which, B, microforce, most_ang, 0, ctx->stream);
	return ht_sync_check(ctx, ctx->stream);
}
// void PhysicsUpdate(const std::vector<RigidBody*> &rigidbodies, std::vector<LimitLinear> &Linears, std::vector<LimitAngular> &Angulars, wgeom = {})
// (physics.h:543-587) on model `which` of slots [0,B): the caller's rows are all there is (plus the collision rows when physics_use_collision is set).
// Rows keep the caller's order: the leading rows that act on one body from the world (rb0 == NULL) run as per-body chains, the rest in groups of up
// to three consecutive rows on the same body pair; a friction row (friction_master -1 / -2) must follow its master directly, as ConstrainContacts
// builds them (physics.h:463-489).  At most 32 such groups per frame.
extern "C" int ht_physics_update(ht_ctx *ctx, int which, int B, const float *linears, int lcap, const int *nlinears, const float *angulars, int acap, const int *nangulars)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (which < 0 || which > 1 || lcap < 0 || acap < 0) return HT_ERR_ARG;
	const int nb = ctx->model.nb;
	std::vector<int> npre(B, 0), ntail(B, 0), ngrp(B, 0), na;
	std::vector<unsigned short> pos((size_t)B * (lcap > 1 ? lcap : 1), 0);
	int most_pre = 0;
	for (int b = 0; b < B; b++)
	{
		const int n = (linears && nlinears) ? nlinears[b] : 0;
		if (n < 0 || n > lcap) { ctx->err = "ht_physics_update: a linear row count is negative or exceeds the stride"; return HT_ERR_ARG; }
		const float *rows = linears + (size_t)b * lcap * HT_ROW;
		for (int i = 0; i < n; i++) if ((int)rows[i * HT_ROW] >= nb || (int)rows[i * HT_ROW + 1] >= nb || ((int)rows[i * HT_ROW] < 0 && (int)rows[i * HT_ROW + 1] < 0)) { ctx->err = "ht_physics_update: body index out of range"; return HT_ERR_ARG; }
		int p = 0;
		while (p < n && (int)rows[p * HT_ROW] < 0 && rows[p * HT_ROW + 15] == 0.0f && !(p + 1 < n && rows[(p + 1) * HT_ROW + 15] != 0.0f)) p++;
		npre[b] = p; ntail[b] = n - p; if (p > most_pre) most_pre = p;
		// groups of the tail: up to three consecutive rows on one body pair; a row that friction rows follow opens a group
		int g = -1, slot = 3, g0 = 0; int pa = -2, pb = -2;
		for (int i = p; i < n; i++)
		{
			const float *r = rows + (size_t)i * HT_ROW;
			const int fm = (int)r[15], ra = (int)r[0], rb = (int)r[1];
			const bool next_is_friction = i + 1 < n && rows[(size_t)(i + 1) * HT_ROW + 15] != 0.0f && fm == 0;
			if (fm != 0)
			{
				if (g < 0 || -fm != slot || slot > 2 || ra != pa || rb != pb) { ctx->err = "ht_physics_update: a friction row must directly follow its master row (friction_master -1, then -2) on the same bodies"; return HT_ERR_ARG; }
				for (int k = g0; k <= i; k++) pos[(size_t)b * lcap + (k - p)] |= 0x8000;
			}
			else if (g < 0 || slot > 2 || ra != pa || rb != pb || next_is_friction || (pos[(size_t)b * lcap + (g0 - p)] & 0x8000)) { g++; slot = 0; g0 = i; pa = ra; pb = rb; }
			pos[(size_t)b * lcap + (i - p)] |= (unsigned short)((g << 2) | slot);
			slot++;
		}
		ngrp[b] = g + 1;
		if (ngrp[b] > HT_MAXNJ) { ctx->err = "ht_physics_update: more than 32 groups of two-body rows in a frame"; return HT_ERR_ARG; }
	}
	REFUSE_EXACT_SOLVER(ctx);
	if (most_pre > ctx->model.pts_cap) { const int r = ht_reserve_points_locked(ctx, most_pre); if (r) return r; }
	{ const int r = ht_user_rows_reserve(ctx, lcap > 1 ? lcap : 1, acap > 1 ? acap : 1); if (r) return r; }
	{ const int r = upload_angulars(ctx, B, angulars, acap, nangulars, na); if (r) return r; }
	const size_t pc = (size_t)ctx->model.pts_cap;
	for (int b = 0; b < B; b++)
	{
		const float *rows = linears ? linears + (size_t)b * lcap * HT_ROW : nullptr;
		if (npre[b]) HIPCHK(ctx, hipMemcpy(ctx->d_rows + (size_t)b * pc * HT_ROW, rows, (size_t)npre[b] * HT_ROW * sizeof(float), hipMemcpyHostToDevice));
		if (ntail[b])
		{
			HIPCHK(ctx, hipMemcpy(ctx->d_user_lin + (size_t)b * ctx->user_lin_cap * HT_ROW, rows + (size_t)npre[b] * HT_ROW, (size_t)ntail[b] * HT_ROW * sizeof(float), hipMemcpyHostToDevice));
			HIPCHK(ctx, hipMemcpy(ctx->d_user_pos + (size_t)b * ctx->user_lin_cap, pos.data() + (size_t)b * lcap, (size_t)ntail[b] * sizeof(unsigned short), hipMemcpyHostToDevice));
		}
	}
	HIPCHK(ctx, hipMemcpy(ctx->d_nrows, npre.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(ctx->d_user_n + (size_t)ctx->B, ntail.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(ctx->d_user_n + 2 * (size_t)ctx->B, ngrp.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
	hipStream_t s = ctx->stream;
	const bool coll = ctx->phys.use_collision != 0;
	if (coll) launch_contacts(ctx, which, nullptr, B, s);
	solve_args a = solve_head(ctx, which, coll);
	a.rows_cloud = ctx->d_rows; a.n_cloud = ctx->d_nrows;
	a.lin_tail = ctx->d_user_lin; a.n_lin_tail = ctx->d_user_n + (size_t)ctx->B; a.lin_tail_stride = ctx->user_lin_cap;
	a.lin_tail_pos = ctx->d_user_pos; a.n_tail_groups = ctx->d_user_n + 2 * (size_t)ctx->B;
	a.no_model_rows = 1;
	return solve_caller_rows(ctx, a, na, B, s);
}

// ------------------------------------------------------------------------------------------------- slowfit (annotation fit loop)
// HandTracker::slowfit (handtrack.h:786-821) on the handmodel of slots [0,B) against the points ht_stage_prepare left on the device.
extern "C" int ht_slowfit(ht_ctx *ctx, int B, int hold, const float *refpose, int steps, int select_rb, const float *spoint, const float *rbpoint, const float *crays, int ncray)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	const int nb = ctx->model.nb;
	if (steps < 1 || ncray < 0 || ncray > 8 || select_rb >= nb || (select_rb >= 0 && (!spoint || !rbpoint)) || (ncray > 0 && !crays)) { ctx->err = "ht_slowfit: bad arguments"; return HT_ERR_ARG; }
	REFUSE_EXACT_SOLVER(ctx);
	hipStream_t s = ctx->stream;
	if (!ctx->d_sf_ref)
	{
		int r;
		if ((r = dev_alloc(ctx, &ctx->d_sf_crays, (size_t)ctx->B * 8 * 4)) || (r = dev_alloc(ctx, &ctx->d_sf_ref, (size_t)ctx->B * nb * HT_POSE))) return r;
	}
	const bool rel = hold && refpose;
	if (rel) HIPCHK(ctx, hipMemcpyAsync(ctx->d_sf_ref, refpose, (size_t)B * nb * HT_POSE * sizeof(float), hipMemcpyHostToDevice, s));
	if (ncray) HIPCHK(ctx, hipMemcpyAsync(ctx->d_sf_crays, crays, (size_t)B * 8 * 4 * sizeof(float), hipMemcpyHostToDevice, s));
	const bool coll = ctx->phys.use_collision != 0;
	for (int st = 0; st < steps; st++)
	{
		const bool cloud = st < steps - 1;
		const cloud_records cr = cloud_rec(ctx);
		const cloud_limits lim = ht_cloud_limits(ctx->par, CLOUD_SLOWFIT, 1.0f * (float)(steps - st) / (float)steps, 0.1f * (float)(st < steps - 2));
		if (cloud) ht_launch_cloud_rows(ctx->model, ctx->d_state[0], ctx->d_pts, ctx->d_npts, ctx->d_cams, nullptr, fit_take(CLOUD_SLOWFIT), lim, ctx->d_rows, ctx->d_nrows, B, s, &cr);
		if (coll) launch_contacts(ctx, 0, nullptr, B, s);
		solve_args a = solve_head(ctx, 0, coll);
		a.cloud_body = cloud ? ctx->d_rowbody : nullptr; a.n_cloud = ctx->d_nrows;
		a.sf_ncray = st < 5 ? ncray : 0; a.sf_crays = ctx->d_sf_crays; a.sf_select = select_rb;
		for (int i = 0; i < 3; i++) { a.sf_spoint[i] = spoint ? spoint[i] : 0.0f; a.sf_rbpoint[i] = rbpoint ? rbpoint[i] : 0.0f; }
		a.ray_rows = (a.sf_ncray > 0 || select_rb >= 0) ? 1 : 0;
		a.sf_refpose = rel ? ctx->d_sf_ref : nullptr; a.sf_hold = rel ? hold : 0;
		a.ang_extra_bound = rel ? 3 * ctx->model.nj : 0;      // RelativeAngularConstraints: one row per ranged axis of a joint at most
		a.steps_keyangles = ctx->par.steps_keyangles; a.min_cray_prob = ctx->par.min_cray_prob;
		a.force_build = ctx->solver_build;
		ht_launch_solve(ctx->model, ctx->phys, a, B, s);
	}
	return ht_sync_check(ctx, s);
}

// Caller-supplied point clouds for the stage functions / ht_slowfit (the reference's slowfit takes its points as an argument):
// points [B][cap][3], npoints [B] (<= cap; the context's point capacity grows to the largest).
extern "C" int ht_set_points(ht_ctx *ctx, int B, const float *points, int cap, const int *npoints)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (!points || !npoints || cap < 1) return HT_ERR_ARG;
	ctx->model.pts_bound = 0;
	{ int most = 0; for (int b = 0; b < B; b++) most = std::max(most, std::min(npoints[b], cap)); if (most > HT_POINTS_LIMIT) return HT_ERR_ARG; const int r = ht_reserve_points_locked(ctx, std::max(most, 1)); if (r) return r; }
	const size_t pc = (size_t)ctx->model.pts_cap;
	std::vector<float4> h((size_t)B * pc, make_float4(0, 0, 0, 0)); std::vector<int> n(B);
	for (int b = 0; b < B; b++)
	{
		n[b] = npoints[b] < 0 ? 0 : npoints[b] > cap ? cap : npoints[b]; if (n[b] > (int)pc) n[b] = (int)pc;
		for (int i = 0; i < n[b]; i++) { const float *p = points + ((size_t)b * cap + i) * 3; h[(size_t)b * pc + i] = make_float4(p[0], p[1], p[2], 0.0f); }
	}
	HIPCHK(ctx, hipMemcpy(ctx->d_pts, h.data(), h.size() * sizeof(float4), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(ctx->d_npts, n.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
	return HT_OK;
}
