// ht_host.hpp -- host-side context behind the C-ABI (product code).
#pragma once
#include <map>
#include <string>
#include <vector>
#include "ht_device.hpp"
#include "ht_launch.hpp"
#include "ht_model_build.hpp"

struct ht_comm_state;      // RCCL communicator + communication stream (ht_comm.hip)
struct ht_prof_entry { std::vector<hipEvent_t> ev; size_t used; float total_ms; int launches; };

// A work history: what every frame took in each launch slot (HT_CONTACT_SLOTS) of the latest update, and the launch tables the current update made from it at its head.
// Both [HT_CONTACT_SLOTS][stride].  Contact launches keep one (work: k_contacts_coop, tables: k_contact_order) and the solves of a batch of several rounds per CU another
// (k_solve's cost, k_rank_desc); which launches take part is their users' rule (ht_solver_api.hip: launch_contacts, solve_step).
struct ht_history
{
	int *work = nullptr, *order = nullptr; int stride = 0, B = 0; unsigned written = 0, published = 0;      // the slots whose work the latest update wrote, for B frames; the slots whose table the current update may use
	struct rows { int *work; const int *order; };
	static int stride_for(int B) { return B + 8; }
	// The head of an update of B_ frames.  `on`: this update's launches take tables; rank(slots) then makes them, when the latest update wrote any for the same B_
	template <class F> void begin(int B_, bool on, F rank)
	{
		published = 0;
		if (on && work && stride_for(B_) <= stride && B == B_ && written) { rank(written); published = written; }
		written = 0; B = B_;
	}
	// A launch of B_ frames in `slot`: where it leaves its work, and its table if the head of the update published one.  Neither for a slot out of range or another B_
	rows take(int slot, int B_)
	{
		if (slot < 0 || slot >= HT_CONTACT_SLOTS || !work || B_ != B) return rows{ nullptr, nullptr };
		written |= 1u << slot;
		return rows{ work + (size_t)slot * stride, (published >> slot) & 1u ? order + (size_t)slot * stride : nullptr };
	}
};

struct ht_ctx
{
	bool ready = false, profile = false;
	bool cnn_only = false;          // created without a hand model: only the CNN entry points work
	bool profile_phases = false;     // also time the minor phases (serialises the side streams; used for the phase table, not for the timed region)
	int B = 0, device = 0;
	int solver_build = 0;           // ht_debug_solver_build: 0 = the launcher's choice; 5 = the exact-order instantiation (tests only): the reference's own sweeps, cloud rows in the reference's layout
	float *d_exact_lin = nullptr, *d_exact_ang = nullptr;      // its two-body linear rows [B][512][HT_ROW] and angular rows [B][256][8] (allocated when first asked for)
	int contact_kernel = 0;         // ht_debug_contact_kernel: 0 = the launcher's choice, 1 cooperative, 2 lane-per-pair
	std::string err;
	hipStream_t stream = nullptr;
	hipStream_t last_user_stream = nullptr;         // stream of the latest *_dev call (host-read helpers wait for it too)
	hipStream_t side[2] = { nullptr, nullptr };     // independent kernels of one fit step (cloud rows, contacts, chamber) run side by side
	hipEvent_t ev_fork = nullptr, ev_join[2] = { nullptr, nullptr }, ev_lap = nullptr;
	unsigned side_open = 0;                         // bit i: side stream i was forked off an update's stream and has not come back to it yet
	// The edges between an update's streams (ht_edge_event, ht_solver_api.hip: fork / join1).  edge_mode: ht_debug_stream_edges, 0 = the product's events and launch forms,
	// 1 = the edges as they were up to round 29 (tests only).  edges_on_launch: this update's solves and cloud-row launches may carry the next edge's event as their own
	// completion event (never while the caller's stream is being captured).  fork_carried: the stream whose last launch, a solve, completes ev_fork -- the fork that follows
	// on that stream records nothing; join_carried, bit i: side stream i's last launch, the cloud rows, completes ev_join[i] -- the join that follows records nothing.
	int edge_mode = 0; bool edges_on_launch = false; hipStream_t fork_carried = nullptr; unsigned join_carried = 0;
	hipEvent_t ev_job = nullptr, ev_seed = nullptr; bool job_pending = false; void *h_job_in = nullptr; size_t h_job_cap = 0;      // ht_job_start: the CNN job of the overlapped update() in flight on this context, its pinned input staging
	ht_params par;
	ht_physics_dev phys;
	ht_model_dev model;
	// The two pose nets (ht_net_of): the reference's, on 64x64 tiles, whose input and convolution buffers come with the context (ht_alloc_buffers), and the same layers on
	// a larger input (BASELINE configs[4]), whose buffers come with its first weights (ht_cnn_load_weights_sized).  Either net's mini-batch arena comes with its first step.
	ht_net net[2] = { { ht_net_dims_of<64>(), "cnn", "CNN weights not loaded (ht_cnn_load_weights)",
	                    ": the context holds no weights of the 64x64-input net (ht_cnn_load_weights); the 128x128-input net is trained by ht_cnn_train_batch_sized",
	                    "weights: expected HT_CNNB_COUNT fp32 values in .cnnb order" },
	                  { ht_net_dims_of<128>(), "cnn128", "weights of the 128x128 net not loaded (ht_cnn_load_weights_sized)",
	                    ": the context holds no weights of the 128x128-input net (ht_cnn_load_weights_sized)", "weights: expected HT_CNNB128_COUNT fp32 values in .cnnb order" } };
	ht_model_rec rec;                                             // the model on the host, the one copy (ht_model_build.hpp): load_model reads it, ht_scale scales it, both lay it out for the device
	std::vector<float> &h_bodyc = rec.bodyc, &h_jointc = rec.jointc;      // its body and joint tables under the names their readers know
	float *d_train = nullptr;                                    // the per-sample step's training arena (the 64x64-input net only): layer outputs, errors, split-K partial sums (allocated on first use)
	char *d_io = nullptr; size_t io_cap = 0;                     // the staging of every synchronous host form (ht_staged_call: inputs up, outputs down), grown to the largest call (dev_grow)
	float *d_sf_ref = nullptr, *d_sf_crays = nullptr;             // slowfit inputs [B][nb][7], [B][8][4] (allocated on first use)
	float4 *d_cverts_rw = nullptr;                                // padded copy of the collision vertices (ht_model_dev::cverts)
	float4 *d_verts_rw = nullptr, *d_planes_rw = nullptr; float *d_bodyc_rw = nullptr, *d_jointc_rw = nullptr;
	std::vector<void *> allocs;
	std::map<std::string, ht_prof_entry> prof;

	// device buffers (capacity B frames / tracker slots)
	uint16_t *d_depth = nullptr;
	uint16_t *d_seg_tiles = nullptr, *d_frames = nullptr; float *d_frame_cams = nullptr, *d_frame_cams_in = nullptr; int *d_overflow = nullptr; size_t frames_cap = 0, seg_tiles_cap = 0;      // full-size frame path (ht_update_frames); d_frames holds the largest frame size seen, d_seg_tiles the largest tile side (dev_grow)
	float *d_cams = nullptr, *d_analysis = nullptr;
	float *d_act3 = nullptr, *d_logits = nullptr, *d_cnn_out = nullptr;      // shared by both nets: the latest evaluation's first FC layer, logits and output, whichever net ran
	float4 *d_pts = nullptr; int *d_npts = nullptr;
	float4 *d_ptsv = nullptr; int *d_nptsv = nullptr;          // the main-thread cloud when subsample_voxel is set (allocated on first use; d_pts stays the CNN job's cloud)
	float *d_state[2] = { nullptr, nullptr };      // [B][nb][HT_STATE_STRIDE]: 0 handmodel, 1 othermodel
	float *d_prev_err = nullptr; int *d_initializing = nullptr;
	float *d_err_old = nullptr, *d_err_new = nullptr; int *d_flags = nullptr, *d_nflags = nullptr;
	int *d_flist = nullptr, *d_nflist = nullptr;      // the flagged frames of an update as a list [B] and its length (k_prepare clears it)
	// How many frames took the full-reset branch so far (device counter, copied to pinned host memory behind every update's reset kernel, never waited for):
	// an update that follows one with more reset frames than the device has CUs launches the reset branch and those frames' first contact step in their
	// many-frames organisation (two reset blocks per CU, four frames per contact block) instead of the few-frames one.  A hint only: both are always correct.
	unsigned *d_nreset = nullptr; volatile unsigned *h_nreset = nullptr;      // [2]: frames that reset, updates that counted them
	unsigned nreset_seen[2] = { 0, 0 }; bool many_reset = false, tail_pending = false; int n_cu = 256;
	int last_reset_many = -1;       // which organisation the latest update launched the reset branch in (ht_debug_reset_organisation): 0 few frames, 1 many
	float *d_rows = nullptr; int *d_nrows = nullptr;            // cloud rows [B][pts_cap][HT_ROW] in the reference's layout (stage calls, UnibodyFit, caller-built rows)
	unsigned char *d_rowbody = nullptr;                          // [B][pts_cap] body of every cloud row whose solver record k_cloud_rows wrote into d_scratch
	float *d_chamber = nullptr; int *d_nchamber = nullptr;      // [B][5*nb][HT_ROW]
	float *d_tables = nullptr;                                   // [B][TB_WORDS] the solve tables k_solve_prep makes and k_solve reads (ht_solve_shared.hpp)
	float *d_chplanes = nullptr; int *d_chon = nullptr; bool planes_valid = false;      // [B][5][4], [B]: the boundary planes of the update's main-thread cloud (k_chamber_planes: once per update); valid inside the update that made them
	int solve_tables = 0;                                       // 1 (ht_debug_solve_tables; tools/exp_tables.sh): k_solve_prep makes every solve's tables beside the contact kernel.  Measured slower in round 6 (profiles/r06_notes.md section 1): off
	int *d_accepted = nullptr;
	float *d_contacts = nullptr; int *d_ncontacts = nullptr;    // [B][HT_MAXCONTACT][HT_CONTACT]
	bool tables_out = false;        // this update's launch tables (contact_hist.order, solve_hist.order) are still being made on side stream 0: until that stream is joined only launches ON it may read them (ht_solver_api.hip: update_beside_net)
	ht_history contact_hist, solve_hist;
	int *d_porder = nullptr;      // [B]: the frames by their point counts (ht_model_dev::frame_order inside an update of a batch of several rounds per CU)
	unsigned char *d_epa_ws = nullptr;                           // expanding-polytope workspace, one per (frame, wave)
	float *d_scratch = nullptr;                                  // solver row records [B][pts_cap + 5*nb + 32][20] (ht_quad.hpp)
	float *d_poses_out = nullptr, *d_start = nullptr;
	float *d_stage = nullptr;                                    // staging for host<->device state copies
	// caller-built constraint rows (ht_fit_rows / ht_physics_update), allocated on first use and grown to the largest call (dev_grow)
	float *d_user_lin = nullptr; unsigned short *d_user_pos = nullptr; float *d_user_ang = nullptr; int *d_user_n = nullptr;      // [B][lin_cap][HT_ROW], [B][lin_cap], [B][ang_cap][HT_AROW], [4][B]
	int user_lin_cap = 0, user_ang_cap = 0;
	ht_comm_state *comm = nullptr;                               // multi-GPU pose gather (ht_comm_init), null on a single-GPU host
	std::vector<float> render_radii; unsigned render_gen = 0;     // ht_render_depth's per-body cull radii (2 per body) and the record's generation (rec.gen) they were derived at
	// ht_render_mesh_depth: the record's mesh rows on the device, [t][4] float4 (corners and PolyPlane), and the farthest corner of every body's mesh from its centre of
	// mass (ht_mesh_upload makes both)
	std::vector<float> mesh_rad; float4 *d_mesh = nullptr;
	float *d_jointl = nullptr;                                   // [nj][HT_JL] the limits of the joint coordinates, made once at model load beside jointc (ht_joint_limits; ht_scale leaves them)
	// ht_update_hands_*: the mirrored inputs an update of flagged frames runs on, [B][hands_px] pixels, [B][12], [B][nb][7], and the flags of the host form [B]; nothing until the
	// first flagged call or ht_reserve_hands, then grown to the largest frame (hands_reserve, ht_solver_api.hip: one synchronising re-allocation, never smaller)
	uint16_t *d_hands_frames = nullptr; size_t hands_px = 0; float *d_hands_cams = nullptr, *d_hands_start = nullptr; unsigned char *d_hands_flags = nullptr;
	// ht_split_hands (ht_split.hip): the label image of a call whose caller wants none (the frames are cut along it), grown to the largest call (dev_grow).
	// ht_update_two_hands_*: its info [B/2][2][8] when the caller wants none, and the flags 0, 1, 0, 1, ... [B] its pose mirrors take (made once)
	uint16_t *d_split_labels = nullptr; size_t split_labels_cap = 0;
	int32_t *d_two_info = nullptr; unsigned char *d_two_flags = nullptr;
	// the model split (ht_split_model.hip): the blob split's component counts of a MERGED call whose caller wants none (ht_update_two_hands_model_*: and behind them, from
	// max_batch / 2, the frames' sources), grown to the largest call (dev_grow)
	int32_t *d_model_ncomp = nullptr; size_t model_ncomp_cap = 0;
	// tracking accuracy (ht_quality.hip): the offsets of HT_KP_FEATURE8 [8][3] (handmodelfeaturepoints, handtrack.h:77-81; ht_scale multiplies them as it does the
	// centres of mass -- HT_KP_SKELETON is read off h_jointc / h_bodyc when asked for); ht_pose_depth_residual's render poses
	// [B][nb][7] and rendered frames [B][h][w], grown to the largest call with one synchronising re-allocation before anything is enqueued (quality_reserve)
	float kp_feature8[24] = { 0, 0, 0, -0.03f, 0, -0.03f, 0.03f, 0, -0.03f, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	float *d_quality_poses = nullptr; size_t quality_poses_cap = 0; uint16_t *d_quality_frames = nullptr; size_t quality_frames_cap = 0;
	// several views (ht_views.hip): the ray origins of the slots' fused clouds [B][2 HT_VIEWS_MAX][3] (k_fuse_views writes them, k_view_rows reads the one a point's
	// .w names), the per-source counts of a call whose caller wants none [B][2 HT_VIEWS_MAX] with the count of cut slots behind them (allocated on first use), the slots
	// [0, views_B) the latest ht_fuse_views filled, and ht_update_views_*'s contiguous copy of view 0's frames and cameras (dev_grow)
	float *d_view_origins = nullptr; int *d_view_src = nullptr; int views_B = 0;
	uint16_t *d_view0 = nullptr; size_t view0_cap = 0; float *d_view0_cams = nullptr;
	// a view's extrinsics (ht_calib.hip): the view's clouds in camera space [calib_B][calib_stride] with their counts [calib_B], the slots' 29 sums
	// [calib_B][CA_PART] and the transforms [calib_B][8], both float64; all four follow the largest call (calib_reserve: one synchronising re-allocation)
	float4 *d_calib_pts = nullptr; int *d_calib_n = nullptr; double *d_calib_part = nullptr, *d_calib_T = nullptr; size_t calib_B = 0, calib_stride = 0;
	// the hand's size (ht_size.hip) takes the cloud, its counts and the transforms above, and keeps the slots' 37 sums with the solve's per-slot pieces [size_B][SZ_PART]
	// and the scales [size_B], both float64 (size_reserve, the same growth)
	double *d_size_part = nullptr, *d_size_s = nullptr; size_t size_B = 0;
};

// The net of a side x side input; any other side is refused here, and only here
static inline ht_net *ht_net_of(ht_ctx *ctx, int side)
{
	for (ht_net &n : ctx->net) if (n.dims.side == side) return &n;
	ctx->err = "CNN input side must be 64 or 128";
	return nullptr;
}
// the entry point's name in the messages of a *_sized call: at side 64 it is the unsized call and says so
static inline const char *ht_form_name(const ht_ctx *ctx, const ht_net *net, const char *unsized, const char *sized) { return net == &ctx->net[0] ? unsized : sized; }
// what every entry point of the C-ABI starts with and wraps its HIP calls in
#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return HT_ERR_HIP; } } while (0)
#define CHECK_READY(ctx) if (!(ctx)) return HT_ERR_ARG; if (!(ctx)->ready) { (ctx)->err = "context not initialised (ht_create failed)"; return HT_ERR_STATE; } ht_device_guard dev_guard_((ctx)->device)
#define CHECK_MODEL(ctx) do { if ((ctx)->cnn_only) { (ctx)->err = "this context was created without a hand model (CNN only)"; return HT_ERR_STATE; } } while (0)
#define CHECK_BATCH(ctx, B) do { if ((B) < 1 || (B) > (ctx)->B) { (ctx)->err = "batch exceeds the capacity given to ht_create"; return HT_ERR_ARG; } } while (0)
// the exact-order instantiation of the solver (ht_debug_solver_build 5, tests only) takes the cloud rows in the reference's layout (ctx->d_rows) instead of records
static inline bool exact_solver(const ht_ctx *ctx) { return ctx->solver_build == 5 || ctx->solver_build == 8; }      // 8: the same sweeps with the product's forked launch sequence (5 takes the kernels in order on one stream)
// The entry points that solve rows of the caller's (ht_fit_rows, ht_physics_update, ht_slowfit, ht_fit_keypoints) refuse that instantiation before they upload or launch anything
#define REFUSE_EXACT_SOLVER(ctx) do { if (exact_solver(ctx)) { (ctx)->err = "the exact-order instantiation (ht_debug_solver_build 5) serves the update entry points only"; return HT_ERR_STATE; } } while (0)
// argument checks the entry points share (each composes its own message): whether two byte ranges overlap (a null or empty one overlaps nothing), and a frame's size
static inline bool ht_ranges_overlap(const void *a, size_t na, const void *b, size_t nb) { return a && b && na && nb && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; }
static inline bool ht_frame_dims_ok(int w, int h) { return w >= 1 && h >= 1 && w <= 4096 && h <= 4096; }

// Device memory of a context.  dev_alloc: n elements, listed in `allocs` (ht_destroy frees the list).  drop_alloc: frees one of them now.  dev_grow: a buffer that follows
// the largest call -- the replacement is allocated FIRST (when that fails the context keeps its old, valid buffer and capacity), then the outgrown one is freed (hipFree
// waits for the device, so nothing can still be reading it); its contents are not carried over.
template <class T> static inline int dev_alloc(ht_ctx *ctx, T **p, size_t n)
{
	void *q = nullptr;
	HIPCHK(ctx, hipMalloc(&q, n * sizeof(T)));
	ctx->allocs.push_back(q);
	*p = (T *)q;
	return HT_OK;
}
static inline void drop_alloc(ht_ctx *ctx, void *o) { if (!o) return; for (auto &q : ctx->allocs) if (q == o) { q = ctx->allocs.back(); ctx->allocs.pop_back(); break; } (void)hipFree(o); }
template <class T, class C> static inline int dev_grow(ht_ctx *ctx, T **p, C *cap, size_t want, size_t per = 1)
{
	if ((size_t)*cap >= want) return HT_OK;
	T *q = nullptr;
	const int r = dev_alloc(ctx, &q, want * per);
	if (r) return r;
	drop_alloc(ctx, *p);
	*p = q; *cap = (C)want;
	return HT_OK;
}
static inline int ht_history_alloc(ht_ctx *ctx, ht_history &h)      // for the context's capacity; the works zeroed: a slot no launch has written yet ranks equal keys, not garbage
{
	h.stride = ht_history::stride_for(ctx->B);
	const size_t n = (size_t)HT_CONTACT_SLOTS * h.stride;
	if (int r = dev_alloc(ctx, &h.work, n)) return r; else if ((r = dev_alloc(ctx, &h.order, n))) return r;
	HIPCHK(ctx, hipMemset(h.work, 0, n * sizeof(int)));
	return HT_OK;
}
// the end of a synchronous entry point: wait for the stream, then report what its launches left behind
static inline int ht_sync_check(ht_ctx *ctx, hipStream_t s)
{
	HIPCHK(ctx, hipStreamSynchronize(s));
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

// A synchronous entry point around its _dev form: the segments laid out 256-aligned in ctx->d_io, which follows the largest call (dev_grow), the inputs uploaded,
// call(stream) run on the device pointers, the outputs downloaded, the context's stream waited for.  A segment without a host pointer (an optional output the
// caller did not ask for) takes no room and keeps a null device pointer.
// Every host form shares the one buffer.  That is sound because a staged call is synchronous on ctx->stream (nothing reads d_io once it has returned, and hipFree
// of an outgrown buffer waits for the device), and because no `call` body enters another host form: each runs its own _dev form or enqueue function, which stage nothing.
struct ht_seg { void *host; size_t bytes; bool out; char *dev; };
template <class F> static inline int ht_staged_call(ht_ctx *ctx, ht_seg *seg, int n, F call)
{
	size_t off[12], end = 0;      // n <= 12
	for (int i = 0; i < n; i++) { off[i] = (end + 255) & ~(size_t)255; if (seg[i].host) end = off[i] + seg[i].bytes; }
	{ const int r = dev_grow(ctx, &ctx->d_io, &ctx->io_cap, end); if (r) return r; }
	for (int i = 0; i < n; i++) seg[i].dev = seg[i].host ? ctx->d_io + off[i] : nullptr;
	hipStream_t s = ctx->stream;
	for (int i = 0; i < n; i++) if (seg[i].host && !seg[i].out) HIPCHK(ctx, hipMemcpyAsync(seg[i].dev, seg[i].host, seg[i].bytes, hipMemcpyHostToDevice, s));
	{ const int r = call(s); if (r) return r; }
	for (int i = 0; i < n; i++) if (seg[i].host && seg[i].out) HIPCHK(ctx, hipMemcpyAsync(seg[i].host, seg[i].dev, seg[i].bytes, hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipStreamSynchronize(s));
	return HT_OK;
}

// Keypoint tables (ht_quality.hip; shared with ht_kpfit.hip): the table a call names, checked -- a built-in one of the context's model as ht_scale left it, or the
// caller's -- as the kernels take it by value, and whether any output of a host form overlaps an input or another output
struct ql_table { int K; unsigned char bone[HT_KP_MAX], rel[HT_KP_MAX]; float off[HT_KP_MAX * 3]; };
struct ql_buf { const void *p; size_t bytes; };
int ql_table_of(ht_ctx *ctx, const char *fn, int which, int K, const int *bones, const float *offsets, const int *rel, ql_table &t);
bool ql_any_overlap(const ql_buf *in, int nin, const ql_buf *out, int nout);
// Caller-built rows (ht_solver_api.hip; shared with ht_kpfit.hip): the context's row buffers for lin_cap linear and ang_cap angular rows a frame, and one
// PhysModel::FitPointCloud step on model `which` of slots [0,B) with the linear rows and counts that d_user_lin / d_user_n hold, enqueued on s and not waited for
int ht_user_rows_reserve(ht_ctx *ctx, int lin_cap, int ang_cap);
void ht_fit_rows_enqueue(ht_ctx *ctx, int which, int B, float microforce, int ang_bound, int zero_momenta, hipStream_t s);
// Several views (ht_views.hip; the fit's launch sequence is ht_solver_api.hip's).  ht_fuse_views_reserve: every refusal of ht_fuse_views_dev and whatever grows, before
// anything runs; ht_fuse_views_enqueue: the launch alone, on s.  ht_views_planes_ok: the mirror planes a host form refuses.  ht_fit_views_enqueue: `passes` times
// ht_fit_rows_enqueue's sequence with the cloud rows of the fused points from their own ray origins and no caller rows, the momenta kept; the last solve writes the user
// poses to d_poses (may be null)
int ht_fuse_views_reserve(ht_ctx *ctx, const char *fn, const void *depth, const void *cams, int w, int h, int V, int B, const ht_views *o);
int ht_fuse_views_enqueue(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, int B, const ht_views *o, int *d_npoints, int *d_per_source,
                          float *d_origins, int *d_cut, hipStream_t s);
int ht_views_planes_ok(ht_ctx *ctx, const char *fn, const float *planes, size_t n);
int ht_fit_views_enqueue(ht_ctx *ctx, int which, int B, int passes, float *d_poses, hipStream_t s);

struct ht_prof_scope
{
	ht_ctx *ctx; ht_prof_entry *ent; hipStream_t stream; size_t slot;
	ht_prof_scope(ht_ctx *c, const char *name, hipStream_t s, bool minor_phase = false);
	~ht_prof_scope();
};

// rows of a frame's slot of the solver scratch: every point and chamber row, k_solve's read-ahead slack, the rows that pad a host body's chain
// to a multiple of 8 when a body beyond the 16th rides on its quad (7 per such body at most), and the tail that takes what does not fit k_solve's LDS
static inline size_t ht_scratch_rows(size_t pts_cap, size_t nb) { return pts_cap + 5 * nb + 32 + 7 * 16 + HT_SCRATCH_TAIL; }
int ht_alloc_buffers(ht_ctx *ctx);
int ht_mesh_upload(ht_ctx *ctx);             // rows and radii of the model's current subdivision meshes to the device (ht_render_mesh.hip); the caller has waited for the renders in flight
// What the mesh renderers' kernel arguments take from the record: the bodies' centres of mass [nb][3] and first mesh triangles [nb + 1] (com, tri_off of rm_model / rz_model)
static inline void ht_mesh_args(const ht_ctx *ctx, float *com, int *tri_off)
{
	for (int b = 0; b <= ctx->model.nb; b++) tri_off[b] = ctx->rec.mesh_off[b];
	for (int b = 0; b < ctx->model.nb; b++) for (int i = 0; i < 3; i++) com[3 * b + i] = ctx->rec.bodyc[(size_t)b * HT_BC + HT_BC_COM + i];
}
// The one creator of the events that order an update's own streams (ev_fork, ev_join[], ev_lap) and the job's seed copy against the caller's stream (ev_seed).  Every
// consumer of these events is a kernel or a copy of THIS device behind a hipStreamWaitEvent, and a kernel's end already releases its writes at device scope, so the events go
// without the system-scope fence of an ordinary record (hipEventDisableSystemFence): tools/exp_stream_edges.hip measured a fork / join pair at 10.0 -> 7.9 us with the join
// hidden and 24.5 -> 20.4 us with the join exposed, every read on the other stream correct across the XCDs (profiles/r30_stream_edges.md; hipEventReleaseToDevice
// measured the same as no flag).  Not for an event the host queries or waits for (ev_job) and not for the events that order an update against RCCL, whose peers are other
// devices (ht_comm.hip): those keep the ordinary fence.  ht_debug_stream_edges(ctx, 1) makes the events as they were up to round 29.
#define HT_EDGE_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
static inline hipError_t ht_edge_event(const ht_ctx *ctx, hipEvent_t *ev) { return hipEventCreateWithFlags(ev, ctx->edge_mode == 1 ? (unsigned)hipEventDisableTiming : (unsigned)HT_EDGE_EVENT_FLAGS); }
int ht_alloc_solve_tables(ht_ctx *ctx);      // d_tables and nothing else, once (d_chplanes / d_chon come with ht_alloc_buffers): from ht_debug_solve_tables(ctx, 1 or 2), and from ht_alloc_buffers under HT_TABLES in a tuning build
int ht_reserve_points_locked(ht_ctx *ctx, int points);      // grows the per-point arrays (ht_api.hip); waits for the context's streams
// *_dev entry points: a NULL stream means the context's own stream (never the legacy default stream); the choice is remembered so that the
// host-read helpers (ht_capacity_events, ht_frames_overflow, ht_get_tracker_flags, ...) can wait for work enqueued on a caller's stream
static inline hipStream_t ht_user_stream(ht_ctx *ctx, void *stream) { hipStream_t s = stream ? (hipStream_t)stream : ctx->stream; ctx->last_user_stream = s; return s; }
static inline hipError_t ht_sync_all(ht_ctx *ctx)
{
	hipError_t e = hipStreamSynchronize(ctx->stream);
	if (e == hipSuccess && ctx->last_user_stream && ctx->last_user_stream != ctx->stream) e = hipStreamSynchronize(ctx->last_user_stream);
	return e;
}
