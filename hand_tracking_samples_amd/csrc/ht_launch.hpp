// ht_launch.hpp -- host-callable launchers of the solver-side kernels (product code).
#pragma once
#include "ht_device.hpp"
#include <hip/hip_ext.h>      // hipExtLaunchKernelGGL: a launch that completes an event of the caller's (ht_launch_solve, ht_launch_cloud_rows)

struct solve_args
{
	const float *rows_pre; const int *n_pre; int pre_stride;      // chamber rows [B][pre_stride][HT_ROW] (may be null)
	const float *rows_cloud; const int *n_cloud;                    // cloud rows [B][pts_cap][HT_ROW] (may be null)
	const unsigned char *cloud_body;                                // [B][pts_cap]: k_cloud_rows has written the cloud rows' RECORDS into the frames' scratch slots (rows_cloud unused) and their bodies here
	const float *contacts; const int *ncontacts;                    // [B][HT_MAXCONTACT][HT_CONTACT] (may be null)
	// caller-built rows (ht_fit_rows / ht_physics_update = PhysModel::FitPointCloud's and PhysicsUpdate's row arguments; all may be null):
	const float *ang_user; const int *n_ang_user; int ang_user_stride;        // angular rows [B][stride][HT_AROW]: first in the angular list
	const float *lin_tail; const int *n_lin_tail; int lin_tail_stride;        // linear rows from the caller's first two-body row on [B][stride][HT_ROW]: ahead of the joint rows
	const unsigned short *lin_tail_pos; const int *n_tail_groups;             // their placement, made by the host: group << 2 | slot, bit 15 = the row's group is a contact triple
	int no_model_rows;                                                        // PhysicsUpdate: the caller's rows are all there is (no joint rows, no HandModelEnhancements)
	const float *analysis; const float *cams;                       // for ApplyAngles / landmark-ray rows / arm cone
	const int *active_flag;                                         // optional per-frame enable
	float *state;                                                   // [B][nb][HT_STATE_STRIDE] of the model being solved
	float *scratch; int scratch_stride;                             // [B][scratch_stride][HT_CREC] pre-computed single-body row records (ht_quad.hpp)
	int batch;                                                      // frames of the launch (the sums of over-size frames live behind all frames' records)
	int apply_angles; float drive_force; int ray_rows; int arm_cone; int zero_momenta; int steps_keyangles; float min_cray_prob;
	// slowfit (handtrack.h:786-821): landmark rays from the origin (sf_crays [B][8][4], first sf_ncray used), a bone nailed to a point, and
	// RelativeAngularConstraints against a reference pose (sf_refpose [B][nb][7], sf_hold = 1 or 2); all off when zero / null
	const float *sf_crays; int sf_ncray; int sf_select; float sf_spoint[3], sf_rbpoint[3]; const float *sf_refpose; int sf_hold;
	int *caps;                                                      // capacity counter: frames x launches whose angular rows exceeded the LDS records (may be null)
	int shared_gpu;                                                 // other kernels run beside this launch (the reset path): keep the small LDS footprint
	const int *frame_order; int *cost_out;                          // batches of several rounds per CU: block i takes frame frame_order[i] (the frames by what they took in the same launch of the previous update, longest first, so that the launch ends on short ones); cost_out [B]: what each took now.  Both may be null
	int two_body_levels;                                            // tests only (ht_debug_solver_build 7): the two-body rows by the level schedule for every frame, as until round 4 (otherwise only frames the blocked form does not hold)
	int force_build;                                                // 0: the launcher chooses k_solve's build; 1 small, 2 only, 3 mid, 4 tiny (every array in HBM): ht_debug_solver_build
	// the last solve of an update also delivers the poses (GetPoseUser physmodel.h:434 + the "initializing = 50" rule of handtrack.h:781-782), instead of a launch of its own
	float *out_poses; const int *out_npts; int *out_initializing; int out_min_point_num;
	int ang_extra_bound;                                            // angular rows a frame can have beyond the 13 CNN-driven ones and 6 per joint (slowfit: 3 per joint; caller-built rows: their largest count): picks the build
	float *exact_lin, *exact_ang;                                   // force_build 5 (tests only, ht_debug_exact_solver): the two-body linear rows [B][512][HT_ROW] and the angular rows [B][256][8] in the reference's layout, for the reference's own sweeps
	const float *tables;                                            // [B][TB_WORDS] (ht_solve_shared.hpp): k_solve_prep has made this solve's tables; null: k_solve's own prologue
	int dbg;                                                        // timing experiments only (HT_DEBUG_SKIP): 1 skip chains, 2 skip two-body linear, 4 skip angular
};

// k_solve_prep (csrc/ht_prep.hip): the tables of one solve, four waves per frame, on a side stream beside the contact kernel (layout: ht_solve_shared.hpp)
#define TB_WORDS 8928      // words of a frame's tables
struct prep_args
{
	const float *state; const float *analysis; const float *cams; const int *active_flag;
	float *scratch; int scratch_stride; int batch;
	const unsigned char *cloud_body; const int *n_cloud;      // the cloud rows' bodies (k_cloud_rows wrote their records into the scratch slots); null: a solve without cloud rows
	const float *ch_planes; const int *ch_on;                   // boundary planes [B][5][4] of the frames whose ch_on is set (k_chamber_planes); null: a solve without them
	float *rows_pre; int *n_pre; float ch_maxforce;             // their rows in the reference's layout [B][5 * nb][HT_ROW] and count, for a frame that falls back to k_solve's own prologue
	int apply_angles; float drive_force; int ray_rows; int arm_cone; int steps_keyangles; float min_cray_prob;
	int parts;                                                  // which tables this launch makes: 1 the pose-only ones (joints' groups, angular records, the blocks' couplings and edges: waves 0 and 1), 2 the chain tables (waves 2 and 3: lists, dealing, four-row couplings, landmark rays, boundary-plane rows)
	float *tables;                                              // [B][TB_WORDS]
	int dbg;
};
void ht_launch_solve_prep(const ht_model_dev &M, const ht_physics_dev &ph, const prep_args &a, int B, hipStream_t s);

// where k_cloud_rows puts the solver's records of its rows (ht_quad.hpp): the frames' scratch slots [B][stride][HT_CREC], the rows' bodies [B][pts_cap], the time step
struct cloud_records { float *scratch; int stride; unsigned char *body; float dt; };
// the boundary-plane rows a main-thread pass takes from the same launch (k_chamber's rows by extra blocks of k_cloud_rows): planes / on as ht_launch_chamber_planes left them, rows [B][5 * nb][HT_ROW], nch [B]
struct plane_rows { const float *planes; const int *on; float maxforce; float *rows; int *nch; };
// Which points of a frame's cloud k_cloud_rows takes (every stride-th), where their rays start (cam_origin: the camera's position; 0: the origin) and how the rows' force limits scale
//   CLOUD_UNIT: forcelimit (-1, 1), CloudConstraints as is     CLOUD_FIT: FitPointCloud (physmodel.h:347)     CLOUD_MULTISTEP: MultiStepSim (handtrack.h:656, 681)
//   CLOUD_UNIBODY: UnibodyFit (handtrack.h:461)                 CLOUD_SLOWFIT: slowfit (handtrack.h:815-816)
enum ht_cloud_mode { CLOUD_UNIT = 0, CLOUD_FIT = 1, CLOUD_MULTISTEP = 2, CLOUD_UNIBODY = 3, CLOUD_SLOWFIT = 4 };
struct cloud_take { int stride, cam_origin, mode; };
// The kernel's five force-limit parameters.  ht_cloud_limits: from the tracker's parameters -- except that slowfit's scaling has no use for weak_force / cf_max_point and
// sends its step ratio and wrist factor in their places
struct cloud_limits { float microforce, weak_force, cf_max_point, cf_max_sum, unibody_force; };
static inline cloud_limits ht_cloud_limits(const ht_params &par, int mode, float sf_ratio = 0.0f, float sf_wrist = 0.0f)
{
	const bool sf = mode == CLOUD_SLOWFIT;
	return cloud_limits{ par.microforce, sf ? sf_ratio : par.physics_weak_force, sf ? sf_wrist : par.cloudforce_max_point, par.cloudforce_max_sum, par.unibody_force };
}
// `done` (here and on ht_launch_solve): an event the launch itself completes when its kernel has ended (the stopEvent of hipExtLaunchKernelGGL), instead of a
// hipEventRecord behind it: the same kernel with the same arguments, one marker less in the stream (ht_solver_api.hip: fork1 / join1)
void ht_launch_cloud_rows(const ht_model_dev &M, const float *state, const float4 *pts, const int *npts, const float *cams, const int *active_flag, const cloud_take &take, const cloud_limits &lim,
                          float *rows, int *nrows, int B, hipStream_t s, const cloud_records *rec = nullptr, const plane_rows *planes = nullptr, hipEvent_t done = nullptr);
// The same rows for a fused cloud of several views (ht_views.hip): every point, CLOUD_FIT's limits, and each point's ray from the origin its .w names in the frame's
// table origins [B][2 HT_VIEWS_MAX][3] (k_view_rows: the compile-time mode of the same per-frame code; no plane rows, they assume one viewpoint)
void ht_launch_cloud_rows_views(const ht_model_dev &M, const float *state, const float4 *pts, const int *npts, const float *origins, const cloud_limits &lim, float *rows, int *nrows, int B, hipStream_t s,
                                const cloud_records *rec = nullptr);
// What follows a FitError in HandTracker::update and needs nothing but that frame's error rides on the kernel's last thread instead of a launch of its own:
// mode 1 = the full-reset decision (handtrack.h:706: flags[b] = angles_only || error > threshold), mode 2 = the accept step (handtrack.h:713-731).
struct ht_fit_after
{
	int mode;
	float reset_thr; int angles_only; int *flags, *nflags; int *list, *nlist; unsigned *nreset;      // list / nlist (may be null): the flagged frames, appended in no particular order; nreset (may be null): running counts of the frames flagged and of the decisions taken (one per update)
	float *hand; const float *other; const float *err_old; float *prev_err; int *initializing, *accepted; int nb, min_point_num, always_take_cnn; float accum_thr;
};
void ht_launch_fit_error(const ht_model_dev &M, const float *state, const float4 *pts, const int *npts, const uint16_t *depth, const float *cams, int w, int h, float scale, float *err, int B, hipStream_t s, const ht_fit_after *after = nullptr);
void ht_launch_chamber_planes(const ht_model_dev &M, const float4 *pts, const int *npts, int min_point_num, int enabled, float *planes, int *on, int B, hipStream_t s);      // the five containing planes [B][5][4], on [B] = the frame has them: once per update
void ht_launch_chamber(const ht_model_dev &M, const float *state, const float *planes, const int *planes_on, float maxforce, float *rows, int *nch, int B, hipStream_t s);      // their rows, pass by pass, from planes / planes_on of ht_launch_chamber_planes (k_solve_prep makes them itself with the solve tables)
// The cooperative contact kernel for a model and a batch: frames a block takes (0: a frame of the model does not fit the kernel), the dynamic LDS that needs, and whether that
// is the few-frames form (a frame per block) a launch on a handful of frames may ask for.  ht_contacts_coop: whether a launch takes that kernel or the lane-per-pair one
struct coop_plan { int nfr; size_t lds; bool few; };
coop_plan ht_contacts_coop_plan(const ht_model_dev &M, int B, bool few_frames = false);
bool ht_contacts_coop(const ht_model_dev &M, int B, int force_kernel, bool beside_cloud_rows);
int ht_contacts_lane_waves(const ht_model_dev &M);      // waves per frame of the lane-per-pair kernel (k_contacts<1> / k_contacts<2>)
void ht_launch_contacts(const ht_model_dev &M, const float *state, float driftmax, float jiggle_sin, const int *active_flag, void *epa_ws, float *contacts, int *ncontacts, int B, hipStream_t s, bool beside_cloud_rows = false, int force_kernel = 0, int few_frames = 0,
                        const int *order = nullptr, int *work_out = nullptr);      // order / work_out (cooperative kernel only, both may be null): the frame of every (slot, block) as k_contact_order dealt them for the plan's whole-batch form; where every live frame leaves what it cost
#define HT_CONTACT_SLOTS 16      // unmasked contact launches of an update that keep a work history: MultiStepSim step st -> slot st (< 8), main-thread pass i -> slot 8 + i
void ht_launch_order_by_points(const int *npts, int *order, int B, hipStream_t s);      // order = the frames by their point counts, most first (ht_model_dev::frame_order)
void ht_launch_rank_desc(const int *work, int *order, int B, int stride, unsigned slots, int nslots, hipStream_t s);      // order[slot][.] = the frames of every segment (ht_rank.hpp: HT_RANK_SEG) by work[slot][.], largest first
void ht_launch_contact_order(const int *work, int *order, int B, int nfr, int stride, unsigned slots, int nslots, int epb, hipStream_t s);
size_t ht_contacts_workspace_bytes(int B);
void ht_launch_solve(const ht_model_dev &M, const ht_physics_dev &ph, const solve_args &a, int B, hipStream_t s, hipEvent_t done = nullptr);
void ht_launch_set_pose(float *state, const float *src, int nb, int n, int mode, hipStream_t s);
void ht_launch_get_state(const float *state, float *dst, int nb, int n, hipStream_t s);
void ht_launch_clear_flags(float *prev_err, int *initializing, int n, hipStream_t s);
// the full-reset branch (PoseFromScratch, then n_unibody x UnibodyFit) of the listed frames, one block per frame at a time (k_reset, csrc/ht_cloud.hip)
void ht_launch_reset(const ht_model_dev &M, const ht_physics_dev &ph, float *state, const float4 *pts, const int *npts, const float *analysis, const float *cams, const int *list, const int *nlist,
                     int n_unibody, const ht_params &par, float *rows, int *nrows, float *scratch, int scratch_stride, int batch, int B, hipStream_t s, bool many_frames, int n_cu, bool exact = false);
void ht_launch_output(const ht_model_dev &M, const float *hand, const int *npts, int *initializing, int min_point_num, float *poses, int n, hipStream_t s, int raw = 0);
// ht_segment.hip
bool ht_segment_supported(int w, int h);                             // frames of the unsized entry points: at most 320x240
bool ht_segment_supported_sized(int w, int h, int side);             // frames and tile sides of the sized ones: at most 640x480, side 64 or 128
void ht_launch_segment(const uint16_t *depth, const float *cams, int w, int h, int entry_options, float wrange_hi, float diam, uint16_t *tiles, float *cams_out, int B, hipStream_t s, int side = 64);
void ht_launch_scale_state(float *state, int nb, int n, float s, hipStream_t st);      // ht_track.hip
// ht_train.hip
void ht_launch_train_step(float *w, float *W2p, const float *x, const float *target, float alpha, float *act, float *err, float *part, float *mse_out, hipStream_t s);
size_t ht_train_act_floats();
size_t ht_train_err_floats();
size_t ht_train_part_floats();
void ht_launch_fc_rowmajor(const float *A, const float *W, const float *bias, float *C, int M, int N, int K, bool tanh, hipStream_t s);      // ht_cnn.hip
// ht_train_batch.hip
void ht_launch_train_batch_step(float *w, float *W2p, const float *inputs, const float *targets, const int *index, int n, float alpha, float *arena, int cap, float *mse_out, hipStream_t s, const ht_net_dims &d);
size_t ht_train_batch_floats(int cap, const ht_net_dims &d);
void ht_train_batch_views(float *arena, int cap, const float *view[7], size_t per[7], const ht_net_dims &d);
// the same launches up to the weight steps, which become G = (accumulate ? G : 0) + sum_b g_b(w) over G [d.count] in .cnnb order; the weights are read only
void ht_launch_train_batch_grad(const float *w, float *G, int accumulate, const float *inputs, const float *targets, const int *index, int n, float *arena, int cap, float *mse_out, hipStream_t s, const ht_net_dims &d);
// ht_optim.hip: the gradient's own kernels, the global norm with the clip factor, the optimiser step (its arithmetic: the head of that file) and conv2's packed copy
struct ht_opt_args { float lr, momentum, beta1, beta2, omb1, omb2, bc1, bc2, eps, wd, gs; int coupled, decoupled; unsigned r[8]; };
void ht_launch_opt_fc_wgrad(float *G, float *GB, const float *X, const float *E, int n, int M, int N, int accumulate, hipStream_t s);
void ht_launch_opt_conv_reduce(const float *pw, int groups, int stride, float *G1, float *GB1, float *G2, float *GB2, int accumulate, hipStream_t s);
size_t ht_opt_stat_doubles();
void ht_launch_opt_norm(const float *G, size_t n, float gs, float clip_norm, double *stat, hipStream_t s);
void ht_launch_opt_step(int kind, float *W, const float *G, float *M, float *V, size_t n, const float *clip, const ht_opt_args &a, hipStream_t s);
void ht_launch_opt_pack_w2(const float *W2, float *W2p, hipStream_t s);
// ht_joints.hip (host only): the limits table [nj][HT_JL] of a joint table [nj][HT_JC], its public form (lo / hi [nj][3], an unbounded axis as -inf / +inf; swapped [nj];
// any may be null), and whether a top-down walk in model order places every body
void ht_joint_limits(const float *jointc, int nj, float *table);
void ht_joint_limits_public(const float *table, int nj, float *lo, float *hi, int *swapped);
bool ht_joints_ordered(const float *jointc, int nb, int nj);
bool ht_joints_hand_layout(const float *jointc, int nb, int nj);
// ht_mirror.hip: the mirror x -> -x of frames [B][h][w], cameras [B][12] and poses [B][per_frame][7] where hands[b] != 0 (hands null: everywhere), a copy elsewhere.
// Frames must not overlap; cameras and poses may be in place.
void ht_launch_mirror_frames(const uint16_t *in, int w, int h, int B, const unsigned char *hands, uint16_t *out, hipStream_t s);
void ht_launch_mirror_cams(const float *in, int w, int B, const unsigned char *hands, float *out, hipStream_t s);
void ht_launch_mirror_poses(const float *in, int per_frame, int B, const unsigned char *hands, float *out, hipStream_t s);
// ht_split.hip: the blobs of frames [B][h][w] (k_split_label: info [B][2][8], eligible components [B] or null, label images [B][h/4][w/4]), one masked frame per hand
// out [B][2][h][w] cut along those labels (the left one mirrored with HT_SPLIT_MIRROR_LEFT; in and out must not overlap) and the cameras [B][2][12].  ht_split_check: the
// arguments every entry point refuses (HT_ERR_ARG and ctx->err, named after `fn`)
struct ht_ctx;
int ht_split_check(ht_ctx *ctx, const char *fn, int w, int h, int range_lo, int range_hi, int min_pixels, int far, int flags);
void ht_launch_split_label(const uint16_t *depth, int w, int h, int B, unsigned lo, unsigned hi, unsigned max_step, int min_pixels, int flags, int32_t *info, int32_t *ncomp, uint16_t *labels, hipStream_t s);
void ht_launch_split_write(const uint16_t *in, const uint16_t *labels, const int32_t *info, int w, int h, int B, unsigned far, int flags, uint16_t *out, hipStream_t s);
void ht_launch_split_cams(const float *in, int w, int B, int flags, float *out, hipStream_t s);
// ht_split_model.hip: the cells of frames go to the nearer of two tracked models (k_split_model; in MERGED mode behind k_split_label, whose counts go to ncomp, never null
// then): info, labels [B][h/4][w/4] (never null), and optionally source [B] and dist [B][h/4][w/4][2].  Hand k of frame f's prior is at poses + ((2 f + k) nb + b) pose_stride
// floats; left_canonical: the left prior is in canonical space already.  ht_split_model_check: what every model entry point refuses on top of ht_split_check
int ht_split_model_check(ht_ctx *ctx, const char *fn, float max_dist, int mode, int flags);
void ht_launch_split_model(ht_ctx *ctx, const uint16_t *depth, const float *cams, const float *poses, int pose_stride, int left_canonical, int w, int h, int B, unsigned lo, unsigned hi, unsigned max_step,
                           int min_pixels, float max_dist, int mode, int flags, int32_t *info, int32_t *ncomp, int32_t *source, float *dist, uint16_t *labels, hipStream_t s);
