/*
 * ht_mi355x.h -- C-ABI of the MI355X-native hand-tracking hot path (libht_mi355x.so).
 *
 * This is the drop-in boundary for the per-frame path of IntelRealSense/hand_tracking_samples:
 *   depth tile -> CNN forward (third_party/cnn.h) -> heat-map decode -> dynamics-based pose solver
 *   (include/physmodel.h, third_party/physics.h, third_party/gjk.h) as driven by include/handtrack.h.
 * The reference has no FFI (it is header-only C++), so each entry point cites the reference interface it replaces.
 * C++ wrappers that keep the reference's own names (HandTracker::update, CNN::Eval ...) live in include/ht_handtrack.hpp;
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes, no exceptions across the ABI, every function returns an int status
 * (HT_OK == 0); the caller owns all buffers it passes, the library owns its device memory; one context per
 * (GPU, stream); a context is not thread safe, but contexts on different GPUs may be used from one process or
 * from several threads: every entry point makes its context's device current for the call and restores the
 * caller's afterwards.  *_dev entry points take DEVICE pointers and a hipStream_t (passed as void*) and are
 * asynchronous; a NULL stream means the context's own stream (not the legacy default stream); the host-read helpers
 * (ht_capacity_events, ht_frames_overflow, ht_get_tracker_flags, ht_get_cnn_results) wait for the stream of the latest
 * *_dev call before they read.  The other entry points take HOST pointers and are synchronous.
 *
 * Layouts: a pose is 7 floats (position xyz, orientation quaternion xyzw) like Pose (third_party/geometric.h:111-125);
 * a body state is 13 floats (pose, linear momentum, angular momentum, physics.h:103-116);
 * a camera is 12 floats (focal xy, principal xy, depth_scale, pose) like DCamera (include/misc_image.h:30-55).
 */
#ifndef HT_MI355X_H
#define HT_MI355X_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HT_OK 0
#define HT_ERR_ARG 1          /* bad argument (NULL, size, batch > capacity) */
#define HT_ERR_IO 2           /* file missing / malformed */
#define HT_ERR_HIP 3          /* a HIP call failed (no device, out of memory, launch failure) */
#define HT_ERR_STATE 4        /* call sequence error (e.g. weights not loaded) */

#define HT_CNN_IN 4096        /* 64x64x1 input, handtrack.h:108 */
#define HT_CNN_OUT 2304       /* 8 heat-maps 16x16 + 16 rows x 16 bins, handtrack.h:117-118 */
#define HT_CNNB_COUNT 9458400 /* fp32 values in a .cnnb file, cnn.h:288,454,590 */
#define HT_CNN128_IN 16384    /* 128x128x1 input of the larger variant (BASELINE configs[4]) */
#define HT_CNNB128_COUNT 30429920 /* its weights: conv1 416, conv2 16448, fc1 12544*2048 + 2048, fc2 2048*2304 + 2304 */
#define HT_POSE 7
#define HT_STATE 13
#define HT_CAM 12
#define HT_MAX_POINTS 4096   /* stride of the point / cloud-row arrays of the stage calls, and the point capacity a context starts with (ht_reserve_points) */
#define HT_POINTS_LIMIT 76800 /* 320x240: the largest cloud a frame can carry (every pixel in range, subsample_fraction 1) */
#define HT_ANALYSIS 84        /* floats per frame, see ht_stage_decode */
#define HT_LABELS_SEGMENT_FRAME 1 /* ht_expected_cnn_batch / _dev flag: train-cnn's compress (train-cnn.cpp:31-50) first, see there */
#define HT_LABELS_SIDE128 2       /* ht_expected_cnn_batch / _dev flag: labels of a 128x128 tile, the heat-map camera camsub(cam, 8), see there */

typedef struct ht_ctx ht_ctx;

/* Tunables of HandTracker (handtrack.h:523-547) and the physics globals it sets (physics.h:34-47, handtrack.h:837-838). */
typedef struct ht_params
{
	float full_reset_on_error;      /* 0.6   */
	int   angles_only;              /* 0     */
	int   always_take_cnn;          /* 0     */
	float drangey;                  /* 0.7   */
	int   boundary_planes;          /* 1     */
	float microforce;               /* 1 (synthetic-tracker.cpp:92 sets 3) */
	float cloudforce_max_point;     /* 15    */
	float cloudforce_max_sum;       /* 3000  */
	int   mainthreadpasses;         /* 1 (synthetic-tracker.cpp:93 sets 3) */
	int   subsample_fraction;       /* 4     */
	int   min_point_num;            /* 400   */
	float accum_error_threshold;    /* 0     */
	float min_cray_prob;            /* 0     */
	int   steps, steps_keypoints, steps_keyangles, steps_palmangle, steps_cloudstart, steps_unibody;   /* 5 3 2 2 1 3 */
	int   physics_iterations, physics_iterations_post, physics_use_collision;                          /* 16 4 1 */
	float physics_weak_force;       /* 0.4 (physmodel.h:234) */
	float bone_sum_error_scale;     /* 4   (handtrack.h:369) */
	float unibody_force;            /* 0.1 (handtrack.h:450) */
	int   subsample_voxel;          /* 0: every subsample_fraction-th point; != 0: voxelsubsample (physmodel.h:66-118) for the main-thread cloud (handtrack.h:751) */
	float subsample_size;           /* 0   voxel edge in metres; subsample_fraction is then the least number of points a voxel must hold */
} ht_params;

/* ---- lifecycle --------------------------------------------------------------------------------------------------
 * ht_create      replaces  HandTracker::HandTracker() (handtrack.h:830-839): builds both hand models and the CNN topology.
 *                model_path: the reference's own model file (assets/model_hand.json: "controlcages" + "joints"), which is
 *                built on the host exactly as PhysModel::PhysModel + LoadHandModel build it (physmodel.h:444-475,
 *                handtrack.h:347-366: 2x subdivision, 48-vertex hull, mass properties, planes, ignore lists), or a model
 *                baked earlier by ht_model_bake (recognised by its "HTFX0001" magic).
 *                max_batch: number of independent tracker slots (frames processed per call).
 *                model_path == NULL gives a context without a hand model that only serves the CNN entry points (ht_cnn_*): what a stand-alone
 *                CNN object is in the reference (CNN PoseInitializerCNN(std::string), handtrack.h:103-130); tracker calls on it return HT_ERR_STATE.
 * ht_destroy     replaces  HandTracker::~HandTracker() (handtrack.h:841-844). */
int ht_create(const char *model_path, int max_batch, int device, ht_ctx **out);
int ht_destroy(ht_ctx *ctx);
/* ht_model_bake  replaces  PhysModel::PhysModel(const char *jsonfile) (physmodel.h:444-475) and, with flags & 1,
 *                LoadHandModel()'s post-processing (handtrack.h:350-358).  Host only (no device needed): writes the built
 *                model as a named-array container that ht_create also accepts. */
int ht_model_bake(const char *json_path, const char *out_path, int flags);
const char *ht_last_error(const ht_ctx *ctx);
int ht_get_params(const ht_ctx *ctx, ht_params *p);
int ht_set_params(ht_ctx *ctx, const ht_params *p);                    /* replaces HandTracker::load_config / visit_fields (handtrack.h:549-581, 822-828) */
int ht_model_info(const ht_ctx *ctx, int *n_bodies, int *n_joints, int *max_batch);
/* ht_scale        replaces  float HandTracker::scale(float s) (handtrack.h:591): PhysModel::scale (physmodel.h:196-219,304-319) on both models of
 *                every tracker slot; the caller multiplies its segment_scale (the compatibility header does). */
int ht_scale(ht_ctx *ctx, float s);
/* ht_config_read  replaces  HandTracker::load_config(const std::string &jsonfile) (handtrack.h:822-828): host only.  Applies the file to
 *                *params the way the reference's field decoder does: every field of visit_fields (handtrack.h:549-581) is assigned, one that
 *                the file does not give as a number becomes 0; a missing file leaves everything untouched.  segment_scale and
 *                prev_frame_error (optional) are the two listed fields that live outside ht_params. */
int ht_config_read(const char *jsonfile, ht_params *params, float *segment_scale, float *prev_frame_error);

/* ---- CNN ---------------------------------------------------------------------------------------------------------
 * ht_cnn_load_weights  replaces  CNN::loadb(std::istream&) (cnn.h:590) / PoseInitializerCNN (handtrack.h:103-130): n must be HT_CNNB_COUNT.
 * ht_cnn_eval          replaces  std::vector<float> CNN::Eval(const std::vector<float>&) (cnn.h:550-556) for B inputs at once:
 *                      in [B][4096] -> out [B][2304]. */
int ht_cnn_load_weights(ht_ctx *ctx, const float *weights, size_t n);
int ht_cnn_eval(ht_ctx *ctx, const float *in, float *out, int B);
int ht_cnn_eval_dev(ht_ctx *ctx, const float *d_in, float *d_out, int B, void *stream);
/* ht_cnn_*_sized       the same three calls for a CNN object built from the reference's layer classes (cnn.h:136-511: LConv, LActivation<TanH>, LMaxPool,
 *                      LFull, LSoftMaxChunked) in PoseInitializerCNN's order but on a `side` x `side` input: side = 64 is the net above; side = 128 is
 *                      BASELINE configs[4]'s input size (conv5 -> 124, pool -> 62 -> 31, conv4 -> 28, pool -> 14, FC 12544 -> 2048 -> 2304; weights
 *                      HT_CNNB128_COUNT values in the same .cnnb order, in [B][16384] -> out [B][2304]).  The two nets of a context are independent. */
int ht_cnn_load_weights_sized(ht_ctx *ctx, int side, const float *weights, size_t n);
int ht_cnn_eval_sized(ht_ctx *ctx, int side, const float *in, float *out, int B);
int ht_cnn_eval_sized_dev(ht_ctx *ctx, int side, const float *d_in, float *d_out, int B, void *stream);

/* ---- tracker -----------------------------------------------------------------------------------------------------
 * ht_tracker_reset    replaces  handmodel.SetPose(p) + othermodel.SetPose(p) with momenta, prev_frame_error and initializing
 *                     cleared (physmodel.h:435; what synthetic-tracker does implicitly at start).  poses [n][nb][7].
 * ht_get_state / ht_set_state   read / write PhysModel rigid-body state (which: 0 handmodel, 1 othermodel), [n][nb][13].
 * ht_update_sync      replaces  std::vector<Pose> HandTracker::update(Image<unsigned short>) (handtrack.h:748-785) for B independent
 *                     trackers, with the background CNN job of :755-768 run synchronously every frame (= update_cnn_model, :734-741,
 *                     then mainthreadpasses passes of :769-780).  depth [B][64*64] (64x64 tiles: HandSegmentVR is the identity,
 *                     :283-284), cams [B][12], poses_out [B][nb][7] = GetPoseUser() (physmodel.h:434).
 *                     cnn_out (optional, [B][2304]) receives HandTracker::cnn_output.
 * ht_update_dev       the same on device buffers, asynchronous on `stream`; d_start_poses (optional, [B][nb][7]) re-seeds every
 *                     tracker slot before the update (independent-frame batches, BASELINE config 3).  The call only enqueues (kernels, two
 *                     side streams forked off `stream` and joined back into it, one 8-byte copy to pinned host memory): it can be captured
 *                     into a HIP graph and replayed (tests/test_gpu_graph.py).  d_depth and d_poses_out may be PINNED HOST memory (hipHostMalloc: one
 *                     address for host and device): the input transform then reads the frames over the host link and the last solve writes the poses there --
 *                     for frames that arrive in host memory this beats uploads on a copy stream beside the step (bench.py host_io: 0.94 against 0.80 of the
 *                     device-resident rate at 1024 frames; tests/test_gpu_zero_copy.py).  d_cams is read by many kernels: keep it in device memory. */
int ht_tracker_reset(ht_ctx *ctx, int first, int n, const float *poses);
int ht_get_state(ht_ctx *ctx, int which, int first, int n, float *state);
int ht_set_state(ht_ctx *ctx, int which, int first, int n, const float *state);
int ht_get_tracker_flags(ht_ctx *ctx, int first, int n, float *prev_frame_error, int *initializing);     /* HandTracker::prev_frame_error / initializing (handtrack.h:546-547) */
int ht_set_tracker_flags(ht_ctx *ctx, int first, int n, const float *prev_frame_error, const int *initializing);
int ht_update_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int B, float *poses_out, float *cnn_out);
int ht_update_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_start_poses, int B, float *d_poses_out, void *stream);
/* ht_update_frames_*  the same call on frames that are not 64x64 (w, h multiples of 4, at most 320x240), as HandTracker::update treats them
 *                     (handtrack.h:693-785): HandSegmentVR(dimage, 0xF, {0.1, drangey}, segment_scale) feeds the CNN (:697-701), the point cloud and
 *                     FitError come from the full frame with its own camera (:703-704, :751), and segment.cam.pose goes to PoseFromScratch,
 *                     UnibodyFit and MultiStepSim (:708-713).  depth [B][h*w], cams [B][12] = the frames' cameras.  Any number of in-range points is
 *                     taken, as handtrack.h:751 does: a call whose frames can carry more points than the context holds (w*h / subsample_fraction)
 *                     first grows the per-point arrays (ht_reserve_points; one synchronising re-allocation, 164 bytes per point and frame), so
 *                     ht_frames_overflow (frames of the last call whose cloud was cut) stays 0.
 * ht_reserve_points   grows the per-point arrays ahead of time to `points` per frame (<= HT_POINTS_LIMIT; never shrinks); ht_point_capacity reads it. */
int ht_update_frames_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, int B, float *poses_out, float *cnn_out);
int ht_update_frames_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, const float *d_start_poses, int B, float *d_poses_out, void *stream);
/* ht_update_direct_*  BASELINE configs[4] end to end (SURVEY 8d "config 5 (i)-(iii)"): the same call on side x side frames (side = 128) that are their own segment
 *                     -- what HandSegmentVR returns for a frame of the net's own size (handtrack.h:283-284) -- evaluated by the net of that input size
 *                     (ht_cnn_load_weights_sized; the reference's layer classes cnn.h:136-511 in the order of handtrack.h:108-118), decoded with
 *                     CNNOutputAnalysis(out, camsub(cam, side / 16)) (handtrack.h:218-241), then FitError, the reset branch, MultiStepSim, the accept step and
 *                     the main-thread passes exactly as handtrack.h:703-785.  The reference has no call of its own for this (PoseInitializerCNN is fixed at
 *                     64x64); oracle/ref_harness.cpp `e2e128` drives the reference's stage functions in that order.  side = 64 is ht_update_*.  d_depth of ht_update_direct_dev must be 16-byte aligned (HT_ERR_ARG otherwise).
 */
int ht_update_direct_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int side, int B, float *poses_out, float *cnn_out);
int ht_update_direct_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int side, const float *d_start_poses, int B, float *d_poses_out, void *stream);
/* ht_update_frames_sized_*  HandTracker::update (handtrack.h:693-785) as ht_update_frames_* states it, for either net and frames up to 640x480
 *                     (ht_segment_vr_supported): HandSegmentVR (:697-698, :280-344) cuts the segment at `side` (ht_segment_vr_sized), the net is the one of
 *                     that input size, and the heat maps are decoded with camsub(segment.cam, side / 16) (:218-241).  The point cloud and FitError stay on the
 *                     full frame (:703-704, :751); PoseFromScratch, UnibodyFit and MultiStepSim take segment.cam.pose (:708-713), which does not depend on the
 *                     side.  side 64 on a frame ht_update_frames_* takes is that call; a side x side frame is ht_update_direct_* (with its alignment rule).
 *                     HT_ERR_STATE without the weights of that net.  HT_ERR_ARG, before anything is uploaded or launched, for a call whose frames can
 *                     carry more than HT_POINTS_LIMIT points (w*h / subsample_fraction, or w*h with the voxel rule: 640x480 needs subsample_fraction >= 4). */
int ht_update_frames_sized_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, int B, float *poses_out, float *cnn_out);
int ht_update_frames_sized_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, const float *d_start_poses, int B, float *d_poses_out, void *stream);
int ht_frames_overflow(ht_ctx *ctx, int *frames_over);
int ht_reserve_points(ht_ctx *ctx, int points);
int ht_point_capacity(ht_ctx *ctx, int *points);
/* ht_update_cnn_model_sync  replaces  std::vector<Pose> HandTracker::update_cnn_model(Image<unsigned short>) (handtrack.h:734-741) and, with
 *                     apply_to_handmodel != 0, void HandTracker::kickstart(Image<unsigned short>) (:743-746) for B trackers: the CNN job alone --
 *                     othermodel is NOT re-seeded from handmodel first, no main-thread passes, no "initializing = 50" rule.  poses_out [B][nb][7] =
 *                     othermodel.GetPose() (physmodel.h:433, body poses, not rig space), accepted_out [B] = 1 where the reference returns that pose and
 *                     0 where it returns an empty vector (:720-722); kickstart copies the accepted poses into handmodel.  Frames w x h as
 *                     ht_update_frames_sync (64x64 tiles: segment_scale unused).  cnn_out optional.
 * ht_get_cnn_results  replaces  the members HandTracker::cnn_input, cnn_output and cnn_output_analysis (handtrack.h:583-585) after an update call:
 *                     cnn_input [n][4096], cnn_output [n][2304], analysis [n][HT_ANALYSIS] (layout: ht_stage_decode); any may be NULL. */
int ht_update_cnn_model_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, int B, int apply_to_handmodel,
                             float *poses_out, int *accepted_out, float *cnn_out);
int ht_get_cnn_results(ht_ctx *ctx, int first, int n, float *cnn_input, float *cnn_output, float *analysis);
/* The reference's OVERLAPPED update (handtrack.h:748-785: the CNN job on a background thread, collected by a later call) on two contexts of one device, `job` for the CNN job
 * and `main` for the caller's part.  The synchronous ht_update_* calls stay the definition parity is stated on (the reference's update() is timing dependent).
 * ht_job_start          replaces :757-758: othermodel.SetPose(handmodel.GetPose()); std::async(update_cnn_model_threadsafe(dimage)).  main's handmodel, prev_frame_error and
 *                       initializing are copied to `job`, the frame to pinned staging, the job is enqueued on job's stream; does not wait for it.
 * ht_job_poll           replaces pose_estimator.wait_for(1 ms) == ready (:760): *ready = 1 when the job has finished (hipEventQuery).  ht_job_wait blocks until it has.
 * ht_job_collect        replaces :761-768: handmodel.SetPose(results.pose) where the job accepted its pose (accepted_out [B], may be NULL), prev_frame_error as the job left it,
 *                       the job's initializing = max(initializing - 1, 0) applied to main's current value.  The job's cnn_input / cnn_output / analysis: ht_get_cnn_results(job).
 * ht_update_passes_sync replaces the caller's part of update() (:751-753, 769-785): the frame's cloud, mainthreadpasses x (HandModelEnhancements, cloud_chamber, FitPointCloud)
 *                       on handmodel, the "initializing = 50" rule, handmodel.GetPoseUser() into poses_out [B][nb][7].  Frames w x h as ht_update_frames_sync. */
int ht_update_passes_sync(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, int B, float *poses_out);
int ht_job_start(ht_ctx *job, ht_ctx *main, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, int B);
int ht_job_poll(ht_ctx *job, int *ready);
int ht_job_wait(ht_ctx *job);
int ht_job_collect(ht_ctx *job, ht_ctx *main, int B, int *accepted_out);
/* ht_get_cnn_layers   the intermediate layers of the latest CNN evaluation of slots [first, first + n), for per-layer parity tests (the reference returns every
 *                     layer's output from its forward() calls, cnn.h:550-556): act1 [n][3600] after conv 5x5 + tanh + two max-pools (layer 3 of the list,
 *                     handtrack.h:108-111), act2 [n][2304] after conv 4x4 + tanh + pool (layer 6), act3 [n][2048] after the first fully connected layer + tanh
 *                     (layer 8), logits [n][2304] after the second one (layer 9, before the chunked soft-max).  Any pointer may be NULL. */
int ht_get_cnn_layers(ht_ctx *ctx, int first, int n, float *act1, float *act2, float *act3, float *logits);
/* ht_get_cnn_layers_sized   the same of the net with a side x side input, side = 64 (ht_get_cnn_layers itself) or 128 (ht_cnn_eval_sized, ht_update_direct_*):
 *                     act1 [n][16 * 31 * 31], act2 [n][12544], act3 [n][2048], logits [n][2304].  act3 and logits are the one pair both nets write: they hold whichever
 *                     net was evaluated last.  Any other side, or side 128 before ht_cnn_load_weights_sized(128), is refused with a message; the context stays usable. */
int ht_get_cnn_layers_sized(ht_ctx *ctx, int side, int first, int n, float *act1, float *act2, float *act3, float *logits);
/* ht_capacity_events  how often, since ht_create, a kernel hit a capacity the reference does not have: expanding-polytope runs cut short (gjk.h:417 /
 *                     hull.h:233-310 loop without bound; here at most 128 iterations, 96 vertices, 192 triangles); touching samples beyond the 192 the contact
 *                     kernel's per-frame pool holds, or beyond 40 five-sample patches (physics.h:451-462 keeps them all; every sample the pool holds IS kept and
 *                     solved -- 192 contacts per frame and launch since round 5, it was 96); solves in which a model's angular rows exceeded what the solver keeps.
 *                     All are 0 unless a scene or a model is out of the ordinary. */
int ht_capacity_events(ht_ctx *ctx, int *epa_cut_short, int *contacts_dropped, int *angular_rows_over);
/* The most touching samples / five-sample patches a frame of THIS model can produce (every colliding, non-ignoring pair once; five samples where neither body is smaller than
 * ContactPatch's 0.05 m proximity test, gjk.h:637) beside what the contact kernel's per-frame pool holds: samples_bound <= pool and patches_bound <= patch_slots proves that the
 * kernel keeps every contact the reference's unbounded list (physics.h:451-462) would hold -- true for the stock 17-bone hand (91 <= 192, 0 <= 40). */
int ht_contact_capacity(ht_ctx *ctx, int *samples_bound, int *patches_bound, int *pool, int *patch_slots);

/* ---- training ----------------------------------------------------------------------------------------------------------
 * ht_cnn_train        replaces  float CNN::Train(const std::vector<float> &x, const std::vector<float> &t, float alpha) (cnn.h:558-580) called for
 *                     n samples in sequence (batch-1 SGD as train-cnn.cpp:156-162 does with alpha = 0.001): inputs [n][4096], targets
 *                     [n][2304], mse_out [n] (optional) = the value Train returns for each sample.  The context's weights are updated in place.
 *                     The arrays are staged through a device buffer of the context that follows the largest call of ht_cnn_train / ht_cnn_train_batch and
 *                     is kept until ht_destroy: n * 6401 floats.
 * ht_cnn_get_weights  replaces  CNN::saveb (cnn.h:591-593): the weights in .cnnb order.
 * ht_expected_cnn     replaces  GatherHandExpectedCNN(pose, hcam).cnn_expected (handtrack.h:160-173), host only: pose [17][7] and the TILE
 *                     camera [12] (the heat-map camera camsub(cam, 4) is formed inside) -> expected [2304]. */
int ht_cnn_train(ht_ctx *ctx, const float *inputs, const float *targets, int n, float alpha, float *mse_out);
int ht_cnn_get_weights(ht_ctx *ctx, float *w, size_t n);
int ht_expected_cnn(const float *pose, const float *cam, float *expected);
int ht_expected_cnn_full(const float *pose, const float *cam, float *expected, float *image_points /* [8][2], may be NULL */, float *vals /* [16], may be NULL */);

/* ---- training samples and training on the device (an addition: train-cnn.cpp runs its loop on the host) -----------------
 * ht_expected_cnn_batch  replaces  GatherHandExpectedCNN(pose, camsub(cam, 4)) (handtrack.h:160-173) for B frames, on the device: poses [B][nb][7]
 *                        (nb = the context's bone count, >= 17: bones 1, 4, 6, 7, 9, 10, 12, 13, 15, 16 are read; HT_ERR_ARG below 17), the TILE cameras
 *                        cams [B][12] -> expected [B][2304], image_points [B][8][2] and vals [B][16] (both may be NULL).  Bit-identical to
 *                        ht_expected_cnn_full frame by frame for every pose whose eight landmark projections are finite.  With flags =
 *                        HT_LABELS_SEGMENT_FRAME the poses are first re-expressed as cam.pose.inverse() * p and the camera's pose taken as the
 *                        identity (train-cnn.cpp:31-50 `compress`): the tiles and cameras of ht_segment_vr with the raw poses give train-cnn's labels.
 *                        B is not bounded by max_batch (no tracker slot; the call stages through a device buffer it grows on demand); B = 0 does
 *                        nothing.  HT_ERR_STATE for a context without a hand model.
 * ht_expected_cnn_dev    the same on device buffers, asynchronous on `stream`; d_expected must be 16-byte aligned.
 * ht_cnn_input_dev       replaces  the net's input of a segment, handtrack.h:700 (1 - (d - 0.1) / (drangey - 0.1) clamped to [0, 1], drangey from the
 *                        context's parameters), for B 64x64 tiles d_tiles [B][4096] with cams [B][12] (depth_scale) -> d_cnn_in [B][4096]; equal to
 *                        ht_stage_prepare's cnn_in.  B is not bounded by max_batch.  d_tiles and d_cnn_in must be 16-byte aligned (HT_ERR_ARG).
 * ht_cnn_train_dev       replaces  CNN::Train (cnn.h:558-580) for n_steps samples drawn from device pools d_inputs [n_pool][4096] and d_targets
 *                        [n_pool][2304]: step k trains on sample order[k] (`order` is a HOST array; every index is checked against [0, n_pool)
 *                        before anything is launched, HT_ERR_ARG otherwise), or on sample k when order is NULL (n_steps <= n_pool).  d_mse
 *                        [n_steps] (optional) = the value Train returns for each step.  Asynchronous on `stream`; the weights change in that
 *                        stream's order, and the caller orders other streams' use of the net after it.  Uses the context's training scratch only.
 *                        ht_cnn_train is an upload followed by this call. */
int ht_expected_cnn_batch(ht_ctx *ctx, const float *poses, const float *cams, int B, int flags, float *expected, float *image_points, float *vals);
int ht_expected_cnn_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int B, int flags, float *d_expected, float *d_image_points, float *d_vals, void *stream);
int ht_cnn_input_dev(ht_ctx *ctx, const uint16_t *d_tiles, const float *d_cams, int B, float *d_cnn_in, void *stream);
int ht_cnn_train_dev(ht_ctx *ctx, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, float alpha, float *d_mse, void *stream);

/* ---- mini-batch training (an addition: the reference trains one sample at a time) --------------------------------------------
 * One step on samples s_0..s_{batch-1} from weights w is  w' = w - alpha * SUM_b g_b(w),  g_b(w) = what CNN::Train(x_b, t_b, alpha) (cnn.h:558-580)
 * subtracts from every weight, divided by alpha, ALL taken at the same w.  It is a SUM, not a mean: alpha keeps the reference's per-sample meaning, and a
 * caller who wants the mean gradient passes alpha / batch.  batch = 1 is CNN::Train (to rounding: another summation order than ht_cnn_train).  A sample
 * that appears twice in a step counts twice.  Every reduction has a fixed order: the same call on the same weights gives the same bits.
 * ht_cnn_train_batch_dev   n_steps steps on device pools d_inputs [n_pool][4096], d_targets [n_pool][2304]: step k trains on samples
 *                          order[k*batch .. (k+1)*batch) (`order` is a HOST array of n_steps*batch indices, all checked against [0, n_pool) before
 *                          anything is launched), or on samples k*batch + b when order is NULL (n_steps*batch <= n_pool).  d_mse [n_steps*batch]
 *                          (optional) = the value Train returns for each sample at its step's weights, sum E^2 / 2304.  1 <= batch <=
 *                          HT_TRAIN_MAX_BATCH, any value.  Asynchronous on `stream` under ht_cnn_train_dev's rules: the weights change in stream
 *                          order, the call ends with the refresh of the inference kernels' packed copies, ht_cnn_get_weights waits for it.  A
 *                          refused call (HT_ERR_ARG, the message names the argument; also without weights of the 64x64-input net: the larger one is trained by the sized forms below) leaves the context as it was.
 * ht_cnn_train_batch       the same on host arrays inputs [n][4096], targets [n][2304], mse_out [n] (optional): an upload, then steps of `batch`
 *                          samples in order; when n is no multiple of batch the remainder forms a last, smaller step.
 *                          Staged through the same buffer as ht_cnn_train (n * 6401 floats, kept by the context until ht_destroy).
 * ht_debug_train_batch_buffers  test aid: the latest step's per-sample tensors, n = that step's sample count (HT_ERR_ARG otherwise): a3 [n][3600],
 *                          a6 [n][2304], a8 [n][2048], e9 [n][2304], e7 [n][2048], e6 [n][2304], e3 [n][3600] (conv2's backward, summed over its groups). */
#define HT_TRAIN_MAX_BATCH 256
int ht_cnn_train_batch_dev(ht_ctx *ctx, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, float alpha, float *d_mse, void *stream);
int ht_cnn_train_batch(ht_ctx *ctx, const float *inputs, const float *targets, int n, int batch, float alpha, float *mse_out);
int ht_debug_train_batch_buffers(ht_ctx *ctx, int n, float *a3, float *a6, float *a8, float *e9, float *e7, float *e6, float *e3);

/* ---- mini-batch training of either net ---------------------------------------------------------------------------------------------
 * The calls above with the net's input side: side = 64 IS the call above (same launches, same bits), side = 128 trains the 128x128-input net of
 * ht_cnn_load_weights_sized under the same contract word for word (w' = w - alpha * SUM_b g_b(w), the same checks before anything is launched or
 * grown, the same order rules, fixed summation orders, no floating-point atomics); any other side is HT_ERR_ARG.  Only the mini-batch step trains the
 * larger net: ht_cnn_train / ht_cnn_train_dev and the C++ CNN class stay 64-only, and a batch of one through the sized call is CNN::Train to rounding.
 * The two nets of a context are independent: training one leaves the other's weights and outputs as they were.
 * ht_cnn_train_batch_sized_dev  side 128: pools d_inputs [n_pool][16384], d_targets [n_pool][2304]; HT_ERR_ARG if the context holds no weights of that
 *                          net.  Ends with the refresh of that net's packed copies.  Its arena (about 370 KB a sample) is allocated by the first such call.
 * ht_cnn_train_batch_sized  the host-array form, staged through the same buffer as ht_cnn_train: n * (side*side + 2305) floats at the largest call.
 * ht_cnn_get_weights_sized  CNN::saveb for either net: n = HT_CNNB_COUNT or HT_CNNB128_COUNT; waits for training on a caller's stream.
 * ht_debug_train_batch_buffers_sized  side 128: a3 / e3 [n][15376], a6 / e6 [n][12544], a8 / e7 [n][2048], e9 [n][2304]; n = the latest step's sample
 *                          count of that net.
 * ht_cnn_input_sized_dev   handtrack.h:700 for B side x side tiles d_tiles [B][side*side] -> d_cnn_in [B][side*side]; side 128 is what ht_update_direct_*
 *                          feeds the net with.  The alignment rule of ht_cnn_input_dev.
 * HT_LABELS_SIDE128        flag of ht_expected_cnn_batch / _dev (may be combined with HT_LABELS_SEGMENT_FRAME): the heat-map camera is camsub(cam, 8), so
 *                          that a 128x128 tile gives 16x16 maps again.  Bit-identical to the call without it on a camera whose focal lengths and
 *                          principal point are halved. */
int ht_cnn_train_batch_sized_dev(ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, float alpha, float *d_mse, void *stream);
int ht_cnn_train_batch_sized(ht_ctx *ctx, int side, const float *inputs, const float *targets, int n, int batch, float alpha, float *mse_out);
int ht_cnn_get_weights_sized(ht_ctx *ctx, int side, float *w, size_t n);
int ht_debug_train_batch_buffers_sized(ht_ctx *ctx, int side, int n, float *a3, float *a6, float *a8, float *e9, float *e7, float *e6, float *e3);
int ht_cnn_input_sized_dev(ht_ctx *ctx, int side, const uint16_t *d_tiles, const float *d_cams, int B, float *d_cnn_in, void *stream);

/* ---- the mini-batch gradient as a buffer, and optimiser steps over it (csrc/ht_optim.hip) --------------------------
 * The calls above fuse w' = w - alpha * SUM_b g_b(w) into the kernels that form the sums.  These write the sums out and step from them, for either net
 * (side 64 or 128, anything else HT_ERR_ARG), so that a caller can accumulate over more than HT_TRAIN_MAX_BATCH samples, clip, reduce G over ranks, or
 * step with momentum or Adam.  The calls above, their launches and their bits are unchanged.
 * ht_cnn_grad_batch_sized_dev  G = (accumulate ? G : 0) + SUM_b g_b(w) over samples order[0..batch) of the pools (order NULL: samples 0..batch-1), g_b as above.
 *                          The weights are NOT touched.  G holds one float per weight in .cnnb order (the order CNN::saveb writes the weights in), one buffer per
 *                          net, owned by the context and allocated by the first call.  1 <= batch <= HT_TRAIN_MAX_BATCH; the checks of
 *                          ht_cnn_train_batch_sized_dev run before anything grows or launches.  d_mse [batch] optional.  Fixed summation orders, no
 *                          floating-point atomics; accumulate != 0 adds the fresh sums to G with one float addition per element.  HT_ERR_STATE for
 *                          accumulate before a buffer exists.  Asynchronous on `stream`.  The forward pass, the soft-max and the backward-data launches are
 *                          those of ht_cnn_train_batch_sized_dev, so ht_debug_train_batch_buffers_sized reads this call's per-sample tensors too.
 * ht_cnn_grad_batch_sized  the same on host arrays inputs [n][side*side], targets [n][2304], mse_out [n] (optional), n <= HT_TRAIN_MAX_BATCH, one gradient call.
 * ht_cnn_grad_get_sized / _set_sized  G to / from a host array, n = HT_CNNB_COUNT or HT_CNNB128_COUNT (HT_ERR_ARG otherwise); both wait for the work in flight.
 *                          set allocates the buffer if there is none; get without one is HT_ERR_STATE.
 * ht_cnn_grad_ptr_sized    the device buffer itself and its length, for a caller's own reduction (in stream order with the calls around it); HT_ERR_STATE
 *                          before a buffer exists.
 *
 * ht_opt / ht_opt_default  the optimiser a step applies.  ht_opt_default (host only) fills kind, lr 0.001, momentum 0.9, beta1 0.9, beta2 0.999, eps 1e-8,
 *                          weight_decay 0, decoupled_decay 0, grad_scale 1, clip_norm 0 (= off); HT_ERR_ARG for an unknown kind or a NULL o.
 * ht_cnn_opt_step_sized_dev  one step over all weights of the net from its G.  fp32, one IEEE operation per written operation, in this order (gs = grad_scale,
 *                          c = the clip factor):
 *                              g = (G[i] * gs) * c
 *                            Decay applies to W1 W2 W3 W4 only, never to B1..B4.
 *                            Coupled decay (decoupled_decay = 0, weight_decay != 0), on the W ranges:   g = g + weight_decay * w
 *                            SGD        w' = w - lr * g
 *                            MOMENTUM   m' = momentum * m + g,   w' = w - lr * m'
 *                            NESTEROV   the same m',             w' = w - lr * (g + momentum * m')
 *                            ADAM       t' = t + 1
 *                                       m' = beta1 * m + omb1 * g
 *                                       v' = beta2 * v + (omb2 * g) * g
 *                                       u = (m' / bc1) / (sqrtf(v' / bc2) + eps)
 *                                       with decoupled_decay, on the W ranges:   u = u + weight_decay * w
 *                                       w' = w - lr * u
 *                                       omb1 = 1.0f - beta1, omb2 = 1.0f - beta2 in float; bc1 = (float)(1.0 - pow((double)beta1, t')), likewise bc2.
 *                            Clip       norm = sqrt(SUM_i ((double)G[i] * (double)gs)^2), float64, in a fixed order;
 *                                       c = norm > clip_norm ? (float)((double)clip_norm / norm) : 1.0f.  clip_norm = 0: c = 1.0f, no norm is formed.
 *                          m and v start as zeros and are allocated on first need of a kind that keeps them; t counts the net's Adam steps (the other kinds
 *                          leave it).  Changing kind between steps is allowed and uses whatever state is there.  The step ends with the refresh of the
 *                          inference kernels' packed copies, so ht_cnn_get_weights_sized and ht_cnn_eval_* see the stepped weights.  Asynchronous on `stream`
 *                          (the factor reaches the step on the device).  o is checked completely before anything launches: kind; every field finite;
 *                          lr >= 0; momentum, beta1, beta2 in [0, 1); eps > 0 for Adam; clip_norm >= 0; decoupled_decay 0 or 1, and 1 only with Adam.  A
 *                          violation is HT_ERR_ARG with the field's name in ht_last_error and leaves the context as it was.  HT_ERR_STATE without a gradient buffer.
 * ht_cnn_opt_reset_sized   m = v = 0, t = 0.
 * ht_cnn_opt_state_get_sized / _set_sized  m, v [n] and t to / from the host; any of m, v, t (get) or m, v (set) may be NULL; n as for G.  A moment that no
 *                          step has needed yet reads as zeros; set allocates what it is given.  t >= 0.
 * ht_cnn_opt_last_sized    the latest step's norm and clip factor; waits for it.  A step that did not clip formed no norm: -1 and 1.0f.  HT_ERR_STATE before a step.
 * ht_cnn_train_opt_sized_dev  n_steps optimiser steps, each preceded by accum >= 1 gradient calls of `batch` samples, the first with accumulate = 0.  order holds
 *                          n_steps * accum * batch indices, all checked before anything is launched (NULL: samples 0, 1, ...; that many must exist).
 *                          d_mse [n_steps * accum * batch] optional.  It is exactly that sequence of ht_cnn_grad_batch_sized_dev and
 *                          ht_cnn_opt_step_sized_dev calls: the same launches, the same bits. */
enum { HT_OPT_SGD = 0, HT_OPT_MOMENTUM = 1, HT_OPT_NESTEROV = 2, HT_OPT_ADAM = 3 };
typedef struct ht_opt { int kind; float lr, momentum, beta1, beta2, eps, weight_decay; int decoupled_decay; float grad_scale; float clip_norm; } ht_opt;
int ht_cnn_grad_batch_sized_dev(ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int batch, int accumulate, float *d_mse, void *stream);
int ht_cnn_grad_batch_sized(ht_ctx *ctx, int side, const float *inputs, const float *targets, int n, int accumulate, float *mse_out);
int ht_cnn_grad_get_sized(ht_ctx *ctx, int side, float *g, size_t n);
int ht_cnn_grad_set_sized(ht_ctx *ctx, int side, const float *g, size_t n);
int ht_cnn_grad_ptr_sized(ht_ctx *ctx, int side, float **d_g, size_t *n);
int ht_opt_default(int kind, ht_opt *o);
int ht_cnn_opt_step_sized_dev(ht_ctx *ctx, int side, const ht_opt *o, void *stream);
int ht_cnn_opt_reset_sized(ht_ctx *ctx, int side);
int ht_cnn_opt_state_get_sized(ht_ctx *ctx, int side, float *m, float *v, size_t n, int *t);
int ht_cnn_opt_state_set_sized(ht_ctx *ctx, int side, const float *m, const float *v, size_t n, int t);
int ht_cnn_opt_last_sized(ht_ctx *ctx, int side, double *grad_norm, float *clip_factor);
int ht_cnn_train_opt_sized_dev(ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, int accum, const ht_opt *o, float *d_mse, void *stream);

/* ---- a hand model that is not being tracked (host only, no device needed) ---------------------------------------------------
 * The reference's applications keep a second PhysModel to pose, draw and ray-cast their synthetic input
 * (`PhysModel fakehand = LoadHandModel();` synthetic-tracker.cpp:94, FakeDepth :69-76).
 * ht_model_open      replaces  PhysModel::PhysModel(const char *jsonfile) (physmodel.h:444-475) and, with hand_tweaks != 0, LoadHandModel()
 *                    (handtrack.h:347-366); a model baked by ht_model_bake is accepted too.  *out is set even on failure (ht_model_error), close it.
 * ht_model_body      per body: vertex / hull-triangle / plane counts, centre of mass in rig space (RigidBody::com) and the rest pose.
 * ht_model_body_mesh the body's collision vertices [nverts][3] (centre-of-mass frame) and hull triangles [ntris][3]: what PhysModel::GetMeshes()
 *                    hands to a renderer (physmodel.h:295-303), posed by the caller.
 * ht_model_hitcheck  replaces  PhysModel::HitCheck(v0, v1) (physmodel.h:287-294) for bodies at poses [nb][7]: nearest hit of the segment with the
 *                    bodies' hulls; *body = -1 and impact = v1 when nothing is hit. */
typedef struct ht_model ht_model;
int ht_model_open(const char *path, int hand_tweaks, ht_model **out);
int ht_model_close(ht_model *m);
const char *ht_model_error(const ht_model *m);
int ht_model_counts(const ht_model *m, int *n_bodies, int *n_joints);
int ht_model_body(const ht_model *m, int body, int *nverts, int *ntris, int *nplanes, float *com3, float *rest_pose7);
int ht_model_body_mesh(const ht_model *m, int body, float *verts, int *tris);
int ht_model_body_sdmesh(const ht_model *m, int body, int *nverts, float *verts);      /* PhysModel::sdmeshes (physmodel.h:258): the twice-subdivided control cage flat-shaded, three corner positions per triangle in the bone's rig frame; verts NULL: the count only */
int ht_model_hitcheck(const ht_model *m, const float *poses, const float *v0, const float *v1, float *impact3, float *normal3, int *body);
/* The ray cast against the subdivision surface (an addition: the application draws these meshes with OpenGL and reads the depth buffer back,
 * synthetic-tracker.cpp:164-165; this is the software statement of that source, as FakeDepth is for the hulls).
 * ht_model_hitcheck_mesh  for bodies at centre-of-mass poses [nb][7]: every triangle of sdmeshes[b] (ht_model_body_sdmesh, stored order) is tested with
 *                    PolyHitCheck (geometric.h:263-273) on the whole segment v0 -> v1 in the frame of its mesh pose Pose{pos_b - qrot(q_b, com_b), q_b}
 *                    (GetMeshes, physmodel.h:297-298), with its PolyPlane (geometric.h:247-260) made once per model in float: a candidate iff d0 > 0,
 *                    d1 < 0 and the three determinants are >= 0.  The candidate with the smallest d0 / (d0 - d1) wins, the first in (body, triangle)
 *                    order on a tie; impact = U_b * (a + (c - a) * d0 / (d0 - d1)), normal = qrot(q_b, plane.xyz).  Nothing hit: *body = *tri = -1,
 *                    impact = v1.  The segment is never shortened, so a triangle's candidacy depends on no other triangle.
 * ht_model_render_mesh    one w x h frame of it: pixel (x, y) = (uint16)(impact.z / depth_scale) for the segment from the origin to
 *                    deprojectz((x + pixel_offset, y + pixel_offset), far) (misc_image.h:48); a plain loop over pixels, bodies and triangles, the
 *                    definition ht_render_mesh_depth equals bit for bit.  pixel_offset in [0, 1]: 0 is FakeDepth's convention, 0.5 where OpenGL samples.
 *                    body (optional) [h][w], -1 = background.  cam12: focal, principal point and depth_scale are used.
 * ht_model_scale     replaces  PhysModel::scale (physmodel.h:304-319) for this view's geometry (hull vertices, plane offsets, sdmeshes, centres of mass),
 *                    by the function ht_scale applies to a context's model: a host model and a context scaled alike render the same bits. */
int ht_model_hitcheck_mesh(const ht_model *m, const float *poses, const float *v0, const float *v1, float *impact3, float *normal3, int *body, int *tri);
int ht_model_render_mesh(const ht_model *m, const float *poses, const float *cam12, int w, int h, float far, float pixel_offset, uint16_t *depth, int8_t *body);
int ht_model_scale(ht_model *m, float s);
/* The same meshes through a forward z-buffer rasteriser (an addition; what the application's GL path does, synthetic-tracker.cpp:164-182, stated in software with a
 * definition of its own, not the ray cast's: work grows with triangles plus covered pixels, not with pixels times triangles).
 * ht_model_raster_mesh    one w x h frame.  For body b at centre-of-mass pose (pos, q), R = qmat(q), up = pos - R com_b, every triangle (v0, v1, v2) of sdmeshes[b] in
 *                    stored order, all in float with one rounding per operation:
 *                      corners   w_i = up + R v_i; the triangle is dropped if any w_i.z < HT_RASTER_NEAR or any coordinate is not finite
 *                      screen    sx_i = (fx (w_i.x / w_i.z) + px) - pixel_offset, sy_i likewise, so pixel (x, y)'s sample is the integer point (x, y); dropped if any
 *                                |sx_i| or |sy_i| >= 2^20 or is not finite; X_i = rint(256 sx_i), Y_i = rint(256 sy_i), round-half-even, as integers
 *                      facing    A2 = (X1-X0)(Y2-Y0) - (X2-X0)(Y1-Y0) in exact integers; kept iff A2 < 0 (with y downwards the side PolyHitCheck's d0 > 0 keeps)
 *                      coverage  pixel (x, y) is inside iff (X_j-X_i)(256y-Y_i) - (Y_j-Y_i)(256x-X_i) <= 0 for the edges i -> j = 0->1, 1->2, 2->0, in exact integers:
 *                                edges are inclusive on both sides, shared corners are bit-equal in sdmeshes, so a closed body has no cracks
 *                      depth     N = cross(w1-w0, w2-w0), k = dot(N, w0); rx = ((x + pixel_offset) - px) / fx, ry likewise; den = (N.x rx + N.y ry) + N.z,
 *                                z = k / den, c = z / depth_scale; a candidate iff c is finite, HT_RASTER_NEAR <= z < far and 0 <= c < 65536; its count is (uint16)c
 *                      winner    the smallest count, the first in (body, triangle) order on equal counts; body = that body.  No candidate: (uint16)(far /
 *                                depth_scale) and body -1, as in the ray cast, so frames of pixel_offset 0 and far 4 are interchangeable with ht_render_depth's.
 *                    No perspective clipping: a triangle that crosses the near distance is dropped.  Arguments as ht_model_render_mesh.  Against the ray cast evaluated
 *                    in double, on the same pixels: counts differ by at most 1 where both pick the same triangle (DESIGN section 35 has the measured shares). */
#define HT_RASTER_NEAR 0.01f   /* metres */
int ht_model_raster_mesh(const ht_model *m, const float *poses, const float *cam12, int w, int h, float far, float pixel_offset, uint16_t *depth, int8_t *body);
/* Scenes of several hands, each right or left, in one z-buffer over an optional background frame (an addition).
 * ht_model_raster_scene   one w x h frame of H instances.  poses [H][nb][7]: centre-of-mass poses as ht_model_raster_mesh takes them; a left instance's are the left
 *                    hand's as this camera sees it (what ht_mirror_poses makes of canonical ones).  hands [H] (uint8): HT_SCENE_RIGHT, HT_SCENE_ABSENT (the instance is
 *                    skipped), any other value left ("nonzero = left", as everywhere); NULL: all right.  cam12, far, pixel_offset as ht_model_raster_mesh.
 *                      layer     of a right instance i: ht_model_raster_mesh's frame of poses[i] through cam12, word for word.  Of a left one: the same definition applied
 *                                to mirror(poses[i]) (the sign bits of px, qy, qz flipped) with the principal point cx' = ((float)(w-1) - cx) + (pixel_offset +
 *                                pixel_offset), the second addition skipped when pixel_offset == 0 (cx' then has ht_mirror_cams' bits); the layer is read at column
 *                                w-1-x.  Pixel x samples x + o and its mirror pixel w-1-x samples w-1-x + o, hence w-1 + 2o - cx: the layer equals the frame of the
 *                                x-negated meshes (ht_model_mirror) through cam12, which the plain ht_mirror_cams camera misses by one pixel at o = 0.5
 *                      winner    among the instances whose layer covers the pixel (body != -1): the smallest count, the lowest instance index on equal counts; within an
 *                                instance the (body, triangle) order of ht_model_raster_mesh
 *                      bg        [h][w] (optional): the winner is written iff bg == 0 or count <= bg, otherwise depth = bg and hand = body = -1; no covering instance:
 *                                depth = bg, zeros included.  Without bg: (uint16)(far / depth_scale), as ht_model_raster_mesh.  bg == depth exactly composes in place
 *                      outputs   depth [h][w]; optional: hand [h][w] the winner's instance index, body [h][w] its body (both -1 where no hand is written), visible [H] the
 *                                number of pixels each instance is written on
 *                    H in [1, HT_SCENE_MAX_HANDS] (HT_ERR_ARG); H times the model's mesh triangles <= 65535 (HT_ERR_STATE; the stock hands have 6016 and 8896); buffers
 *                    that overlap, other than bg == depth, are HT_ERR_ARG; the other arguments as ht_model_raster_mesh. */
#define HT_SCENE_RIGHT 0
#define HT_SCENE_ABSENT 255
#define HT_SCENE_MAX_HANDS 4
int ht_model_raster_scene(const ht_model *m, const float *poses, const uint8_t *hands, int H, const float *cam12, int w, int h, float far, float pixel_offset,
                          const uint16_t *bg, uint16_t *depth, int8_t *hand, int8_t *body, int32_t *visible);

/* ---- segmentation: the step before the tracker for full-size frames --------------------------------------------------
 * ht_segment_vr       replaces  Image<unsigned short> HandSegmentVR(const Image<unsigned short> &depth, int entry_options = 0xF,
 *                     float2 wrange = {0.1f, 0.65f}, float diam = 0.17f) (handtrack.h:280-344) for B frames of w x h pixels:
 *                     depth [B][h*w], cams [B][12] -> tiles [B][64*64] and the segment cameras cams_out [B][12] (focal, principal
 *                     (32,32), depth_scale, pose = (0, rotation)), ready for ht_update_sync.  A 64x64 frame is passed through.
 *                     Frames up to 320x240 (the reference's camera), dimensions multiples of 4.
 * ht_segment_vr_dev   the same on device buffers, asynchronous on `stream`. */
int ht_segment_vr(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, int B, int entry_options, float wrange_lo, float wrange_hi, float diam,
                  uint16_t *tiles, float *cams_out);
int ht_segment_vr_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, int entry_options, float wrange_lo, float wrange_hi, float diam,
                      uint16_t *d_tiles, float *d_cams_out, void *stream);
/* ht_segment_vr_supported  the size rule of the sized calls, in one place and without a context: HT_OK for side 64 or 128 and a frame with w, h >= 8, both
 *                     multiples of 4, and (w/4)*(h/4) <= 19200 (640x480, the SR300's native frame, or any other shape with that many quarter-size
 *                     pixels: the two DownSampleMin of handtrack.h:285-286 stay in on-chip memory), or a side x side frame; HT_ERR_ARG otherwise.
 * ht_segment_vr_sized      HandSegmentVR (handtrack.h:280-344) with the side of its 64x64 tile a parameter: dstcam (:338-340) becomes
 *                     ({side,side}, avgdepth*side/diam, {side/2,side/2}) and SampleD (:342, misc_image.h:154-162) runs over side x side pixels; nothing else
 *                     of the function sees the side.  tiles [B][side*side]; the segment camera of side 128 is that of side 64 with focal doubled and
 *                     principal (64,64), bit for bit.  A side x side frame is passed through (:283-284 for the net's own size).  Needs no weights.
 *                     side 64 runs the very kernel of ht_segment_vr and returns its bits.  HT_ERR_ARG for what ht_segment_vr_supported refuses.
 * ht_segment_vr_sized_dev  the same on device buffers, asynchronous on `stream`. */
int ht_segment_vr_supported(int w, int h, int side);
int ht_segment_vr_sized(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, int B, int entry_options, float wrange_lo, float wrange_hi, float diam,
                        uint16_t *tiles, float *cams_out);
int ht_segment_vr_sized_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, int entry_options, float wrange_lo, float wrange_hi, float diam,
                            uint16_t *d_tiles, float *d_cams_out, void *stream);

/* ---- synthetic depth frames (an addition: the reference renders its fake hand on the host) ---------------------------
 * ht_render_depth     replaces  the software_rasterizer branch of synthetic-tracker.cpp:182, FakeDepth (:69-76), for B frames: pixel (x, y) of
 *                     frame f is (uint16)(PhysModel::HitCheck({0,0,0}, deprojectz((x, y), far)).impact.z / depth_scale) (physmodel.h:287-294,
 *                     geometric.h:275-302, misc_image.h:48) with the context's hand model (as ht_create built it and ht_scale left it) at the
 *                     centre-of-mass poses poses [B][nb][7] (PhysModel::SetPose, :435).  cams [B][12]: focal, principal point and depth_scale are
 *                     used; the camera's pose is not -- the ray starts at the origin of the poses' frame, as in FakeDepth.  Bit-identical to the
 *                     host's HitCheck.  depth [B][h][w]; body (optional, [B][h][w]) = ModelHitInfo::rb, -1 for background.  w, h in [1, 4096],
 *                     far > 0 (the application uses 4); B is not bounded by the context's max_batch (no tracker slot is used; the call stages
 *                     through device buffers it grows on demand); B = 0 does nothing.  HT_ERR_STATE for a context without a hand model.
 * ht_render_depth_dev the same on device buffers, asynchronous on `stream`. */
int ht_render_depth(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, float far, int B, uint16_t *depth, int8_t *body);
int ht_render_depth_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int w, int h, float far, int B, uint16_t *d_depth, int8_t *d_body, void *stream);
/* ht_render_mesh_depth     the hand's subdivision surface instead of its hulls (GetMeshes(true), the application's default depth source,
 *                     synthetic-tracker.cpp:164-165): ht_model_render_mesh for B frames, bit-identical to it, with the context's model as ht_create
 *                     built it and ht_scale left it.  poses [B][nb][7], cams [B][12], depth [B][h][w], body (optional) [B][h][w] as ht_render_depth;
 *                     w, h in [1, 4096], far > 0, pixel_offset finite and in [0, 1] (HT_ERR_ARG otherwise).  The application's GL frames are
 *                     pixel_offset 0.5, far 0.85; frames interchangeable with ht_render_depth's are pixel_offset 0, far 4.  B is not bounded by
 *                     max_batch; B = 0 does nothing.  HT_ERR_STATE for a context without a hand model, or whose model file holds no meshes.
 * ht_render_mesh_depth_dev the same on device buffers, asynchronous on `stream`. */
int ht_render_mesh_depth(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, float far, float pixel_offset, int B, uint16_t *depth, int8_t *body);
int ht_render_mesh_depth_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int w, int h, float far, float pixel_offset, int B, uint16_t *d_depth, int8_t *d_body, void *stream);
/* ht_raster_mesh_depth     the same meshes rasterised: ht_model_raster_mesh (above, where the definition is) for B frames, bit-identical to it for depth and body,
 *                     with the context's model as ht_create built it and ht_scale left it.  Shapes, argument rules and return codes are ht_render_mesh_depth's;
 *                     also HT_ERR_STATE for a model of 65535 or more mesh triangles (the z-buffer keeps a 16-bit triangle index; the stock hands have 6016 and
 *                     8896).  Deterministic: the z-buffer is filled with atomic minima of (count, triangle), so the order of arrival does not matter.
 * ht_raster_mesh_depth_dev the same on device buffers, asynchronous on `stream`. */
int ht_raster_mesh_depth(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, float far, float pixel_offset, int B, uint16_t *depth, int8_t *body);
int ht_raster_mesh_depth_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int w, int h, float far, float pixel_offset, int B, uint16_t *d_depth, int8_t *d_body, void *stream);
/* ht_raster_scene_depth    ht_model_raster_scene (above, where the definition is) for B frames, bit-identical to it on every output, with the context's model as
 *                     ht_create built it and ht_scale left it: poses [B][H][nb][7], hands [B][H] (optional), cams [B][12], bg [B][h][w] (optional) -> depth [B][h][w] and,
 *                     each optional, hand [B][h][w], body [B][h][w], visible [B][H].  One z-buffer pass: every band of a frame is cleared and written once, whatever H.
 *                     Argument rules and return codes are ht_raster_mesh_depth's; in addition H outside [1, HT_SCENE_MAX_HANDS] is HT_ERR_ARG, H times the model's mesh
 *                     triangles above 65535 HT_ERR_STATE, and any overlap among the buffers HT_ERR_ARG, except bg == depth exactly (in-place composition: each pixel is
 *                     read and then written by one thread).  B is not bounded by max_batch; B = 0 does nothing.  Deterministic: atomic minima of (count, instance,
 *                     triangle), integer atomic adds for visible.
 * ht_raster_scene_depth_dev the same on device buffers (hands included), asynchronous on `stream`; it zeroes visible on the stream before the kernel adds to it. */
int ht_raster_scene_depth(ht_ctx *ctx, const float *poses, const uint8_t *hands, int H, const float *cams, int w, int h, float far, float pixel_offset, int B, const uint16_t *bg,
                          uint16_t *depth, int8_t *hand, int8_t *body, int32_t *visible);
int ht_raster_scene_depth_dev(ht_ctx *ctx, const float *d_poses, const uint8_t *d_hands, int H, const float *d_cams, int w, int h, float far, float pixel_offset, int B, const uint16_t *d_bg,
                              uint16_t *d_depth, int8_t *d_hand, int8_t *d_body, int32_t *d_visible, void *stream);

/* ---- joint coordinates (an addition: the reference decomposes every joint on every solver pass and never hands the result out) ----
 * Joint j of the model (parent body rbi0 at orientation q0, child rbi1 at q1, jointframe F, anchors p0 / p1) has the coordinates c = (s.x, s.y, t.z) of
 * ConstrainAngularRangeW (third_party/physics.h:351-393): Jb = q0 F, Jf = q1, both times cb = normalize(0,-1,0,1) for a "swapped" joint (:358-362: rangemin.x ==
 * rangemax.x == 0 and rangemin.z < rangemax.z; its limits become (min.z, min.y, 0), (max.z, max.y, 0)); r = conj(Jb) Jf, s = quat_from_to((0,0,1), qzdir(r))
 * (geometric.h:319-328), t = conj(s) r.  No sign is canonicalised: t.z follows the sign of the stored quaternions, as in the reference.  An angle in the
 * reference's degrees is 2 asin(c) 180 / 3.14.  All arrays are fp32; poses [B][nb][7] are position + quaternion xyzw per body, user poses (GetPoseUser
 * physmodel.h:434, what the update calls return) unless flags has HT_JOINTS_COM_POSES: then centre-of-mass poses (GetPose, what ht_render_depth takes), on
 * input and on output, the root included.  B is not bounded by max_batch; B = 0 does nothing; every check runs before anything grows or launches;
 * HT_ERR_STATE for a context without a hand model.
 * ht_model_joint_limits  host only, no context: the values of c that satisfy the reference's rows (:367-391), lo / hi [nj][3], swapped [nj] (any may be NULL).
 *                     With jmin = deg * 3.14f / 180.0f: x locked at sinf(jmin.x / 2), or in [sinf(jmin.x / 2), sinf(jmax.x / 2)], or, for a range of
 *                     360 * 3.14 / 180 or more (no rows), -inf .. +inf; y locked at jmin.y IN RADIANS (:378), or ranged by sines; z locked at 0 whatever
 *                     jmin.z is (:386), or ranged by sines.  A context computes the same table once at model load; ht_scale leaves it alone.
 * ht_joint_coords     poses [B][nb][7] -> coords [B][nj][3] and (optional) gaps [B][nj] = |PoseUser(rbi0) p0 - PoseUser(rbi1) p1|, the distance
 *                     GetLinearConstraints / FixPositions close (physmodel.h:328-334, 404-408): a per-joint tracking-quality figure.
 * ht_joint_pose       forward kinematics, FixOrientations / FixPositions top down (physmodel.h:357-408): roots [B][7] (body 0's pose) and coords [B][nj][3] ->
 *                     poses [B][nb][7].  Joints in model order: s = (cx, cy, 0, sqrt(max(0, 1 - cx cx - cy cy))), t = (0, 0, cz, sqrt(max(0, 1 - cz cz))),
 *                     q1 = normalize(q0 F [cb] s t [conj(cb)]), PositionUser1 = PoseUser0 p0 - q1 p1.  HT_ERR_STATE for a model whose joints are not in
 *                     top-down order from body 0 (both shipped models are).  The host form refuses non-finite coordinates, |c| > 1 and
 *                     cx cx + cy cy > 1 (HT_ERR_ARG); the device form cannot look and clamps them through the two max(0, .) above.
 *                     ht_joint_coords of the result gives coords back; the other way round the orientations come back where the twist quaternion of
 *                     the read-out has t.w >= 0 (a twist within 180 degrees between quaternions stored on the same side): with no sign canonicalised,
 *                     t.z alone does not tell t from its mirror image.
 * ht_sample_poses     B poses inside the model's joint limits: sample i, joint j, axis a takes u in [0, 1) from a counter-based hash of (seed, first_index + i,
 *                     j, a) (24 bits, exact in fp32; independent of B and of the launch), c = (lo + hi) / 2 + (u - 0.5) (hi - lo) spread, a locked axis its
 *                     lock value, an unbounded one +-sinf(90 deg / 2); then ht_joint_pose's walk in the same kernel.  Uniform in the coordinate, not the
 *                     angle.  spread in [0, 1] (HT_ERR_ARG otherwise).  coords [B][nj][3] is optional.  The poses respect every joint limit; they are not
 *                     checked for contact between fingers (run solver passes on them for that).
 *                     flags & HT_SAMPLE_ENHANCED applies HandModelEnhancements' couplings (handtrack.h:417-420, 434-440) as the tracker sees them, for hand
 *                     layouts (at least 17 bodies, fingers as chains of bones 5..16 on bone 1; HT_ERR_ARG otherwise): the x of each fingertip joint
 *                     (6, 9, 12, 15) is locked at sin of half of acos(clamp(dot(qzdir(q[b-2]), qzdir(q[b-1])), 0, 1)) * 180 / 3.14159f / 2 degrees taken
 *                     back to radians with 3.14f (both literals are the reference's), and a knuckle (joint 4, 7, 10, 13) whose finger is not "up" on the
 *                     built pose (dot(qydir(q[1]), qydir(q[bone])) > cos(40 * 3.14 / 180) fails) has its y set to 0 and is rebuilt once.
 * The *_dev forms take device buffers and are asynchronous on `stream`. */
#define HT_JOINTS_COM_POSES 1
#define HT_SAMPLE_ENHANCED 2
int ht_model_joint_limits(const ht_model *m, float *lo, float *hi, int *swapped);
int ht_joint_coords(ht_ctx *ctx, const float *poses, int B, int flags, float *coords, float *gaps);
int ht_joint_coords_dev(ht_ctx *ctx, const float *d_poses, int B, int flags, float *d_coords, float *d_gaps, void *stream);
int ht_joint_pose(ht_ctx *ctx, const float *roots, const float *coords, int B, int flags, float *poses);
int ht_joint_pose_dev(ht_ctx *ctx, const float *d_roots, const float *d_coords, int B, int flags, float *d_poses, void *stream);
int ht_sample_poses(ht_ctx *ctx, const float *roots, int B, uint64_t seed, uint64_t first_index, float spread, int flags, float *poses, float *coords);
int ht_sample_poses_dev(ht_ctx *ctx, const float *d_roots, int B, uint64_t seed, uint64_t first_index, float spread, int flags, float *d_poses, float *d_coords, void *stream);

/* ---- camera front end: the depth filters of RSCam::GetDepth (include/dcam.h:238-244) for raw sensor frames ------------------------------
 * Every real-time program of the reference feeds the tracker htk.update(dcam.GetDepth()); GetDepth filters the sensor's frame first.  All arithmetic is
 * integer, the constants are dcam.h's own (it assumes millimetre counts, dcam.h:180).
 * ht_sensor_out_dims    the size a filtered frame has: k = the number of halvings until w >> k <= max_width (dcam.h:205-206, 212-213), *w_out = w >> k,
 *                       *h_out = h >> k.  No context.  HT_ERR_ARG for what the filter refuses on sizes alone (below).
 * ht_sensor_filter      kind HT_SENSOR_IVY replaces  Image<unsigned short> RSCam::FilterIvy(unsigned short *dp) (dcam.h:209-226), SR300 / F200: output pixel
 *                       (x, y) = input pixel (x << k, y << k) (DownSampleFst k times, misc_image.h:81-94,136), the camera is cam / 2 k times (focal and
 *                       principal halved, depth_scale and pose kept, misc_image.h:62), then every output pixel equal to 0 becomes
 *                       (unsigned short)(4.0f / depth_scale), formed as the x86 build forms it: the float quotient, a truncating conversion to int32, its
 *                       low 16 bits.
 *                       kind HT_SENSOR_DS4 replaces  Image<unsigned short> RSCam::FilterDS4(unsigned short *dp) (dcam.h:174-208), R200: (1) d < 30 || ir < 8
 *                       -> 4096; (2) pixels i = 0 .. w*h-1 in raster order, skipping x < 2, x >= w-2, y < 2, y >= h-2: with has(s) = |p[i+s] - p[i]| < 10 ||
 *                       |p[i-s] - p[i]| < 10 in int, p[i] = 4096 AT ONCE unless has(1), has(w), has(2) and has(2w) all hold -- so p[i-1], p[i-2], p[i-w],
 *                       p[i-2w] are read as already rewritten; (3) with a background model, p[i] > background[i] -> 4096.  Bit-identical to that
 *                       sequential loop (csrc/ht_sensor.hip has the decomposition).
 *                       depth [B][h*w], ir [B][h*w] (DS4: required; Ivy: ignored), cams [B][12], background [B][h*w] (DS4 only, caller-owned, may be NULL)
 *                       -> depth_out [B][h_out*w_out], cams_out [B][12]: an ordinary input of ht_update_frames_* and ht_segment_vr*, which keep their own
 *                       checks (a 640x480 frame: the *_sized forms).  B is not bounded by max_batch (no tracker slot; the host form stages through a device buffer it grows on demand); B = 0
 *                       does nothing.  HT_ERR_ARG, checked before anything is launched or grown: a NULL required buffer; w or h < 1 or > 4096;
 *                       max_width < 1; Ivy with w or h not divisible by 2^k (the reference reads past the image there); DS4 with w > max_width (the
 *                       reference indexes the full-size frame with an IR image it has already halved, dcam.h:170-171,184; R200 streams 320x240); a
 *                       background with Ivy (its path has none); depth_out overlapping depth.
 * ht_sensor_filter_dev  the same on device buffers, asynchronous on `stream`.
 * ht_sensor_background  replaces  void RSCam::addbackground(const unsigned short *dp, unsigned short fudge = 3) (dcam.h:157-162) for B frames:
 *                       background[i] = min(background[i], (unsigned short)(dp[i] - fudge)), the subtraction in int, the cast wrapping; init != 0 treats
 *                       the old model as 4096 everywhere (what the first call's resize gives, dcam.h:159).  depth, background [B][h*w].
 * ht_sensor_background_dev  the same on device buffers, asynchronous on `stream`. */
#define HT_SENSOR_IVY 0
#define HT_SENSOR_DS4 1
int ht_sensor_out_dims(int kind, int w, int h, int max_width, int *w_out, int *h_out);
int ht_sensor_filter(ht_ctx *ctx, int kind, const uint16_t *depth, const uint8_t *ir, const float *cams, int w, int h, int B, int max_width, const uint16_t *background, uint16_t *depth_out, float *cams_out);
int ht_sensor_filter_dev(ht_ctx *ctx, int kind, const uint16_t *d_depth, const uint8_t *d_ir, const float *d_cams, int w, int h, int B, int max_width, const uint16_t *d_background, uint16_t *d_depth_out, float *d_cams_out, void *stream);
int ht_sensor_background(ht_ctx *ctx, const uint16_t *depth, int w, int h, int B, int fudge, int init, uint16_t *background);
int ht_sensor_background_dev(ht_ctx *ctx, const uint16_t *d_depth, int w, int h, int B, int fudge, int init, uint16_t *d_background, void *stream);

/* ---- raw camera frames from rendered depth (an addition: the reference has no sensor model) --------------------------------------------
 * ht_render_depth and ht_render_mesh_depth give perfect frames.  ht_sensor_simulate turns them into what a camera of either kind would hand to the filters
 * above: axial noise that grows with depth, silhouettes that fray (drop-outs and flying pixels), drop-outs at grazing angles, random holes, the R200's
 * disparity quantisation and an IR image -- the input ht_sensor_filter was written for.  Frames keep their size and their camera.  Reproducible from a seed.
 * All arithmetic is integer; an intermediate is int64 wherever a product can exceed 31 bits; `//` is floor division; `>>` is arithmetic on signed values.
 *
 * Random bits.  mix is the 64-bit mixing function of ht_sample_poses (csrc/ht_mix.hpp).  Frame f of a call is stream first_index + f (mod 2^64):
 *     key = mix(seed ^ ((first_index + f) * 0x9E3779B97F4A7C15))                    per frame
 *     H   = mix(key ^ ((i + 1) * 0xD6E8FEB86659FD93)),  i = y*w + x                 per pixel: one mix
 *     H2  = mix(H ^ 0xA0761D6478BD642F)                                             per pixel, only with an IR image
 *   fields of H:  ua = bits 0-15, t = bits 16-23, ub = bits 24-39, g = the sum of the four 6-bit fields at bits 40, 46, 52 and 58, minus 126 (mean 0, sd 36.95)
 *   fields of H2: dark = bits 0-2, gi = the sum of the two 6-bit fields at bits 8 and 14, minus 63
 *   A frame's output depends on (seed, first_index + f) and the frame alone, never on B, on the frame's position in the call or on the launch.
 * Axial noise.  s(d) = sigma0_256 + ((int64)sigma2 * d * d >> 20) is the sd in 1/256 count at depth d, and
 *     noise(d) = clamp(d + (s(d) * g + 4736) // 9472, 1, 65535)                     9472 = 256 * 37; the sd of the sum is sqrt((s/256)^2 * 1365/1369 + 1/12) counts
 * A count c is foreground iff c != 0 && c < far_count.  A foreground pixel p at (x, y), in this order:
 *   1  its neighbours are the 8-neighbours that lie in the image, in raster order (x-1,y-1) (x,y-1) (x+1,y-1) (x-1,y) (x+1,y) (x-1,y+1) (x,y+1) (x+1,y+1);
 *      v(q) = q if q is foreground, else fly_bg_count; diff(q) = |v(q) - p|
 *   2  it is an edge pixel iff some diff(q) > edge_step; its far neighbour is the first neighbour in that order with the largest diff
 *   3  edge pixel, ua < p_edge_drop: dropped
 *   4  edge pixel, otherwise ua < p_edge_drop + p_edge_fly: a flying pixel, base = p + ((v(far) - p) * t >> 8), between p and v(far)
 *   5  any other pixel: base = p
 *   6  not an edge pixel: gx = |p[x+1] - p[x-1]| if both are in the image and foreground, else 0; gy likewise along y; max(gx, gy) > slope_step and
 *      ub < p_slope_drop: dropped
 *   7  every foreground pixel with ub >= 65536 - p_hole: dropped
 *   8  d1 = noise(base)
 *   9  DS4 with disparity_k = K > 0: disp = (2K + d1) // (2 d1); disp == 0: dropped; otherwise d1 = min(65535, (2K + disp) // (2 disp))
 *   10 the output is d1; a dropped pixel is 0
 * A background pixel: Ivy 0 (the sensor's "no data", which FilterIvy turns into the far count); DS4 with wall_count > 0: noise(wall_count) through step 9;
 *   DS4 otherwise 0.  Background pixels never become flying pixels: the silhouette frays inwards only, the hand never grows.
 * IR (ir_out given).  A pixel whose output depth d is nonzero: min(255, max(8, ir_floor + ir_gain // ((d * d >> 8) + 1) + (gi * ir_noise >> 6))); a pixel whose
 *   output is 0: dark, in [0, 8) -- what FilterDS4's `ir < 8` rule looks for.
 *
 * ht_sensor_noise_default  fills *out for `kind` from the camera's depth_scale (metres per count) and far (metres).  Host only, no context.  far_count is formed as
 *                       FilterIvy forms its constant, (unsigned short)(far / depth_scale) the x86 way: 3999 at 0.001 and 4.  NOBODY HAS MEASURED THESE FIGURES AGAINST A
 *                       CAMERA: there is no camera and no recording in this project.  They are defaults for experiments, reasoned from data sheets, not a
 *                       calibrated model (c = 1 / depth_scale counts per metre):
 *                         axial sd a + b z^2 metres: sigma0_256 = 256 a c, sigma2 = 2^28 b / c.  Ivy (SR300, coded light) a = 0.5 mm, b = 2 mm/m^2: 1 mm at half a
 *                           metre, 2.5 mm at one.  DS4 (R200, stereo) a = 0.2 mm, b = 4 mm/m^2: the stereo error z^2 * 0.08 px / (305 px * 70 mm) = 3.7 mm/m^2 at
 *                           the 320x240 stream's focal length, the R200's 70 mm baseline and a twelfth of a pixel of matching error
 *                         disparity_k (DS4) = 305 px * 0.070 m * 32 * c: the R200 reports disparity in steps of 1/32 pixel, disp = K / d
 *                         edge_step 20 mm, slope_step 15 mm over two pixels (a surface turned about 75 degrees away at half a metre), fly_bg_count = far_count
 *                         p_edge_drop / p_edge_fly 0.35 / 0.25 (Ivy: coded light loses the pattern at an edge) and 0.25 / 0.35 (DS4: block matching blends
 *                           the two sides), p_slope_drop 0.5, p_hole 0.002 (Ivy) and 0.01 (DS4), wall_count 0
 *                         ir_floor 16, ir_gain so that a surface at half a metre reads 128 above it (ir_gain = c^2 / 8) and falls with 1 / z^2, ir_noise 8 (sd 3.3 grey levels)
 *                       HT_ERR_ARG: out NULL, a kind that is neither, depth_scale or far not positive (NaN included), a far_count that comes out 0.
 * ht_sensor_simulate    depth [B][h*w] -> depth_out [B][h*w], ir_out [B][h*w] (optional for Ivy, required for DS4).  *noise is read on the host at call time.  B is
 *                       not bounded by max_batch (no tracker slot; the host form stages through a device buffer it grows on demand); B = 0 does nothing.
 *                       HT_ERR_ARG, checked before anything is launched or grown: a NULL required buffer; a kind that is neither; w or h < 1 or > 4096; B < 0;
 *                       far_count outside [1, 65536]; a probability outside [0, 65536] or p_edge_drop + p_edge_fly > 65536; depth_out overlapping depth; and, so
 *                       that no intermediate leaves the width the definition gives it (s(d) * g stays inside 31 bits, 2K + d1 inside 32): sigma0_256, ir_floor or
 *                       ir_noise outside [0, 65536], sigma2 outside [0, 4096], edge_step, slope_step, fly_bg_count or wall_count outside [0, 65535],
 *                       disparity_k outside [0, 2^30], ir_gain < 0.
 * ht_sensor_simulate_dev  the same on device buffers, asynchronous on `stream`: it only enqueues.  The noise set travels by value in the kernel's arguments. */
typedef struct ht_sensor_noise
{
	uint64_t seed, first_index;        /* frame f of a call is stream first_index + f */
	int far_count;                     /* an input count of 0 or >= far_count is background */
	int sigma0_256, sigma2;            /* axial sd in 1/256 count at depth d: sigma0_256 + ((int64)sigma2 * d * d >> 20) */
	int edge_step, slope_step;         /* counts */
	int p_edge_drop, p_edge_fly, p_slope_drop, p_hole;      /* probabilities in 1/65536 */
	int fly_bg_count;                  /* the depth a background neighbour stands for when an edge is judged and a flying pixel is mixed */
	int disparity_k;                   /* DS4 only; 0 = no disparity quantisation */
	int wall_count;                    /* DS4 only; the depth of the background, 0 = none */
	int ir_floor, ir_gain, ir_noise;   /* the IR image */
} ht_sensor_noise;
int ht_sensor_noise_default(int kind, float depth_scale, float far, ht_sensor_noise *out);
int ht_sensor_simulate(ht_ctx *ctx, int kind, const uint16_t *depth, int w, int h, int B, const ht_sensor_noise *noise, uint16_t *depth_out, uint8_t *ir_out);
int ht_sensor_simulate_dev(ht_ctx *ctx, int kind, const uint16_t *d_depth, int w, int h, int B, const ht_sensor_noise *noise, uint16_t *d_depth_out, uint8_t *d_ir_out, void *stream);

/* ---- left hands (an addition: the reference's model, nets and segmentation are a right hand's; its README lists left / right as open work) ----------------
 * A left hand seen by a camera is the mirror image of a right hand seen by the mirrored camera.  The mirror M is x -> -x of the camera's space:
 *   frame  [h][w] u16:  F'[y][x] = F[y][w-1-x]
 *   camera [12]:        focal, cy and depth_scale unchanged; cx' = (float)(w-1) - cx, one fp32 subtraction (DCamera::deprojectz's whole-pixel convention,
 *                       misc_image.h:48, the one PointCloud, FakeDepth and pixel_offset 0 use); the camera's pose mirrored as a pose
 *   pose   [7]:         (px,py,pz, qx,qy,qz,qw) -> (-px,py,pz, qx,-qy,-qz,qw): the pose of a bone whose geometry is x-negated in its own frame; it holds for
 *                       centre-of-mass poses and rig-space (user) poses alike.  Sign BITS are flipped: -0.0 and NaNs follow.
 * A left-hand update mirrors the frame, its camera and (if given) its start poses, runs the existing update on them in the frame's slot, and mirrors the poses
 * that come out.  The slot's state stays CANONICAL (the right hand's, mirrored space) from update to update: ht_get_state / ht_set_state, ht_tracker_reset,
 * cnn_out and ht_get_cnn_results, the stage calls and ht_joint_coords all speak the canonical space -- a caller who seeds a left slot mirrors the poses first
 * (ht_mirror_poses), and the joint coordinates of a left hand are those of its mirror image: the same numbers for both hands.  Changing a slot's flag without
 * re-seeding it is the caller's error.  Which hand a frame shows is not decided here.
 * hands [B] (uint8, nonzero = left) is optional everywhere: NULL means every frame for the three mirror calls, and NO frame for ht_update_hands_*.
 * ht_mirror_frames    depth [B][h][w] -> depth_out [B][h][w]; frames whose flag is 0 are copied.  w, h in [1, 4096].  Not in place: equal or overlapping
 *                     buffers are HT_ERR_ARG.  The device form moves 16 bytes per thread when w % 8 == 0 and both pointers are 16-byte aligned, 8 or 4
 *                     bytes for lesser widths and alignments, and single pixels for a buffer aligned to two bytes only (a view one pixel into an allocation).
 * ht_mirror_cams      cams [B][12] -> cams_out [B][12] for frames w pixels wide; may be in place.
 * ht_mirror_poses     poses [B][per_frame][7] -> poses_out; per_frame poses per frame (nb for a hand, 1 for single camera poses); may be in place.
 *                     For all three B is not bounded by max_batch (no tracker slot; the host forms stage through a buffer that follows the largest call);
 *                     B = 0 does nothing; the *_dev forms take device buffers (hands included) and are asynchronous on `stream`.
 * ht_update_hands_*   ht_update_frames_sized_* with a handedness flag per frame: shapes, sides, errors and point-capacity rules are exactly that call's,
 *                     64x64 tiles and side x side frames included (the update runs on the context's own 16-byte aligned staging, so ht_update_direct_dev's
 *                     alignment rule is met whatever d_depth is).  d_hands is a DEVICE pointer [B].  Without flags (NULL) the call forwards to
 *                     ht_update_frames_sized_* with the caller's own pointers: no staging, no extra launch, the same bits.  With flags it enqueues the three
 *                     mirror kernels, the update on the staging, and the pose mirror in place on d_poses_out; it only enqueues, so it can be captured into a
 *                     HIP graph once its staging exists.  cnn_out stays canonical.
 * ht_reserve_hands    allocates that staging ahead of time: max_batch frames of w x h pixels (at most 640x480), cameras and start poses.  Nothing is allocated
 *                     before the first flagged call or this one; it never shrinks; a flagged call that finds it too small grows it with one synchronising
 *                     re-allocation, as ht_reserve_points does.  1024 frames of 640x480 are 629 MB.  ht_hands_capacity reads the pixels per frame it holds.
 * ht_model_mirror     host only: mirrors the drawn and ray-cast geometry of an untracked model in place, by sign flips of the stored arrays: x of the hull vertices,
 *                     the sdmesh corners, the centres of mass and every stored plane (hull planes and the meshes' PolyPlanes) negated, the rest poses mirrored as
 *                     poses, every triangle (hull and sdmesh) keeping its first corner and swapping the other two.  Applied twice it restores every array byte for
 *                     byte; it commutes with ht_model_scale; ht_model_joint_limits is unchanged by it. */
int ht_mirror_frames(ht_ctx *ctx, const uint16_t *depth, int w, int h, int B, const uint8_t *hands, uint16_t *depth_out);
int ht_mirror_frames_dev(ht_ctx *ctx, const uint16_t *d_depth, int w, int h, int B, const uint8_t *d_hands, uint16_t *d_depth_out, void *stream);
int ht_mirror_cams(ht_ctx *ctx, const float *cams, int w, int B, const uint8_t *hands, float *cams_out);
int ht_mirror_cams_dev(ht_ctx *ctx, const float *d_cams, int w, int B, const uint8_t *d_hands, float *d_cams_out, void *stream);
int ht_mirror_poses(ht_ctx *ctx, const float *poses, int per_frame, int B, const uint8_t *hands, float *poses_out);
int ht_mirror_poses_dev(ht_ctx *ctx, const float *d_poses, int per_frame, int B, const uint8_t *d_hands, float *d_poses_out, void *stream);
int ht_update_hands_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, const uint8_t *hands, int B, float *poses_out, float *cnn_out);
int ht_update_hands_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, const uint8_t *d_hands, const float *d_start_poses, int B, float *d_poses_out, void *stream);
int ht_reserve_hands(ht_ctx *ctx, int w, int h);
int ht_hands_capacity(ht_ctx *ctx, size_t *frame_pixels);
int ht_model_mirror(ht_model *m);
int ht_model_body_planes(const ht_model *m, int body, float *hull_planes, float *mesh_planes);      /* the stored planes ht_model_mirror flips: the hull's [nplanes][4] (ht_model_body), the PolyPlane [t][4] of every sdmesh triangle; either may be NULL */

/* ---- two hands in one frame (an addition: HandSegmentVR, handtrack.h:280-344, treats everything nearer than wrange.y as ONE hand and arm) ----------------------
 * One front-end step on the device finds the blobs of a frame, takes the two largest, decides from their position which is the right hand and which the left, and
 * writes one masked frame per hand.  All integers on u16 pixels; W4 = w / 4, H4 = h / 4; sizes as ht_segment_vr_supported: w, h >= 8, multiples of 4, W4 * H4 <= 19200.
 *   quarter image  Q[Y][X] = the minimum of the 4x4 block of input pixels [4Y..4Y+3][4X..4X+3] (DownSampleMin(DownSampleMin(depth)), handtrack.h:285)
 *   foreground     range_lo <= Q < range_hi, raw depth units (range_lo = 0: the reference's one-sided threshold, :287)
 *   connectivity   two 4-neighbours are connected iff both are foreground and |Qa - Qb| <= max_step (65535 switches the depth test off)
 *   label          of a cell: the smallest raster index Y * W4 + X in its connected component; background cells carry 0xFFFF
 *   selection      components of count >= min_pixels cells are eligible and n_components counts them; the two with the largest count are taken, ties to the smaller label
 *   left / right   a is LOWER than b iff sum_x_a * count_b < sum_x_b * count_a (64-bit), a tie to the smaller label.  HT_SPLIT_RIGHT_IS_LOW_X clear (an egocentric
 *                  camera, HandSegmentVR's): the higher component is the right hand, the lower the left; set (a camera facing the user): the other way round.  A single
 *                  eligible component is low iff 2 * sum_x < count * (W4 - 1); it becomes the hand the flag puts on that side and the other hand is absent
 *   frames         depth_out[b][k][y][x] = depth[b][y][x] if label[y/4][x/4] is hand k's, else `far` (e.g. 4 / depth_scale, SampleD's background :343); k = 0 the right
 *                  hand, k = 1 the left; an absent hand's frame is all far.  With HT_SPLIT_MIRROR_LEFT frame k = 1 is written mirrored, out[1][y][x] = masked[y][w-1-x],
 *                  and cams_out[b][1] is the mirrored camera ("left hands" above); cams_out[b][0], and [b][1] without the flag, are the frame's camera
 *   info [B][2][8] int32 per hand: count (0 = absent), label, sum_x, sum_y, min_x, min_y, max_x, max_y in quarter-image cells; an absent hand reads 0, 0xFFFF, 0 ...
 * ht_split_hands      depth [B][h][w] -> depth_out [B][2][h][w], cams_out [B][2][12], info, n_components [B], labels [B][H4][W4] (uint16).  cams with cams_out (both or
 *                     neither), n_components and labels are optional (NULL).  B is not bounded by max_batch and the call needs no tracker slot, model or weights; the
 *                     host form stages through a buffer that follows the largest call; B = 0 does nothing; depth and depth_out must not overlap.  HT_ERR_ARG for a size
 *                     the rule refuses, range_lo >= range_hi, far < range_hi, min_pixels < 1 and unknown flag bits.  The device form takes device buffers, is
 *                     asynchronous on `stream`, and moves 16, 8 or 4 bytes per thread as the width and both frame pointers allow, else single pixels; without
 *                     d_labels it cuts along a label image the context keeps (grown with one synchronising re-allocation to the largest call).
 * ht_update_two_hands_*  B frames of two hands each, tracked in 2B slots (2 * B <= max_batch): slot 2i frame i's right hand, slot 2i + 1 its left hand in canonical
 *                     (mirrored) space.  The split writes straight into the left-hands staging (ht_reserve_hands sizes it; a call that finds it too small grows it the
 *                     same way), right hands unmirrored, left hands mirrored whether or not HT_SPLIT_MIRROR_LEFT is given; ht_update_frames_sized_* runs on those 2B
 *                     frames with that call's shapes, sides, errors and point-capacity rules; the odd slots' poses are mirrored back.  poses_out [B][2][nb][7] and
 *                     d_start_poses [B][2][nb][7] are in the camera's own space; cnn_out [2B][HT_CNN_OUT] and the slots' state stay canonical.  An absent hand's slot
 *                     sees an all-far frame and takes the update's too-few-points path: info [B][2][8] (optional) tells the caller that its pose means nothing.  The
 *                     device form only enqueues once its staging exists. */
#define HT_SPLIT_RIGHT_IS_LOW_X 1
#define HT_SPLIT_MIRROR_LEFT 2
int ht_split_hands(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, int B, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, int flags, uint16_t *depth_out, float *cams_out, int32_t *info, int32_t *n_components, uint16_t *labels);
int ht_split_hands_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, int flags, uint16_t *d_depth_out, float *d_cams_out, int32_t *d_info, int32_t *d_n_components, uint16_t *d_labels, void *stream);
int ht_update_two_hands_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, int flags, int B, float *poses_out, int32_t *info, float *cnn_out);
int ht_update_two_hands_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, int flags, const float *d_start_poses, int B, float *d_poses_out, int32_t *d_info, void *stream);

/* ---- two hands that touch or cross (an addition: the blob split above gives ONE blob for hands that touch, and names hands by their place in the image) ---------
 * Each foreground cell of the quarter image goes to the hand whose tracked model is nearer, by the tracker's own closest() (physmodel.h:137-162, the signed distance
 * FitError and the cloud rows use).  Labels, info and frames have the blob split's shape, so the frame writer, the cameras and the update behind them are the calls above.
 * The context needs a hand model (HT_ERR_STATE otherwise).  Sizes as ht_split_hands.
 *   cell depth     Q[Y][X] as above; (x*, y*) the first pixel of the 4x4 block, in raster order, that attains it; foreground range_lo <= Q < range_hi
 *   cell point     v = deprojectz((x*, y*), (float)Q * depth_scale) with cams[f]'s focal, principal point and depth_scale in the expression order of misc_image.h:48;
 *                  the camera's pose is not used: poses are in the camera's own space, as ht_update_two_hands_*'s poses_out and d_start_poses and as ht_render_depth
 *   priors         poses [B][2][nb][7]: index 0 the right hand, 1 the left hand in real (unmirrored) space; centre-of-mass poses (ht_tracker_reset's, ht_render_depth's).
 *                  The left prior is first mirrored into canonical space ("left hands" above: sign bits, exact).  With HT_SPLIT_USER_POSES every pose is a user pose
 *                  (an update's poses_out) and pos += qrot(q, com[b]) is applied after that mirror, in the space the model's com[b] belongs to
 *   distances      d_R = dot(plane, (v, 1)) with plane = closest(bodies at the right prior, v); d_L the same with the bodies at the canonical left prior and the
 *                  point (-v.x, v.y, v.z).  fp32, one IEEE operation after another in the reference's order
 *   assignment     a foreground cell gets label 0 (right) iff d_R <= d_L, otherwise 1; if (d_L < d_R ? d_L : d_R) > max_dist it is background.  max_dist in metres;
 *                  +inf or FLT_MAX switch the test off; NaN or negative: HT_ERR_ARG.  Background cells carry 0xFFFF
 *   info [B][2][8] as above over the cells of each label, label = 0 or 1; a hand of count < min_pixels is absent (0, 0xFFFF, 0, ...) and the frame writer matches none
 *                  of its cells
 *   modes          HT_SPLIT_MODEL_ALWAYS: every frame as above; no blob labelling runs, max_step is not used, HT_SPLIT_RIGHT_IS_LOW_X is refused; n_components is the
 *                  number of present hands.  HT_SPLIT_MODEL_MERGED: the blob split runs first, unchanged; a frame takes the model assignment iff the blob split found
 *                  n_components < 2 AND the model assignment leaves both hands present; otherwise the blob split's labels and info stand, byte for byte.
 *                  n_components is the blob split's
 *   source [B]     int32, optional: 0 the frame's result is the blob split's, 1 the model's
 *   dist           [B][H4][W4][2] fp32, optional: d_R, d_L of every foreground cell (also of one that max_dist dropped), +inf for the others; in MERGED mode +inf
 *                  throughout a frame whose blob split found two components (nothing was evaluated)
 * ht_split_hands_model      depth, cams, poses -> depth_out [B][2][h][w], cams_out [B][2][12], info, n_components, source, dist, labels.  cams is required; cams_out,
 *                  n_components, source, dist and labels are optional (NULL).  B is not bounded by max_batch; the host form stages through the buffer that follows
 *                  the largest call; B = 0 does nothing; every check runs before anything grows or launches and a refused call leaves the context usable.
 * ht_update_two_hands_model_*  ht_update_two_hands_* with this split in front: the same staging, 2 * B <= max_batch rule and errors.  The priors are the poses the
 *                  update starts from: d_start_poses where given, else slot 2i's and 2i + 1's carried hand-model state (the left one is canonical already and is not
 *                  mirrored: the same bits).  HT_SPLIT_USER_POSES is refused here (d_start_poses also seed the slots, as centre-of-mass poses). */
#define HT_SPLIT_MODEL_ALWAYS 0
#define HT_SPLIT_MODEL_MERGED 1
#define HT_SPLIT_USER_POSES   4   /* accepted by the new calls only */
int ht_split_hands_model(ht_ctx *ctx, const uint16_t *depth, const float *cams, const float *poses, int w, int h, int B, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, float max_dist, int mode, int flags, uint16_t *depth_out, float *cams_out, int32_t *info, int32_t *n_components, int32_t *source, float *dist, uint16_t *labels);
int ht_split_hands_model_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_poses, int w, int h, int B, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, float max_dist, int mode, int flags, uint16_t *d_depth_out, float *d_cams_out, int32_t *d_info, int32_t *d_n_components, int32_t *d_source, float *d_dist, uint16_t *d_labels, void *stream);
int ht_update_two_hands_model_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, float max_dist, int mode, int flags, int B, float *poses_out, int32_t *info, int32_t *source, float *cnn_out);
int ht_update_two_hands_model_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, float max_dist, int mode, int flags, const float *d_start_poses, int B, float *d_poses_out, int32_t *d_info, int32_t *d_source, void *stream);

/* ---- tracking accuracy (an addition: the reference places model points in the image in every application and measures nothing) -----------------------------
 * Keypoints of a batch of poses in 3-D and in pixels with their visibility against the depth frame, keypoint errors between two pose sets with the literature's
 * summary figures, the depth residual and silhouette overlap of two sets of frames, and poses against frames in one call.  Everything fp32, one IEEE operation
 * after another in the written order; a pose is position + quaternion xyzw, a camera the 12 floats of the header (focal xy, principal xy, depth_scale, pose).
 * For all of them B is not bounded by max_batch, B = 0 does nothing, every check runs before anything grows or launches, and a refused call leaves the context usable.
 *   keypoint table  K entries (bone, offset[3], rel): rel = 0, the offset is in the body's user frame (GetPoseUser); rel = 1, in its centre-of-mass frame (GetPose).
 *                   HT_KP_FEATURE8: handmodelfeaturepoints (handtrack.h:77-81) verbatim, rel = 1, hand layouts only (HT_SAMPLE_ENHANCED's rule; HT_ERR_ARG otherwise).
 *                   HT_KP_SKELETON, all rel = 0: body 0's user origin; then per joint in model order its child-side anchor (rbi1, p1); then per leaf body (a body
 *                   that is no joint's rbi0) in body order (b, com[b]): 1 + 16 + 5 = 22 entries for the stock hand.  ht_scale rescales both with the model.
 *                   HT_KP_CALLER: the caller's bones / offsets [K][3] / rel (HOST arrays in both forms), 1 <= K <= HT_KP_MAX, bones in [0, nb), finite offsets.
 *   position        o' = o when rel matches the poses' convention; user poses (the default, what the update calls return) and rel = 1: o' = o + com[bone];
 *                   HT_KP_COM_POSES and rel = 0: o' = o - com[bone]; then, for a frame flagged in hands [B] (uint8, optional: a left hand in real space as
 *                   ht_update_hands_* returns it), the sign bit of o'.x is flipped.  X = pos + qrot(q, o'): Skin (handtrack.h:82-84).  xyz [B][K][3], the poses' frame.
 *   pixels          v = qrot(conj(qc), X - pc) with the camera's pose (pc, qc); u = v.x / v.z * fx + cx, likewise y: projectz(cam.pose.inverse() * X),
 *                   ImageFeaturePoints (handtrack.h:92-96; the overlay :632-634, dataexporter.cpp:82,105, annotation-fixer.cpp:315-317).  pix [B][K][2], zc [B][K] = v.z.
 *   visibility      vis [B][K] uint8 against depth [B][h][w]: ix = floorf(u + 0.5f), iy likewise (deprojectz's whole-pixel convention, misc_image.h:48); tested in
 *                   this order: 4 if !(v.z > 0); 3 if !(u + 0.5f >= 0 && u + 0.5f < w) or the same fails for y (in float, so non-finite values land here);
 *                   with d = (float)depth[iy][ix] * depth_scale: 1 (occluded) if d < v.z - near_tol; 2 (nothing there) if d > v.z + far_tol; 0 (visible) otherwise.
 *                   Keypoints lie inside their bones: near_tol must cover a bone's half thickness.
 * ht_keypoint_table   a built-in table of the context's model as ht_scale left it: *K, bones [K], offsets [K][3], rel [K]; any output may be NULL.
 * ht_keypoints        poses [B][nb][7] -> xyz, pix, zc, vis, each optional (NULL).  which: HT_KP_FEATURE8, HT_KP_SKELETON or HT_KP_CALLER (K, bones, offsets, rel are
 *                     read only then).  flags: HT_KP_COM_POSES.  pix and zc need cams [B][12]; vis needs cams and depth, w, h in [1, 4096] and finite tolerances >= 0
 *                     in metres (HT_ERR_ARG otherwise).  HT_ERR_STATE for a context without a hand model.
 * ht_keypoint_errors  a, b [B][K][3] -> dist [B][K] = sqrtf(dx dx + dy dy + dz dz) summed left to right; frame [B][2] = the fp32 sum over k ascending divided by
 *                     (float)K, and the maximum over k (a NaN distance makes both NaN); over the batch sum_kp [K] (double: every distance widened, then added, in
 *                     any order), hits_kp [T] (int64: pairs with dist <= thr[t]) and hits_frame [T] (int64: frames whose maximum is <= thr[t], the "fraction of
 *                     frames with the worst joint under e" curve).  NaN hits nothing.  1 <= K <= HT_KP_MAX, 0 <= T <= HT_KP_MAX_THR, thr [T] a HOST array in both
 *                     forms; every output is optional.  Needs no model: works on a CNN-only context.
 * ht_depth_compare    a, b [B][h][w] u16 -> info [B][8] int64; a pixel is foreground iff lo <= p < hi in raw units (ht_split_hands' half-open rule; 0 <= lo < hi <= 65536):
 *                     n_a, n_b, n_both, n_close (in both, |a - b| <= tol), sum |a - b| over both, sum (a - b)^2 over both, max |a - b| over both (0 if none), 0.
 *                     Exact integers.  w, h in [1, 4096], tol in [0, 65535].  IoU = n_both / (n_a + n_b - n_both); residuals in metres are host arithmetic with
 *                     depth_scale.  The device form loads 16, 8 or 4 bytes per thread as the width and both pointers allow (ht_mirror_frames' rule), else single
 *                     pixels.  Needs no model.
 * ht_pose_depth_residual  poses against frames: each pose is brought to what ht_render_depth takes -- without HT_KP_COM_POSES pos += qrot(q, com[b]) (the inverse of
 *                     PositionUser, physics.h:142); then, unless the frame's camera pose is bit for bit (0,0,0, 0,0,0,1), pos' = qrot(conj(qc), pos - pc) and
 *                     q' = qmul(conj(qc), q) -- ht_render_depth renders them at `far` into a buffer of the context (grown to the largest call by one synchronising
 *                     re-allocation before anything is enqueued), and ht_depth_compare runs with a = depth (observed) and b = rendered.  rendered [B][h][w] is
 *                     an optional output.  Choose hi <= far / depth_scale to keep the rendered background out (not checked: depth_scale is per frame).
 *                     HT_ERR_STATE for a context without a hand model.  No left-hand form (mirror first).
 * ht_pose_mesh_residual   the same against the hand's subdivision surface: arguments, pose preparation and comparison are ht_pose_depth_residual's, the renderer is
 *                     ht_raster_mesh_depth at pixel offset 0.  Also HT_ERR_STATE where that call gives it (a model file without meshes).
 * The host forms refuse output buffers that overlap an input (HT_ERR_ARG); the *_dev forms take device buffers (hands included) and are asynchronous on `stream`. */
#define HT_KP_COM_POSES 1
#define HT_KP_FEATURE8 0
#define HT_KP_SKELETON 1
#define HT_KP_CALLER 2
#define HT_KP_MAX 64
#define HT_KP_MAX_THR 32
int ht_keypoint_table(ht_ctx *ctx, int which, int *K, int *bones, float *offsets, int *rel);
int ht_keypoints(ht_ctx *ctx, const float *poses, int B, int flags, int which, int K, const int *bones, const float *offsets, const int *rel, const uint8_t *hands, const float *cams, const uint16_t *depth, int w, int h, float near_tol, float far_tol, float *xyz, float *pix, float *zc, uint8_t *vis);
int ht_keypoints_dev(ht_ctx *ctx, const float *d_poses, int B, int flags, int which, int K, const int *bones, const float *offsets, const int *rel, const uint8_t *d_hands, const float *d_cams, const uint16_t *d_depth, int w, int h, float near_tol, float far_tol, float *d_xyz, float *d_pix, float *d_zc, uint8_t *d_vis, void *stream);
int ht_keypoint_errors(ht_ctx *ctx, const float *a, const float *b, int B, int K, const float *thr, int T, float *dist, float *frame, double *sum_kp, int64_t *hits_kp, int64_t *hits_frame);
int ht_keypoint_errors_dev(ht_ctx *ctx, const float *d_a, const float *d_b, int B, int K, const float *thr, int T, float *d_dist, float *d_frame, double *d_sum_kp, int64_t *d_hits_kp, int64_t *d_hits_frame, void *stream);
int ht_depth_compare(ht_ctx *ctx, const uint16_t *a, const uint16_t *b, int w, int h, int B, int lo, int hi, int tol, int64_t *info);
int ht_depth_compare_dev(ht_ctx *ctx, const uint16_t *d_a, const uint16_t *d_b, int w, int h, int B, int lo, int hi, int tol, int64_t *d_info, void *stream);
int ht_pose_depth_residual(ht_ctx *ctx, const float *poses, const float *cams, const uint16_t *depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *info, uint16_t *rendered);
int ht_pose_depth_residual_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, const uint16_t *d_depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *d_info, uint16_t *d_rendered, void *stream);
int ht_pose_mesh_residual(ht_ctx *ctx, const float *poses, const float *cams, const uint16_t *depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *info, uint16_t *rendered);
int ht_pose_mesh_residual_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, const uint16_t *d_depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *d_info, uint16_t *d_rendered, void *stream);

/* ---- keypoint fit (an addition: the reference nails one dragged bone and pulls its own eight landmarks onto rays, one frame at a time) -----------------------
 * From keypoint targets to a pose: the inverse of ht_keypoints.  The slots' current state of model which_model (0 handmodel, 1 othermodel) is the start pose; every
 * step writes the targets' constraint rows from that state on the device and solves them with ht_fit_rows' own launch sequence without points (the joint ranges
 * brought up to date, contacts if physics_use_collision, the rows ahead of the joints' rows); nothing is copied or waited for between the steps.
 *   table      which / K / bones / offsets / rel exactly as ht_keypoints takes them (HT_KP_FEATURE8, HT_KP_SKELETON, HT_KP_CALLER; HOST arrays in both forms).
 *   position   the states are centre-of-mass poses: rel = 1, o' = o; rel = 0, o' = o - com[bone]; X = pos + qrot(q, o').
 *   kind [K]   HOST array in both forms, NULL = all 0.  0: a point target t = xyz[b][k], three rows as ConstrainPositionNailed writes them (physics.h:342-346): rb0 = -1,
 *              rb1 = bone, position0 = t, position1 = o', normals (1,0,0), (0,1,0), (0,0,1), targetdist = (X - t) by component, forcelimit (-f, f).
 *              1: a pixel target (u, v) = pix[b][k] in the frame's camera (pc, qc) = cams[b]: r = normalize(qrot(qc, ((u - cx) / fx, (v - cy) / fy, 1))) (deprojectz,
 *              misc_image.h:48), q = quat_from_to((0,0,1), r); for the axes a = qxdir(q), then qydir(q): d = dot(X - pc, a) and the dead-zone pair of
 *              ConstrainAlongDirectionDeadzone (physics.h:337-338): targetdist d + ray_radius with forcelimit (0, fr), then d - ray_radius with (-fr, 0); position0 = pc,
 *              the camera's position (handtrack.h:672), so a camera away from the origin is served.  Four rows.
 *   presence   a keypoint is present iff its weight > 0 (weights [B][K] optional, NULL = 1) and every target component it reads is finite: NaN is "not annotated".
 *              Absent keypoints write no rows; the others keep the table's order.  f = max_force * weight, fr = ray_force * weight.
 *   resid      [B][2][K], optional: at the start pose and after the last step; sqrtf(dx dx + dy dy + dz dz) of X - t for a point, the distance to the ray
 *              sqrtf(d d + d' d') of the two axes' d for a pixel, -1 for an absent keypoint.
 *   poses      [B][nb][7], optional: the user poses (GetPoseUser) after the last step, as the update calls return them.
 *   options    steps in [1, 64]; max_force > 0 (INFINITY is taken as FLT_MAX); ray_radius >= 0; ray_force > 0.  HT_KPFIT_KEEP_MOMENTA: the momenta are never touched
 *              (slowfit's behaviour); otherwise they are zeroed on entry and after every step (MultiStepSim's, handtrack.h:686-687).  NULL = ht_kpfit_default's:
 *              6 steps, FLT_MAX, 0.01, 100000, no flags (slowfit's figures).
 * xyz [B][K][3] is read (and required) only if kind 0 occurs, pix [B][K][2] and cams [B][12] only if kind 1 does.  Refused before anything grows or runs (HT_ERR_ARG /
 * HT_ERR_STATE): a context without a hand model, the exact-order solver build, B outside [1, max_batch], a bad table or kind, a table of more than 5 * nb + 128 rows
 * (3 a point, 4 a pixel), a missing array, bad options; the host form also refuses a weight outside [0, 1] and an output that overlaps an input.  A refused call leaves
 * the context usable and the states unchanged.  The _dev form takes device arrays, grows the context's row buffer before its first launch and only enqueues on
 * `stream`; the host form stages through the context's buffer and returns when the work is done.  Slots >= B are not touched.  Like ht_fit_rows, the call leaves
 * the slots' prepared points empty (follow with ht_update_passes_sync or ht_stage_prepare for a depth cloud).  There is no left-hand form: mirror the targets
 * (x -> -x) and bring the poses back with ht_mirror_poses. */
#define HT_KPFIT_KEEP_MOMENTA 1
typedef struct { int steps; float max_force, ray_radius, ray_force; int flags; } ht_kpfit;
int ht_kpfit_default(ht_kpfit *o);
int ht_fit_keypoints(ht_ctx *ctx, int which_model, int B, int which, int K, const int *bones, const float *offsets, const int *rel, const int *kind, const float *xyz, const float *pix, const float *weights, const float *cams, const ht_kpfit *o, float *poses, float *resid);
int ht_fit_keypoints_dev(ht_ctx *ctx, int which_model, int B, int which, int K, const int *bones, const float *offsets, const int *rel, const int *kind, const float *d_xyz, const float *d_pix, const float *d_weights, const float *d_cams, const ht_kpfit *o, float *d_poses, float *d_resid, void *stream);

/* ---- several views (an addition: the reference keeps the pieces -- ImageClip, PlaneSplit, Mirror, MirrorPlaneSplit "to get some view of the back of an object",
 * misc_image.h:401-485, and a mirror plane in every data set header, dataset.h:24,45 -- and tracks from one camera) ----------------------------------------------
 * One hand seen by V <= HT_VIEWS_MAX depth cameras at once, and by their mirror images where a view holds a mirror.  Per slot: frames depth [B][V][h][w] (one w x h for
 * all views of a call), cameras cams [B][V][12] in the usual layout with their poses in ONE tracking space, and optionally mirror planes planes [B][V][4], each in its
 * view's camera space; NULL, or a plane (0,0,0,FLT_MAX) as dataset.h:45 defaults it, means none.
 * ht_fuse_views       the views' clouds as one, fp32, one IEEE operation after another (no contraction):
 *                       1. the views in order, each view's pixels in raster order;
 *                       2. d = pixel * depth_scale, in range iff d >= range_lo && d < range_hi (FallsWithinRange, misc_image.h:24);
 *                       3. p = deprojectz(x, y, d) = (((x - cx) / fx) * d, ((y - cy) / fy) * d, d) (misc_image.h:48);
 *                       4. with a mirror plane, pd = dot(float4(p, 1), plane) (PlaneSplit, misc_image.h:462-473): pd <= -mirror_eps, the point is virtual,
 *                          p += n * (pd * -2) (Mirror, :474-479), source 2v + 1; pd > mirror_eps, direct, source 2v; otherwise (coplanar) the pixel is dropped.
 *                          Without a plane every in-range pixel is direct;
 *                       5. the kept pixels of a view are ranked in raster order, rank r is emitted iff r % fraction == 0 (takesubsample, physmodel.h:58-64);
 *                       6. an emitted point goes to tracking space by its view's pose, pos + qrot(q, p); a pose that is exactly identity is not applied at all;
 *                       7. the fused cloud is view-major and keeps the order within a view; direct and mirrored points interleave as they come.
 *                     The cloud is left where a fit pass reads the slot's prepared points (as ht_stage_prepare or an update leaves theirs), x y z and the source index
 *                     as a float beside them (the .w the other producers write as 0).  Outputs of the host form, all optional: points [B][cap][4], cut at cap (the
 *                     point capacity grows to min(cap, V * ceil(w h / fraction)), HT_ERR_ARG if that exceeds HT_POINTS_LIMIT); npoints [B]; per_source [B][2V], the
 *                     points kept of every source; origins [B][2V][3]: the view's camera position for a direct source, pos + qrot(q, n * (plane.w * -2)) for a
 *                     mirrored one (the camera's image in the mirror; the camera position again where the view has no plane); *cut, the slots whose cloud was cut.
 * ht_fuse_views_dev   device arrays, enqueued on `stream`.  Grows the point capacity to V * ceil(w h / fraction) before its launch (one synchronising re-allocation,
 *                     as ht_reserve_points) and refuses a call that could exceed HT_POINTS_LIMIT, so no cloud is cut.  d_npoints, d_per_source, d_origins, d_cut optional.
 *                     It cannot read the planes: a view whose plane is neither "none" nor finite with a normal other than zero emits nothing.
 * ht_views_default    range {0.1, drangey} (handtrack.h:703), fraction = subsample_fraction, mirror_eps 0.02 (PlaneSplit's default).  NULL options mean these.
 * ht_stage_view_rows  CloudConstraints (physmodel.h:164-181) of model `which` for every fused point with FitPointCloud's force limits (:347), each point's ray from ITS
 *                     source's origin: CloudConstraint decides "the point lies behind the body" by dot(v - origin, n) > 0 and casts ConvexHitCheck from that origin
 *                     (:170-171), so a point seen from behind and judged from another camera's origin takes the wrong branch.  rows [B][cap][16] in
 *                     ht_stage_cloud_rows' layout, nrows [B].  Host buffers, synchronous.
 * ht_fit_views        `passes` (1..64) times PhysModel::FitPointCloud's sequence on model `which` of slots [0,B) against the fused cloud: the joint ranges brought up to
 *                     date (HandModelEnhancements), those rows, contacts if physics_use_collision, the solve.  No boundary planes (they assume one viewpoint); the
 *                     momenta are kept from pass to pass as in update()'s main passes (handtrack.h:769-780); the last solve writes the user poses [B][nb][7]
 *                     (optional).  The tracker's flags are not touched.  _dev: everything on `stream`, no copy or wait between the passes.  HT_ERR_STATE unless
 *                     the latest ht_fuse_views of the context covered slots [0,B); points another call leaves there afterwards read as source 0.
 * ht_update_views_*   ht_update_frames_sized_* on view 0, byte for byte the existing call, then ht_fuse_views of all views and ht_fit_views(0, B, passes), whose poses
 *                     the caller gets.  The net, the segmentation, FitError and MultiStepSim see view 0 only.  View 0's camera pose must be identity (the reference's
 *                     PointCloud is camera-local, handtrack.h:703): HT_ERR_ARG in the host form; the device form cannot read the cameras.
 * Refused before anything grows or runs, the context left usable (HT_ERR_ARG / HT_ERR_STATE): V outside [1, HT_VIEWS_MAX]; a bad range (0 <= range_lo < range_hi),
 * fraction (>= 1) or mirror_eps (>= 0); in the host forms a plane with a non-finite or zero normal that is not the "none" plane, and an output that overlaps an input
 * or another output; B outside [1, max_batch]; a context without a hand model; for the fits the exact-order solver build.  Slots >= B and the other model are not
 * touched.  There is no left-hand form: mirror the inputs with ht_mirror_* and the poses back.  Views of different sizes, the voxel subsample and a net evaluation on
 * views other than view 0 are not served. */
#define HT_VIEWS_MAX 4
typedef struct { float range_lo, range_hi; int fraction; float mirror_eps; } ht_views;
int ht_views_default(ht_ctx *ctx, ht_views *o);
int ht_fuse_views(ht_ctx *ctx, const uint16_t *depth, const float *cams, const float *planes, int w, int h, int V, int B, const ht_views *o, float *points, int cap, int *npoints, int *per_source, float *origins, int *cut);
int ht_fuse_views_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, int B, const ht_views *o, int *d_npoints, int *d_per_source, float *d_origins, int *d_cut, void *stream);
int ht_stage_view_rows(ht_ctx *ctx, int which, int B, float *rows, int cap, int *nrows);
int ht_fit_views(ht_ctx *ctx, int which, int B, int passes, float *poses);
int ht_fit_views_dev(ht_ctx *ctx, int which, int B, int passes, float *d_poses, void *stream);
int ht_update_views_sync(ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, const float *planes, int w, int h, int V, float segment_scale, int B, const ht_views *o, int passes, float *poses_out, float *cnn_out);
int ht_update_views_dev(ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, float segment_scale, const float *d_start_poses, int B, const ht_views *o, int passes, float *d_poses_out, void *stream);
/* Timing only (tools/bench_views.py): the yardsticks the calls above are measured beside, on device buffers, enqueued on `stream` and not waited for.
 * ht_debug_prepare_frames_dev   k_prepare_frame alone on B frames [B][h][w] with the tracker's range and fraction, into the slots' prepared points (what an update's input
 *                               stage launches for full-size frames; takesubsample(PointCloud(..)), handtrack.h:703,751).
 * ht_debug_fit_rows_pass_dev    one pass of ht_fit_rows' launch sequence on model `which` against the slots' prepared points, without caller rows, the momenta kept. */
int ht_debug_prepare_frames_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, void *stream);
int ht_debug_fit_rows_pass_dev(ht_ctx *ctx, int which, int B, void *stream);

/* ---- a view's extrinsics from the tracked hand (an addition: the reference never calibrates anything, it has no rig) -----------------------------
 * "Several views" above needs every camera posed in one tracking space.  While view 0 tracks the hand, the tracked model is a known 3-D object in that space and another
 * view's depth pixels lie on its surface: ht_calibrate_view registers that view's cloud rigidly against the tracked models of a batch of frames, a Gauss-Newton loop
 * around the tracker's own closest() (physmodel.h:137-162).  depth [B][h][w] and cams [B][12] are the view's frames and cameras, one a slot.
 *   cloud      per slot, the view's pixels in raster order: d = pixel * depth_scale, kept iff d >= range_lo && d < range_hi (FallsWithinRange, misc_image.h:24),
 *              p = deprojectz(x, y, d) (misc_image.h:48), every fraction-th kept pixel emitted (takesubsample, physmodel.h:58-64): exactly ht_fuse_views' cloud for
 *              V = 1, an identity pose and no plane.  The points stay in the camera's space in a buffer of the context's own, grown to ceil(w h / fraction) points a
 *              slot by one synchronising re-allocation as ht_reserve_points grows its arrays (more than HT_POINTS_LIMIT: HT_ERR_ARG, raise the fraction).  The slots'
 *              prepared points, both models' states and the tracker's flags are not touched.  Mirror planes are not accepted.
 *   model      poses == NULL: the state of model `which` (0 handmodel, 1 othermodel) of slots [0,B), B <= max_batch.  Otherwise poses [B][nb][7], centre-of-mass poses
 *              in tracking space as ht_split_hands_model takes them; no slot is read and B is bounded by 65535 only.  The same poses give the same bits either way.
 *   transform  T = (pos, q) maps camera space to tracking space as the fused cloud does: x = pos + qrot(q, p).  The guess is the pose in cams[b][5:12].
 *              HT_CALIB_RIG: one T for the batch (the rig is fixed and the hand moves), N = 1, the guess is slot 0's.  HT_CALIB_PER_SLOT: one T a slot, N = B.
 *              T is carried in float64.  Per point x is formed in fp32 from T rounded to fp32 (quaternion not renormalised), so closest() sees what a fused cloud holds.
 *   per point  fp32, one IEEE operation after another in ht_fuse_views' forms (dot = ((ax bx + ay by) + az bz) [+ w], qrot over qmat's columns):
 *              plane = closest(bodies of slot b, x), bit for bit the reference's (strict "<", the first minimum in body order, both walks);
 *              r = dot(plane, (x, 1)); n = plane.xyz; J = [n, cross(x - c, n)] about the caller's centre c = o.centre; w = |r| <= max_dist ? 1 : 0.
 *   sums       29 float64 values S: k = 0..20 the upper triangle of J J^T row by row ((0,0), (0,1), .. (0,5), (1,1), ..), 21..26 J r, 27 the truncated cost
 *              (r r < m ? r r : m with m = (double)max_dist * (double)max_dist), 28 the inlier count.  Every product is of the two fp32 terms widened to float64;
 *              the first 27 take w ? term : 0.0, the cost takes every point.
 *   order      part of the definition.  Thread t of 256 adds its points t, t + 256, .. in cloud order onto +0.0.  A wave's 64 threads are reduced by the butterfly
 *              v[l] += v[l ^ 32], then ^ 16, 8, 4, 2, 1 (five levels of pairwise adds; every lane holds the same bits); the four waves as (w0 + w1) + (w2 + w3).
 *              In RIG mode the slots' sums are added in slot order onto slot 0's.  No floating-point atomics, nothing depends on arrival.
 *   step       float64, + - * / and sqrt only, no contraction.  A is S's symmetric matrix with A_ii *= 1 + (double)damping, g = S[21..26].  Cholesky A = L L^T column by
 *              column: s = A_jj - L_j0 L_j0 - .. (k ascending); the pivot s must be > 0; L_jj = sqrt(s); L_ij = (A_ij - L_i0 L_j0 - ..) / L_jj.  Forward
 *              y_i = (-g_i - L_i0 y_0 - ..) / L_ii, back d_i = (y_i - L_{i+1,i} d_{i+1} - .. - L_{5,i} d_5) / L_ii (k ascending).  dt = d[0..2], dw = d[3..5].
 *              dq = (dw / 2, 1) / sqrt(((x x + y y) + z z) + 1), q <- qmul(dq, q) / its length, pos <- (c + qrot(dq, pos - c)) + dt, qmul and qrot in the forms above.
 *   degenerate fewer than min_points inliers (flag bit 0), a pivot that is not > 0 or a step that is not finite (bit 1): the step is zero, T keeps its bits.
 *              A NaN never comes out of finite inputs.
 *   iterations every one of o.iterations (0..64) is the same pair of launches on the caller's stream, one more evaluates the final state.  iterations = 0 evaluates
 *              the guess and returns its cost: the way to score any T.
 *   T_out      fp32 [N][7], T rounded.  stats float64 [iterations + 1][N][HT_CALIB_STATS]: row i describes the state before step i, row `iterations` the final state
 *              (no step: |dt| = |dw| = 0, flag bit 0 only).  A record: inliers, points, truncated cost, |dt|, |dw|, flag, then the 21 entries of the undamped A in
 *              S's order -- a flat hand shows as a sliding direction in A.
 * ht_calib_default    range {0.1, drangey}, fraction = subsample_fraction, HT_CALIB_RIG, 10 iterations, max_dist 0.03 m, damping 1e-3, min_points 12, centre (0,0,0).
 *                     NULL options mean these.
 * ht_calibrate_view   host arrays, synchronous.  ht_calibrate_view_dev: device arrays (d_stats and d_T_out 4-byte aligned), everything enqueued on `stream`, no host
 *                     wait inside but the re-allocation above.
 * Refused before anything grows or runs, the context left usable (HT_ERR_ARG / HT_ERR_STATE): frames or cameras missing, w or h outside [1, 4096]; T_out or stats NULL;
 * which not 0 or 1; B < 1 or beyond the bound above; a bad range (0 <= range_lo < range_hi, finite), fraction (>= 1), mode, iterations (0..64), max_dist (> 0, finite),
 * damping (>= 0, finite), min_points (>= 0) or centre (finite); a context without a hand model.  Out of scope: estimating a mirror plane, intrinsics, time offsets
 * between cameras, several views in one call (call once a view), the overlapped arrangement, and feeding T back into ht_update_views_* (the caller writes it into cams). */
#define HT_CALIB_RIG 0
#define HT_CALIB_PER_SLOT 1
#define HT_CALIB_STATS 27
#define HT_CALIB_FEW_INLIERS 1
#define HT_CALIB_BAD_PIVOT 2
typedef struct { float range_lo, range_hi; int fraction, mode, iterations; float max_dist, damping; int min_points; float centre[3]; } ht_calib;
int ht_calib_default(ht_ctx *ctx, ht_calib *o);
int ht_calibrate_view(ht_ctx *ctx, int which, const float *poses, const uint16_t *depth, const float *cams, int w, int h, int B, const ht_calib *o, float *T_out, double *stats);
int ht_calibrate_view_dev(ht_ctx *ctx, int which, const float *d_poses, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, const ht_calib *o, float *d_T_out, double *d_stats, void *stream);

/* ---- the hand's size from tracked frames (an addition: every live application of the reference asks the user for it, "hand size %f cm (use +/- to scale)",
 * openvr-demo.cpp:109, realtime-annotator.cpp:238) ---------------------------------------------------------------------------------------------------
 * The tracker fits a model of one fixed size; ht_scale applies a size and nothing found it.  PhysModel::scale(s) (physmodel.h:196-219, :304-319) is a uniform
 * similarity about body 0's position w, so a depth point y lies at distance s * dist(w + (y - w) / s) from the hand scaled by s, dist being the unscaled model's
 * closest(): size is a seventh degree of freedom beside "a view's extrinsics"' six, evaluated against the model the context holds, and ht_estimate_scale is that
 * section's Gauss-Newton loop with it.  depth [B][h][w] and cams [B][12] are ONE view's frames and cameras, one a slot; cloud, model (poses or the state of model
 * `which`) and their bounds are ht_calibrate_view's, the cloud in the same buffer of the context's.  The result is the scale at which the model best explains the frames;
 * applying it stays the caller's ht_scale(ctx, s).
 *   transform  every slot has its own T_b = (pos, q), carried in float64, starting at the camera's pose cams[b][5:12]; y = pos + qrot(q, p) from T_b rounded to fp32.
 *   scale      s is carried in float64 and starts at (double)o.scale0.  HT_SIZE_SHARED: one s for the batch (one user, many frames), N = 1.  HT_SIZE_PER_SLOT: one s a
 *              slot, N = B.
 *   per point  fp32, one IEEE operation after another in the forms of "a view's extrinsics" (dot = (ax bx + ay by) + az bz [+ w]; vector by scalar per component):
 *              w = body 0's position in slot b's poses; e = y - w; u = w + e * (float)(1.0 / s) (the division in float64, then rounded);
 *              plane = closest(bodies of slot b, u), bit for bit the reference's; r0 = dot(plane, (u, 1)); n = plane.xyz; r = (float)s * r0;
 *              J = [n, cross(e, n), r - dot(n, e)] -- the last entry is dr for a relative step dsigma = ds / s; in = |r| <= max_dist.
 *   sums       37 float64 values a slot: k = 0..27 the upper triangle of J J^T row by row ((0,0), (0,1), .. (0,6), (1,1), ..), 28..34 J r, 35 the truncated cost
 *              (r r < m ? r r : m with m = (double)max_dist * (double)max_dist, every point), 36 the inlier count; every product of the two fp32 terms widened, the
 *              first 35 take in ? term : 0.0.  Order: "a view's extrinsics"' (thread t of 256 its points t, t + 256, .. onto +0.0; the wave's xor butterfly 32, 16,
 *              .. 1; the four waves as (w0 + w1) + (w2 + w3)).  Below A is the slot's symmetric 7 x 7, A6 its leading 6 x 6, c = A[0..5][6], a = A[6][6],
 *              g = S[28..33], h = S[34].  No floating-point atomics, nothing depends on arrival.
 *   usable     a slot with fewer than min_points inliers (slot flag HT_SIZE_FEW_INLIERS) or whose pivot below is not > 0 (HT_SIZE_BAD_PIVOT) contributes nothing and
 *              its T keeps its bits.
 *   step       float64, + - * / and sqrt only, no contraction; D = 1 + (double)damping; Cholesky, forward and back substitution and the update of a transform are
 *              those of "a view's extrinsics" (L L^T x = rhs: y_i = (rhs_i - L_i0 y_0 - ..) / L_ii, x_i = (y_i - L_{i+1,i} x_{i+1} - ..) / L_ii).
 *              free_pose = 0 (the poses are trusted; T never moves; a slot's pivot is a):  PER_SLOT dsigma = -h / (a D);  SHARED  S = sum a_b, H = sum h_b over the
 *              usable slots in slot order onto +0.0, dsigma = -H / (S D).
 *              free_pose = 1 (every slot may also shift rigidly about its wrist, which absorbs the pose bias a wrongly sized model leaves):
 *                PER_SLOT  Cholesky of A with A_ii *= D (all seven), d = the solution for rhs -[g, h], dsigma = d[6], the slot's step d[0..5].
 *                SHARED    the bordered system by its Schur complement: every usable slot factors A6 with A6_ii *= D, solves A6 z = c and A6 v = g;
 *                          S = sum (a - c.z), H = sum (h - c.v) over the usable slots in slot order onto +0.0 (x.y = ((((x0 y0 + x1 y1) + x2 y2) + x3 y3) + x4 y4)
 *                          + x5 y5; a slot whose two terms are not finite is not usable); dsigma = -H / (S D); the slot's step d_i = -(v_i + z_i dsigma).
 *              Every moved T_b takes (dt, dw) = d by the update of "a view's extrinsics" about c = (double)w_b; a candidate that is not finite leaves T_b's bits and
 *              sets the slot's BAD_PIVOT (PER_SLOT: and the scale stays too).  In every form s <- s + s * dsigma.
 *   degenerate no usable slot (scale flag HT_SIZE_FEW_INLIERS when every slot has too few inliers, else HT_SIZE_BAD_PIVOT), S not > 0 or dsigma or the new s not
 *              finite (HT_SIZE_BAD_PIVOT): s and every T of that scale keep
 *              their bits.  A new s below (double)scale_lo or above (double)scale_hi becomes that bound (HT_SIZE_CLAMPED; the transforms still take their steps).
 *              A NaN never comes out of finite inputs.
 *   iterations every one of o.iterations (0..64) is one accumulate and one solve launch on the caller's stream, one more pair evaluates the final state.
 *              iterations = 0 scores scale0 at the cameras' poses.
 *   outputs    scale_out fp32 [N], s rounded.  T_out fp32 [B][7], T_b rounded: the cameras' poses when free_pose = 0.  stats float64
 *              [iterations + 1][HT_SIZE_ROW(N, B)]: row i describes the state before step i, row `iterations` the final state (no step, flags FEW_INLIERS only).  A row:
 *              N scale records of HT_SIZE_STATS (inliers, points, truncated cost -- sums over the scale's slots in slot order --, |dsigma| taken (0: none), the s the
 *              row was evaluated at, flag), then B slot records of HT_SIZE_SLOT_STATS (inliers, truncated cost, flag).
 * ht_size_default     range, fraction, max_dist, damping and min_points are ht_calib_default's; HT_SIZE_SHARED, free_pose 1, 10 iterations, scale0 1, scale_lo 0.5,
 *                     scale_hi 2.  NULL options mean these.
 * ht_estimate_scale   host arrays, synchronous.  ht_estimate_scale_dev: device arrays (d_scale_out, d_T_out and d_stats 4-byte aligned), everything enqueued on
 *                     `stream`, no host wait inside but the buffers' re-allocation.  The slots' prepared points, both models' states, the tracker's flags and the model
 *                     are not touched.
 * Refused before anything grows or runs, the context left usable (HT_ERR_ARG / HT_ERR_STATE): everything ht_calibrate_view refuses (scale_out NULL as T_out); a mode
 * or free_pose outside its values; scale0, scale_lo or scale_hi not finite or not 0 < scale_lo <= scale0 <= scale_hi.  Out of scope: left hands (mirror the frames
 * first), mirror planes, several views in one call, per-finger or per-bone proportions (one number scales the whole hand), and applying the result. */
#define HT_SIZE_SHARED 0
#define HT_SIZE_PER_SLOT 1
#define HT_SIZE_STATS 6
#define HT_SIZE_SLOT_STATS 3
#define HT_SIZE_ROW(N, B) ((N) * HT_SIZE_STATS + (B) * HT_SIZE_SLOT_STATS)
#define HT_SIZE_FEW_INLIERS 1
#define HT_SIZE_BAD_PIVOT 2
#define HT_SIZE_CLAMPED 4
typedef struct { float range_lo, range_hi; int fraction, mode, free_pose, iterations; float max_dist, damping; int min_points; float scale0, scale_lo, scale_hi; } ht_size;
int ht_size_default(ht_ctx *ctx, ht_size *o);
int ht_estimate_scale(ht_ctx *ctx, int which, const float *poses, const uint16_t *depth, const float *cams, int w, int h, int B, const ht_size *o, float *scale_out, float *T_out, double *stats);
int ht_estimate_scale_dev(ht_ctx *ctx, int which, const float *d_poses, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, const ht_size *o, float *d_scale_out, float *d_T_out, double *d_stats,
                          void *stream);

/* ---- annotation fit loop ---------------------------------------------------------------------------------------------
 * ht_slowfit          replaces  void HandTracker::slowfit(const std::vector<float3> &points, int hold, const std::vector<Pose> &refpose,
 *                     int steps_ = 6, RigidBody *selectrb = NULL, const float3 &spoint, const float3 &rbpoint, const std::vector<float4> &crays)
 *                     (handtrack.h:786-821) on the handmodel of slots [0,B), with the points ht_stage_prepare left on the device.
 *                     refpose [B][nb][7] (NULL or hold = 0: no RelativeAngularConstraints), select_rb < 0: no nailed bone,
 *                     crays [B][8][4] (first ncray used for the reference's 8 model feature points). */
int ht_set_points(ht_ctx *ctx, int B, const float *points, int cap, const int *npoints);      /* caller-supplied clouds [B][cap][3] instead of ht_stage_prepare's */
int ht_slowfit(ht_ctx *ctx, int B, int hold, const float *refpose, int steps, int select_rb, const float *spoint, const float *rbpoint, const float *crays, int ncray);

/* ---- stage entry points (same kernels, exposed one reference function at a time so parity tests can pin each) -----
 * All take HOST buffers and are synchronous.  `which` selects the model (0 handmodel, 1 othermodel) of slots [0,B).
 * ht_stage_prepare    depth -> CNN input (handtrack.h:700) and sub-sampled point cloud (misc_image.h:409-417, physmodel.h:58-64):
 *                     cnn_in [B][4096] (optional), points [B][HT_MAX_POINTS][4] (optional), npoints [B] (optional).
 * ht_stage_decode     CNNOutputAnalysis (handtrack.h:218-241): cnn_out [B][2304] -> analysis [B][HT_ANALYSIS]:
 *                     crays 8x4 | image_points 8x2 | confidence 8 | vals 16 | wristroll pitch tilt | palmq 4 | finger_clenched 5.
 * ht_stage_fit_error  FitError (handtrack.h:371-399) of model `which` against the prepared points / depth: err [B].
 * ht_stage_cloud_rows CloudConstraints (physmodel.h:164-181) of model `which`, every `stride`-th prepared point, ray origin =
 *                     camera position if use_cam_origin else 0: rows [B][HT_MAX_POINTS][16] (layout: rb0 rb1 position0 position1 normal
 *                     targetdist targetspeednobias forcelimit.xy friction_master), nrows [B].
 * ht_stage_chamber    cloud_chamber (physmodel.h:486-496) with the five directions and the force limit of handtrack.h:774-778, of model `which` against the
 *                     prepared points: rows [B][5*nb][16], nrows [B] (0 unless boundary_planes is set and the frame has more than min_point_num points).
 * ht_stage_contacts   FindShapeShapeContacts (physics.h:451-462): contacts [B][cap][12] (rb0 rb1 normal p0w p1w separation), n [B].
 * ht_stage_fit        one PhysModel::FitPointCloud(points, chamber-rows-if-enabled, HandModelEnhancements) pass on handmodel
 *                     exactly as HandTracker::update runs it (handtrack.h:769-780).
 * ht_stage_multistep  HandTracker::MultiStepSim on othermodel with the given analysis (handtrack.h:642-690). */
int ht_stage_prepare(ht_ctx *ctx, const uint16_t *depth, const float *cams, int B, float *cnn_in, float *points, int *npoints);
int ht_stage_decode(ht_ctx *ctx, const float *cnn_out, const float *cams, int B, float *analysis);
int ht_stage_fit_error(ht_ctx *ctx, int which, int B, float *err);
int ht_stage_cloud_rows(ht_ctx *ctx, int which, int stride, int use_cam_origin, int B, float *rows, int *nrows);
int ht_stage_chamber(ht_ctx *ctx, int which, int B, float *rows, int *nrows);
int ht_stage_contacts(ht_ctx *ctx, int which, int B, int cap, float *contacts, int *ncontacts);
int ht_stage_fit(ht_ctx *ctx, int B);
int ht_stage_multistep(ht_ctx *ctx, const float *analysis, int B);
int ht_stage_multistep_range(ht_ctx *ctx, const float *analysis, int B, int from_step, int to_step);      /* steps [from_step, to_step) of MultiStepSim alone (handtrack.h:660-688) from othermodel's current state: single-step, teacher-forced comparisons */
int ht_stage_scratch_unibody(ht_ctx *ctx, const float *analysis, int B, int n_unibody);

/* ---- caller-built constraint rows ----------------------------------------------------------------------------------------
 * Row layouts: a linear row (LimitLinear, physics.h:267-308) is 16 floats: rb0 rb1 position0[3] position1[3] normal[3] targetdist targetspeednobias
 * forcelimit.x forcelimit.y friction_master (the layout ht_stage_cloud_rows returns); an angular row (LimitAngular, physics.h:239-265) is 8 floats:
 * rb0 rb1 axis[3] targetspin mintorque maxtorque.  A body is its index in PhysModel::rigidbodies, -1 = NULL.  Arrays are [B][cap][16] / [B][cap][8]
 * with per-frame counts; `which` selects the model (0 handmodel, 1 othermodel) of slots [0,B).  Host buffers, synchronous.
 * ht_fit_rows        replaces  void PhysModel::FitPointCloud(const std::vector<float3> &points, std::vector<LimitLinear> linears = {},
 *                    std::vector<LimitAngular> angulars = {}, float microforce = 1.0f) (physmodel.h:345-356): the caller's linear rows, then
 *                    CloudConstraints(points) limited to +-microforce (x physics_weak_force on bodies 0-2), then the joints' nailed rows; the caller's
 *                    angular rows, then the joints' range rows; PhysicsUpdate with collision rows; SanityCheck.  points [B][pcap][3].  As at every call
 *                    site of the reference the joint ranges are first brought up to date from the pose (HandModelEnhancements, handtrack.h:417-420,
 *                    434-440).  The caller's linear rows must act on one body from the world (rb0 == -1), as those of every such call site do
 *                    (landmark rays handtrack.h:672-673, boundary planes :774-778, the annotator's nail :803-810); HT_ERR_ARG otherwise.
 * ht_physics_update  replaces  void PhysicsUpdate(const std::vector<RigidBody*> &rigidbodies, std::vector<LimitLinear> &Linears,
 *                    std::vector<LimitAngular> &Angulars, const std::vector<std::vector<float3>*> &wgeom) (physics.h:543-587) with an empty wgeom: the
 *                    caller's rows are all there is (plus the collision rows when physics_use_collision is set), any mix of one- and two-body rows in
 *                    the caller's order; a friction row (friction_master -1 / -2) must directly follow its master row, as ConstrainContacts emits
 *                    them (physics.h:463-489).  Capacity: 32 groups of up to three consecutive two-body rows on one body pair, 126 angular rows. */
int ht_fit_rows(ht_ctx *ctx, int which, int B, const float *points, int pcap, const int *npoints, const float *linears, int lcap, const int *nlinears,
                const float *angulars, int acap, const int *nangulars, float microforce);
int ht_physics_update(ht_ctx *ctx, int which, int B, const float *linears, int lcap, const int *nlinears, const float *angulars, int acap, const int *nangulars);

/* ---- multi-GPU: the result gather -------------------------------------------------------------------------------------------
 * Frames are independent, so a host shards a batch one GPU (one process, one context) per contiguous block of frames and nothing crosses GPUs but the
 * results (BASELINE north star: "RCCL over xGMI for the result gather only"; the reference is a single-process CPU program and has no counterpart).
 * ht_comm_unique_id   rank 0 makes the 128-byte RCCL id (ncclGetUniqueId); the host program hands it to the other ranks (MPI, a socket, a file ...).
 * ht_comm_init        every rank joins with it (ncclCommInitRank on the context's device).  RCCL is loaded (dlopen) by these two calls only.
 * ht_comm_info        what the communicator itself reports: ranks and this rank's number (ncclCommCount / ncclCommUserRank).
 * ht_gather_poses_dev one ncclAllGather of d_local [frames][nb][7] into d_all [world][frames][nb][7] (device pointers), on the context's communication
 *                     stream behind everything enqueued on `stream` so far: the next step's kernels do not wait for it.  slot (0 / 1) names which of the
 *                     caller's two buffer pairs the call uses; ht_gather_wait(ctx, slot, stream) makes `stream` (NULL: the context's own stream, as everywhere)
 *                     wait for that slot's gather before the pair is reused or read, ht_gather_wait_host(ctx, slot) the calling thread.  A gather issued
 *                     into a slot whose previous gather was never waited for is refused (HT_ERR_STATE): the wait has to stand in front of the work that refills
 *                     the slot's buffers, nothing issued afterwards can order that.  ht_gather_wait_host synchronises the thread also after a stream-side wait.
 * ht_comm_available   1 when RCCL can be loaded here.  ncclCommInitRank blocks until every rank has arrived, so the ranks of a job agree on this (a MIN
 *                     over the host program's own channel) BEFORE any of them calls ht_comm_init; a rank without the library then cannot strand the others.
 * ht_comm_destroy     leaves the communicator (ht_destroy does it too). */
int ht_comm_available(void);
int ht_gather_wait_host(ht_ctx *ctx, int slot);
int ht_comm_unique_id(void *id128);
int ht_comm_init(ht_ctx *ctx, int world, int rank, const void *id128);
int ht_comm_info(ht_ctx *ctx, int *world, int *rank);
int ht_gather_poses_dev(ht_ctx *ctx, const float *d_local, float *d_all, int frames, int slot, void *stream);
int ht_gather_wait(ht_ctx *ctx, int slot, void *stream);
int ht_comm_destroy(ht_ctx *ctx);

/* ---- timing hooks for bench.py: HIP-event time (ms) per named phase accumulated since the last reset.
 * on = 1: only the dominant kernel ("solve") is bracketed (negligible perturbation, used inside the timed region);
 * on = 2: every phase is bracketed and the side streams are serialised (phase table). ----- */
int ht_profile_enable(ht_ctx *ctx, int on);
int ht_profile_read(ht_ctx *ctx, int reset, int max_entries, char *names, int name_stride, float *total_ms, int *launches, int *n_entries);
/* Tuning aid, no reference counterpart: with the environment variable HT_DEBUG_SKIP=2048 every k_solve launch accumulates per-frame
 * statistics (launches, cycles in chains / two-body linear / angular rows / all sweeps, steps, longest chain, row counts, prologue parts), 16 floats per frame. */
int ht_debug_solve_stats(ht_ctx *ctx, int B, float *out, int reset);
int ht_debug_contact_stats(ht_ctx *ctx, int B, float *out, int reset);      /* same for k_contacts: 24 floats per frame (5 about its wave's polytope runs, 7 unused, 12 about the frame) */
/* Test aid: pins which build of the solver kernel runs (0 = chosen per launch; 1-3 the LDS sizes for tile batches / small batches / large frames and models;
 * 4 = a build whose LDS arrays hold nothing, so every frame places its row records in HBM; 6 = the build with four angular-row slots per lane that models with more
 * than 18 joints take).  Placement only: results are identical bit for bit.  7 = the launcher's choice, with the two-body rows of every frame applied through the level
 * schedule (the sweeps of round 4) instead of block by block (csrc/ht_block.hpp): the same rows in the same order, another rounding.  8 = the exact-order sweeps of 5 under
 * the product's forked launch sequence (5 runs an update's kernels in order on one stream). */
int ht_debug_solver_build(ht_ctx *ctx, int which);
int ht_debug_reset_flags(ht_ctx *ctx, int *flags, int n);      /* test aid: flags[i] = 1 if tracker slot i took the full-reset branch (handtrack.h:706-711) in the latest update */
/* Test aid: 5 additionally selects the EXACT-ORDER instantiation of the solver -- the same rows swept by the reference's own LimitLinear::Iter / LimitAngular::Iter
 * (physics.h:251-265, 289-307) in the reference's row order, no fused multiply-adds (update entry points only; tests/test_gpu_exact_solver.py).
 * ht_debug_reset_organisation: how the latest update launched the full-reset branch (0 few frames, 1 many frames, -1 none yet). */
int ht_debug_reset_organisation(ht_ctx *ctx, int *many);
/* Test aid: ht_stage_scratch_unibody for the frames list[0 .. nlist) alone, launched through the flagged-frame list as an update launches its full-reset branch
 * (many_frames 0: one block per CU, the few-frames build; 1: two blocks per CU).  The frames not listed keep their state and their row counts.  HT_ERR_ARG, with nothing
 * uploaded, for a null pointer, nlist outside [0, B], an index outside [0, B) or an index listed twice. */
int ht_debug_row_counts(ht_ctx *ctx, int B, int *nrows);      /* test aid: the cloud-row counts of slots [0, B) as the latest launch that wrote them left them */
int ht_stage_scratch_unibody_listed(ht_ctx *ctx, const float *analysis, int B, int n_unibody, const int *list, int nlist, int many_frames);
/* Test aid: pins the organisation of the contact kernel (0 = chosen per launch: the cooperative kernel whenever the model fits its LDS; 1 cooperative,
 * 2 one lane group per body pair).  Same contacts in the same order either way. */
int ht_debug_contact_kernel(ht_ctx *ctx, int which);
/* Test aid: how the edges between an update's streams are made (0 = the product's events and launch forms; 1 = a record and a wait per edge on events with
 * hipEventDisableTiming alone, as up to round 29).  Waits for the context's work.  Same results either way, bit for bit. */
int ht_debug_stream_edges(ht_ctx *ctx, int mode);
/* Test aid: the kernel a contact launch on B frames takes under that pin: *coop_frames = frames per block of the cooperative kernel (0: the lane-group kernel runs, also
 * under pin 1 when a frame of the model does not fit the cooperative kernel's LDS), *lane_waves = waves per frame of the lane-group kernel (0: the cooperative kernel
 * runs; 2 for models of more than 200 body pairs). */
int ht_debug_contact_plan(ht_ctx *ctx, int B, int *coop_frames, int *lane_waves);
/* Test aid: the launch tables an update makes at its head from the previous update's per-frame costs, here from a cost array the caller gives (one launch slot, host memory):
 * ht_debug_contact_order: the assignment of frames to the cooperative contact kernel's blocks of nfr frames (1-8; epb: frames with polytope runs per block);
 *   order_out[ceil(B / nfr) * nfr], order_out[round * blocks + block] = frame, B = no frame.  work[i] = candidate pairs + 2 x patches | polytope runs << 16.
 * ht_debug_rank_desc: order_out[B] = the frames of every 4096-frame segment by work, largest first, ties by index. */
int ht_debug_contact_order(ht_ctx *ctx, const int *work, int B, int nfr, int epb, int *order_out);
int ht_debug_rank_desc(ht_ctx *ctx, const int *work, int B, int *order_out);
/* Test / measurement aid: 0 (default) = every solve makes its tables (joint groups, angular records, block couplings, chain lists) in k_solve's own one-wave prologue;
 * 1 = k_solve_prep makes them on a side stream beside the contact kernel (csrc/ht_prep.hip; round 6's experiment: k_solve 8 % shorter, the step longer -- profiles/r06_notes.md);
 * 2 = only the pose-only tables (joint groups, angular records, block couplings), on the side stream the cloud rows do not use: also measured slower.
 * Where the tables are made, never what they hold: results are identical bit for bit (tests/test_gpu_solve_tables.py). */
int ht_debug_solve_tables(ht_ctx *ctx, int mode);
/* Test aid: the layer outputs and the errors that the latest training step (ht_cnn_train / ht_cnn_train_dev) left in the context's training scratch, read after
 * every stream of the context has drained.  Indices are CNN::Eval's layers (cnn.h:550-556), errors[i] is the error at the output of layer i (cnn.h:565-572).
 *   act [74768]: a1 [16][60][60] layer 1 (conv 5x5 + tanh) | a3 [16][15][15] layer 3 (two max-pools) | a5 [64][12][12] layer 5 (conv 4x4 + tanh) |
 *                a6 [2304] layer 6 (max-pool) | a8 [2048] layer 8 (fully connected + tanh)
 *   err [64272]: e9 [2304] errors[9] (under the soft-max) | e7 [2048] errors[7] (tanh' folded in) | e6 [2304] errors[6] |
 *                part3 [16][3600] errors[3] as sixteen partial sums, one per group of four conv2 output channels (their sum is the error) |
 *                sqp [9] the soft-max blocks' sums of E^2 (their sum / 2304 is the value Train returns), 7 unused
 * n_act / n_err must be exactly those counts (HT_ERR_ARG); HT_ERR_STATE when the context has not trained yet. */
int ht_debug_train_buffers(ht_ctx *ctx, float *act, size_t n_act, float *err, size_t n_err);
int ht_debug_solve_tables_header(ht_ctx *ctx, int B, int *hdr);      /* tuning aid: the 32 header words of every frame's tables as the latest k_solve_prep left them ([B][32]; words 20-27: cycle stamps of a -DHT_TUNING build) */

#ifdef __cplusplus
}
#endif
#endif
