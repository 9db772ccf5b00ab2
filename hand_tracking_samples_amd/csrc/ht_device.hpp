// ht_device.hpp -- device-side data model shared by the kernels and the C-ABI layer (product code).
//
// HBM layout (per context, capacity = max_batch tracker slots; everything resident for the life of the context):
//   constants  : model (vertices, planes, per-body and per-joint constants), CNN weights (37.8 MB in .cnnb order + conv2 repacked k-major + the last layer repacked for k_fc144_pk, 18.9 MB)
//   per slot   : handmodel / othermodel state [nb][16] floats (pos3 quat4 linmom3 angmom3 pad3), prev_frame_error, initializing
//   per frame  : depth u16[4096] (only for host-buffer calls), cam[12], per net (ht_net: the 64x64-input net's with the context, the 128x128-input net's with its
//                first weights) in[side side], act1[16 P2 P2], act2[64 P3 P3] (cnn_dims), for both nets act3[2048], logits/cnn_out[2304], analysis[84],
//                points float4[HT_MAXPTS] + count, cloud rows [HT_MAXPTS][16], chamber rows [5*nb][16], contacts, solver scratch (pre-computed row stream)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ht_mi355x.h"
#include <stdlib.h>
#include <mutex>
#include "ht_math.hpp"

// Every extern "C" entry point that touches the device makes its context's GPU current for the duration of the call and restores the caller's
// device afterwards: a process may hold contexts on several GPUs and call from any thread (first-use allocations, blocking copies and kernel
// lookups all go to the current device).
struct ht_device_guard
{
	int prev = -1, want;
	explicit ht_device_guard(int dev) : want(dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
	~ht_device_guard() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
	ht_device_guard(const ht_device_guard &) = delete;
	ht_device_guard &operator=(const ht_device_guard &) = delete;
};
// Tuning switches (skip parts of a kernel, serialise streams) exist only in builds made with -DHT_TUNING (HT_TUNING=1 python -m
// hand_tracking_samples_amd.build, used by tools/ablate_*.sh and tools/solve_stats.py): the shipped library ignores the environment.
static inline int ht_tuning_flags()
{
#ifdef HT_TUNING
	static int v = -1;
	if (v < 0) { const char *e = getenv("HT_DEBUG_SKIP"); v = e ? atoi(e) : 0; }
	return v;
#else
	return 0;
#endif
}
// In device code the switches are tested through HT_DBG(flags, bit): a constant 0 in the shipped build, so the kernels carry none of the tuning code
// (no cycle counters, no skip branches), and `flags & bit` in a -DHT_TUNING build.
#ifdef HT_TUNING
#define HT_DBG(flags, bit) ((flags) & (bit))
#else
#define HT_DBG(flags, bit) 0
#endif
static inline int ht_tuning_int(const char *name, int def)
{
#ifdef HT_TUNING
	const char *e = getenv(name); return e ? atoi(e) : def;
#else
	(void)name; return def;
#endif
}
static inline bool ht_tuning_env(const char *name)
{
#ifdef HT_TUNING
	return getenv(name) != nullptr;
#else
	(void)name; return false;
#endif
}

// The dynamic-LDS limit of a family of kernels (every instantiation a launcher may pick), raised on the current device when a launch asks for more than the device's copy of
// the code object has been given so far.  One per launcher, static: contexts of several host threads (one per GPU) launch at the same time, and the limit is up before anybody
// launches with it.  A device beyond the table's 64 gets the attribute set at every launch.
struct ht_lds_limit
{
	std::mutex lock; size_t have[64] = {};
	template <class... K> void raise(size_t bytes, K... kernels)
	{
		int dev = -1; (void)hipGetDevice(&dev); const bool listed = dev >= 0 && dev < 64;
		std::lock_guard<std::mutex> lk(lock);
		if (listed && have[dev] >= bytes) return;
		for (const void *k : { reinterpret_cast<const void *>(kernels)... }) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
		if (listed) have[dev] = bytes;
	}
};

#define HT_MAXPTS 4096          // default point capacity of a context (ht_model_dev::pts_cap): every point of a 64x64 tile, every 4th of a 128x128 frame; a context grows
                                // it when a call brings larger frames (ht_reserve_points)
static_assert(HT_MAXPTS == HT_MAX_POINTS, "public header and kernels disagree on the point capacity");
#define HT_MAXNB 32             // bodies
#define HT_MAXNJ 32             // joints
#define HT_STATE_STRIDE 16      // floats per body in device state arrays
#define HT_ROW 16               // floats per linear row: rb0 rb1 position0[3] position1[3] normal[3] targetdist targetspeednobias fmin fmax friction_master
#define HT_AROW 8               // floats per angular row: rb0 rb1 axis[3] targetspin mintorque maxtorque
#define HT_MAXCONTACT 192       // contacts kept per frame (3 rows each): every touching sample the contact kernel's per-frame pool can hold (GJK_POOL, ht_gjk.hip)
#define HT_MAXCONTACT_LDS 96    // contacts whose groups k_solve's level schedule has LDS tables for; a frame with more applies its two-body linear rows one group at a time from its HBM scratch slot
#define HT_EX_LIN 768           // two-body linear rows of a frame in the exact-order instantiation of the tests (3 rows x (32 joints + 192 contacts) and slack)
#define HT_CONTACT 12           // floats per contact: rb0 rb1 normal[3] p0w[3] p1w[3] separation
#define HT_MAXPAIRS 160         // candidate pair slots per frame
#define HT_CREC 16              // floats per pre-computed single-body row record of the solver scratch (ht_quad.hpp)
#define HT_SCRATCH_TAIL 1288    // records at the end of a frame's scratch slot: its two-body linear groups and angular records when a frame does not fit k_solve's LDS (ht_solver.hip)

// analysis layout (HT_ANALYSIS = 84 floats)
#define HT_AN_CRAYS 0
#define HT_AN_IMGPT 32
#define HT_AN_CONF 48
#define HT_AN_VALS 56
#define HT_AN_ANGLES 72
#define HT_AN_PALMQ 75
#define HT_AN_CLENCH 79

// per-body constants, 32 floats each
#define HT_BC 32
#define HT_BC_MASS 0
#define HT_BC_MASSINV 1
#define HT_BC_RADIUS 2
#define HT_BC_RINNER 3
#define HT_BC_DAMPLEFT 4        // powf(1 - max(damping, physics_damping), dt), physics.h:506 (constant per body)
#define HT_BC_FRICTION 5
#define HT_BC_DIAM 6            // max vertex-vertex distance (lets the contact patch skip provably rejected jiggle runs)
#define HT_BC_COM 8             // 3
#define HT_BC_POS0 12           // 3  position_start
#define HT_BC_Q0 16             // 4  orientation_start
#define HT_BC_TINV 20           // 9  tensorinv_massless, column major
// per-joint constants, 24 floats each: rbi0 rbi1 p0[3] p1[3] rangemin[3] rangemax[3] jointframe[4]
#define HT_JC 24
#define HT_JC_RB0 0
#define HT_JC_RB1 1
#define HT_JC_P0 2
#define HT_JC_P1 5
#define HT_JC_RMIN 8
#define HT_JC_RMAX 11
#define HT_JC_FRAME 14
// per-joint limits of the joint coordinates (ht_joints.hip: ht_joint_limits), 8 floats each: lo[3] hi[3] swapped unbounded-axes-as-bits
#define HT_JL 8
#define HT_JL_LO 0
#define HT_JL_HI 3
#define HT_JL_SWAPPED 6
#define HT_JL_UNBOUNDED 7

struct ht_model_dev
{
	int nb, nj;
	int pts_bound;            // most sub-sampled points a frame of the current call can carry (<= pts_cap; 0 = pts_cap): sizes per-point LDS arrays
	int pts_cap;              // points a frame's slot of the per-point arrays holds (stride of points / cloud rows; >= HT_MAXPTS)
	const int *frame_order;   // the kernels with one block per frame (k_cloud_rows, k_fit_error): block i takes frame frame_order[i] -- inside an update of a batch of several rounds per CU the frames by
	                          // their points, most first, so that a launch ends on short blocks; null: block i takes frame i.  Results do not depend on it
	const float4 *verts;      // all bodies back to back (com-centred collision vertices)
	const float4 *cverts;     // the same vertices with every body padded to whole rows of 16 (pads repeat vertex 0, index 0): the contact kernel's LDS image
	int cvert_off[HT_MAXNB + 1];
	const float4 *planes;     // all bodies back to back (local half-space planes)
	const float *bodyc;       // [nb][HT_BC]
	const float *jointc;      // [nj][HT_JC]
	int vert_off[HT_MAXNB + 1];
	int plane_off[HT_MAXNB + 1];
	unsigned ignore[HT_MAXNB];          // bit j of ignore[i]: body i ignores body j (physmodel.h:260-277, handtrack.h:354-358)
	int collide[HT_MAXNB];
	// UnibodyFit's cube proxy (handtrack.h:454-455)
	float ub_massinv, ub_dampleft; float ub_com[3]; float ub_tinv[9];
};
// float4s kept free behind the LDS copy of the face planes (csrc/ht_cloud.hip: stage_planes).  closest_chunk's face scan reads four faces ahead without a range test
// and discards what lies past a body's last face: up to face npmax + 11 of ANY body, npmax the model's largest face count.  Behind every body but the last that is
// the next bodies' planes; behind the last it is this slack, which has to reach npmax - (faces of the last body) + 12.  16 where all bodies have one count (the hand).
__host__ __device__ inline int ht_plane_slack(const ht_model_dev &M)
{
	int npmax = 0;
	for (int b = 0; b < M.nb; b++) { const int np = M.plane_off[b + 1] - M.plane_off[b]; npmax = np > npmax ? np : npmax; }
	const int need = M.nb > 0 ? npmax - (M.plane_off[M.nb] - M.plane_off[M.nb - 1]) + 12 : 0;
	return need > 16 ? need : 16;
}

struct ht_physics_dev      // physics.h:34-47 after handtrack.h:837-838
{
	float deltaT, restitution, gravity_len, coloumb, biasfactorjoint, biasfactorpositive, falltime_to_ballistic, driftmax;
	int iterations, iterations_post, use_collision;
	float weak_force, bone_sum_error_scale, unibody_force;
	float cos40;          // cos(40*3.14/180) evaluated in double like handtrack.h:437, rounded to float for transport and widened again on use
	double cos40d;        // the double itself
	float jiggle_sin;     // sinf(3.14f/180.0f*4.0f/2.0f), gjk.h:628
};

struct ht_cnn_weights { const float *W1, *B1, *W2p, *B2, *W3, *B3, *W4, *B4, *W4p; };      // W2p, W4p: copies of the conv2 / last-layer weights in the order the matrix kernels read them (ht_cnn.hip)
#define HT_W4_COUNT ((size_t)2048 * 2304)
// The layer dimensions of either net from its input side S (64: 60 -> 15, 12 -> 6, FC 2304; 128: 124 -> 31, 28 -> 14, FC 12544): C1 = conv1's output side,
// P2 = after the two pools, C2 = conv2's output side, P3 = after the third pool; A3 / A6 = floats of a sample's a3 [16][P2][P2] / a6 [64][P3][P3]
template <int S> struct cnn_dims
{
	static constexpr int SIDE = S, C1 = S - 4, P2 = C1 / 4, NP2 = P2 * P2, A3 = 16 * NP2, C2 = P2 - 3, NC2 = C2 * C2, P3 = C2 / 2, NP3 = P3 * P3, A6 = 64 * NP3;
};
// The .cnnb order of the weights (CNN::saveb cnn.h:591-593) from the base pointer; fc_in = inputs of the first fully connected layer (a sample's a6)
template <class T> struct cnnb_layout { T *W1, *B1, *W2, *B2, *W3, *B3, *W4, *B4; };
template <class T> static inline cnnb_layout<T> cnnb_layout_of(T *w, size_t fc_in = cnn_dims<64>::A6)
{
	cnnb_layout<T> L;
	L.W1 = w; L.B1 = L.W1 + 400; L.W2 = L.B1 + 16; L.B2 = L.W2 + 16384; L.W3 = L.B2 + 64; L.B3 = L.W3 + fc_in * 2048; L.W4 = L.B3 + 2048; L.B4 = L.W4 + (size_t)2048 * 2304;
	return L;
}
// The same at run time, for the host layer: floats a frame of the net's input, of its two convolution buffers (act2 is the first FC layer's fc_in) and the .cnnb
// value count; sub: the heat-map camera is camsub(cam, sub)
struct ht_net_dims { int side; size_t in, act1, act2, count; int sub; };
template <int S> constexpr ht_net_dims ht_net_dims_of()
{
	return { S, (size_t)S * S, (size_t)cnn_dims<S>::A3, (size_t)cnn_dims<S>::A6, 400 + 16 + 16384 + 64 + (size_t)cnn_dims<S>::A6 * 2048 + 2048 + (size_t)2048 * 2304 + 2304, S / 16 };
}
static_assert(ht_net_dims_of<64>().in == HT_CNN_IN && ht_net_dims_of<64>().count == HT_CNNB_COUNT, "public header and cnn_dims disagree on the 64x64-input net");
static_assert(ht_net_dims_of<128>().in == HT_CNN128_IN && ht_net_dims_of<128>().count == HT_CNNB128_COUNT, "public header and cnn_dims disagree on the 128x128-input net");
// One pose net of a context (ht_ctx::net, ht_net_of): its weights on the device (.cnnb order, then W2p, then W4p) and the views the kernels take, its input and
// convolution buffers [max_batch][dims.in / act1 / act2], the arena of its mini-batch training step (ht_train_batch.hip) for `cap` samples, grown to the largest batch
// seen (dev_grow), with the latest step's sample count, its label in the profile and the texts of its refusals: no weights (forward pass; training, behind the
// entry point's name), a wrong value count.
struct ht_net
{
	ht_net_dims dims; const char *prof, *missing, *train_missing, *bad_count;
	bool have = false; float *d_weights = nullptr; ht_cnn_weights w = {};
	float *d_in = nullptr, *d_act1 = nullptr, *d_act2 = nullptr;
	struct { float *buf = nullptr; int cap = 0, last = 0; } train;
	// the gradient buffer G [dims.count] of ht_cnn_grad_batch_* (with its first call, or ht_cnn_grad_set_sized), the optimiser's moments m and v (on first need of
	// the kind that keeps them), the count t of Adam steps, the norm, clip factor and partial sums of the latest step (ht_opt_stat_doubles) and whether that step clipped
	struct { float *G = nullptr, *m = nullptr, *v = nullptr; double *stat = nullptr; int t = 0, steps = 0; bool clipped = false; } opt;
};
void ht_launch_pack_w4(const float *W4, float *W4p, hipStream_t s);      // refreshes the packed copy (after a weight upload, after a training step)

// ---- kernel launchers (defined in the .hip files) ----
// what k_prepare can do on the side for the frame it has in hand anyway (each replaces a tiny kernel and its dependent launch gap at the head of an update):
// copy the caller's camera into the context's array, seed both models of the tracker from a start pose (pose taken, momenta zeroed), clear its flags
struct ht_prepare_extra { float *cams_out; float *state0, *state1; const float *start; float *prev_err; int *initializing; int nb; int *zero; };      // zero: an int the kernel clears (the update's list of flagged frames starts empty)
void ht_launch_prepare(const uint16_t *depth, const float *cams, float drangey, int fraction, float *cnn_in, float4 *pts, int *npts, int cap, int B, hipStream_t s, const ht_prepare_extra *extra = nullptr);
void ht_launch_voxel(const float4 *all, const int *nall, int cap, float size, int min_count, float4 *out, int *nout, int B, hipStream_t s);
void ht_launch_prepare_frame(const uint16_t *depth, const float *cams, int w, int h, float drangey, int fraction, float4 *pts, int *npts, int *overflow, int cap, int B, hipStream_t s);
void ht_launch_cnn(const ht_net &net, const float *cnn_in, float *act3, float *logits, int B, hipStream_t s, bool beside_other_work = false);      // the net's act1 / act2 on the way; beside_other_work: another stream's kernel runs beside the net (an update's side branch): picks the launch arrangement, not the results
void ht_launch_softmax_decode(const float *logits, float *cnn_out, const float *cams, float *analysis, int softmax, int B, hipStream_t s, int sub = 4);      // sub: the heat-map camera is camsub(cam, sub)
void ht_launch_cnn_input(const uint16_t *depth, const float *cams, int npx, float drangey, float *cnn_in, int B, hipStream_t s);
