// ht_quality.hip -- tracking accuracy on the device: keypoints of a batch of poses in 3-D and in pixels with their visibility against the depth frame, keypoint errors
// between two pose sets, the depth residual and silhouette overlap of two sets of frames, and poses against frames in one call (an addition).
//
// Reference computations:
//   Skin                           include/handtrack.h:82-84 (pose[bone] * offset), handmodelfeaturepoints :77-81
//   ImageFeaturePoints             include/handtrack.h:92-96 (projectz(cam.pose.inverse() * Skin)); the overlay :632-634, dataexporter.cpp:82,105, annotation-fixer.cpp:315-317
//   DCamera::deprojectz            include/misc_image.h:48 (the whole-pixel convention the visibility test samples the frame by)
//   RigidBody::PositionUser        third_party/physics.h:142 (its inverse brings user poses to what the renderer takes)
// The semantics are include/ht_mi355x.h's "tracking accuracy"; tests/quality_ref.py restates them in numpy and the kernels equal it bit for bit (fp32, one rounding
// per operation in the written order: the library is built without contraction, division and sqrtf are correctly rounded).
//
// Mapping.  Only k_depth_compare moves bytes that matter; the others are launch- and latency-bound.
//   k_keypoints         one thread per (frame, keypoint).  The table comes by value in the kernel arguments (at most 64 entries, 900 bytes); the block's first threads bring
//                       it to the poses' convention (o' = o +- com[bone]) and into LDS once.  A thread reads its bone's pose and its frame's camera straight from global
//                       memory (as k_joint_coords does: a wave covers a few frames whose records are contiguous, every line fetched is used).  Visibility's one depth
//                       load per keypoint is a gather.
//   k_kp_errors         one block per 256 frames, one thread per frame walks the keypoints in order (the ordered fp32 mean).  Per keypoint a wave adds its lanes'
//                       distances in double (__shfl) and counts the hits per threshold (__ballot); each wave leaves its partials in its own LDS row, the block adds
//                       the rows in a fixed order and issues one atomicAdd per quantity into the summary, which the call zeroes first (hipMemsetAsync).
//   k_depth_compare<N>  grid (chunks of a frame, frames).  One thread takes N dwords = 2N pixels of both inputs per load (16 / 8 / 4 bytes by the one width rule, ht_frame_vec_pixels,
//                       on the width and both pointers; <0>: single pixels), about four loads of each input per thread.  Counters in registers (32-bit counts, 64-bit
//                       sums), wave reduction by __shfl_xor, the four waves through LDS, then one 64-bit atomicAdd / atomicMax per quantity per block into info
//                       (zeroed first).  Integers: exact and order-free.
//   k_pose_to_render    one thread per (frame, body): user pose -> centre-of-mass pose -> the camera's frame (skipped for a camera whose pose is the identity bit for bit).
#include <string.h>
#include <math.h>
#include "ht_host.hpp"
#include "ht_frame_vec.hpp"

#define QL_THREADS 256

struct ql_thr { int T; float v[HT_KP_MAX_THR]; };

// ---- keypoints ---------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QL_THREADS) void k_keypoints(const ht_model_dev M, const ql_table T, const float *__restrict__ poses, long long n, int com_poses, const unsigned char *__restrict__ hands,
                                                          const float *__restrict__ cams, const uint16_t *__restrict__ depth, int w, int h, float near_tol, float far_tol,
                                                          float *__restrict__ xyz, float *__restrict__ pix, float *__restrict__ zc, unsigned char *__restrict__ vis)
{
	__shared__ float s_off[HT_KP_MAX * 3];
	__shared__ int s_bone[HT_KP_MAX];
	const int nb = M.nb, K = T.K;
	for (int i = threadIdx.x; i < K; i += QL_THREADS)
	{
		const int b = T.bone[i];
		const v3 com = load3(M.bodyc + b * HT_BC + HT_BC_COM);
		v3 o = load3(T.off + 3 * i);
		if (T.rel[i] && !com_poses) o = o + com; else if (!T.rel[i] && com_poses) o = o - com;
		s_off[3 * i] = o.x; s_off[3 * i + 1] = o.y; s_off[3 * i + 2] = o.z; s_bone[i] = b;
	}
	__syncthreads();
	const long long idx = (long long)blockIdx.x * QL_THREADS + threadIdx.x;
	if (idx >= n) return;
	const long long f = idx / K; const int k = (int)(idx - f * K);
	v3 o = load3(s_off + 3 * k);
	if (hands && hands[f]) o.x = __uint_as_float(__float_as_uint(o.x) ^ 0x80000000u);
	const float *p = poses + ((size_t)f * nb + s_bone[k]) * HT_POSE;
	const v3 X = load3(p) + qrot(load4(p + 3), o);
	if (xyz) { xyz[idx * 3] = X.x; xyz[idx * 3 + 1] = X.y; xyz[idx * 3 + 2] = X.z; }
	if (!cams) return;
	const float *cam = cams + (size_t)f * HT_CAM;
	const v3 v = qrot(qconj(load4(cam + 8)), X - load3(cam + 5));
	const float u0 = v.x / v.z * cam[0] + cam[2], u1 = v.y / v.z * cam[1] + cam[3];
	if (pix) { pix[idx * 2] = u0; pix[idx * 2 + 1] = u1; }
	if (zc) zc[idx] = v.z;
	if (!vis) return;
	const float ux = u0 + 0.5f, uy = u1 + 0.5f;
	unsigned char code;
	if (!(v.z > 0.0f)) code = 4;
	else if (!(ux >= 0.0f && ux < (float)w) || !(uy >= 0.0f && uy < (float)h)) code = 3;
	else
	{
		const int ix = (int)floorf(ux), iy = (int)floorf(uy);      // in [0, w) x [0, h): tested above, in float
		const float d = (float)depth[((size_t)f * h + iy) * w + ix] * cam[4];
		code = d < v.z - near_tol ? 1 : d > v.z + far_tol ? 2 : 0;
	}
	vis[idx] = code;
}

// ---- keypoint errors ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QL_THREADS) void k_kp_errors(const float *__restrict__ a, const float *__restrict__ b, long long B, int K, const ql_thr thr, float *__restrict__ dist,
                                                          float *__restrict__ frame, double *__restrict__ sum_kp, unsigned long long *__restrict__ hits_kp, unsigned long long *__restrict__ hits_frame)
{
	__shared__ double s_sum[QL_THREADS / 64][HT_KP_MAX];
	__shared__ unsigned s_hk[QL_THREADS / 64][HT_KP_MAX_THR], s_hf[QL_THREADS / 64][HT_KP_MAX_THR];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = thr.T;
	const long long f = (long long)blockIdx.x * QL_THREADS + tid;
	const bool live = f < B;
	const float *pa = a + (size_t)(live ? f : 0) * K * 3, *pb = b + (size_t)(live ? f : 0) * K * 3;
	float sum = 0.0f, mx = 0.0f;
	unsigned my_hk = 0u, my_hf = 0u;      // lane t keeps its wave's counts for threshold t
	for (int k = 0; k < K; k++)
	{
		float d = 0.0f;
		if (live)
		{
			const float dx = pa[3 * k] - pb[3 * k], dy = pa[3 * k + 1] - pb[3 * k + 1], dz = pa[3 * k + 2] - pb[3 * k + 2];
			d = sqrtf((dx * dx + dy * dy) + dz * dz);
			if (dist) dist[(size_t)f * K + k] = d;
			sum = sum + d;
			if (d > mx || d != d) mx = d;      // a NaN stays
		}
		double dd = live ? (double)d : 0.0;
		for (int o = 32; o; o >>= 1) dd += __shfl_xor(dd, o, 64);
		if (lane == 0) s_sum[wave][k] = dd;
		for (int t = 0; t < T; t++)
		{
			const unsigned c = (unsigned)__popcll(__ballot(live && d <= thr.v[t]));
			if (lane == t) my_hk += c;
		}
	}
	if (live && frame) { frame[f * 2] = sum / (float)K; frame[f * 2 + 1] = mx; }
	for (int t = 0; t < T; t++)
	{
		const unsigned c = (unsigned)__popcll(__ballot(live && mx <= thr.v[t]));
		if (lane == t) my_hf = c;
	}
	if (lane < T) { s_hk[wave][lane] = my_hk; s_hf[wave][lane] = my_hf; }
	__syncthreads();
	if (sum_kp && tid < K) atomicAdd(&sum_kp[tid], ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid]);
	if (tid < T)
	{
		if (hits_kp) atomicAdd(&hits_kp[tid], (unsigned long long)(s_hk[0][tid] + s_hk[1][tid] + s_hk[2][tid] + s_hk[3][tid]));
		if (hits_frame) atomicAdd(&hits_frame[tid], (unsigned long long)(s_hf[0][tid] + s_hf[1][tid] + s_hf[2][tid] + s_hf[3][tid]));
	}
}

// ---- depth comparison --------------------------------------------------------------------------------------------------------------------------------------------
struct ql_acc { unsigned na, nb, both, close, mx; unsigned long long sabs, ssq; };
__device__ __forceinline__ void ql_pixel(ql_acc &c, unsigned pa, unsigned pb, unsigned lo, unsigned hi, unsigned tol)
{
	const bool ia = pa >= lo && pa < hi, ib = pb >= lo && pb < hi, both = ia && ib;
	const unsigned d = pa > pb ? pa - pb : pb - pa, dm = both ? d : 0u;
	c.na += ia; c.nb += ib; c.both += both; c.close += both && d <= tol;
	c.sabs += dm; c.ssq += (unsigned long long)dm * dm; c.mx = dm > c.mx ? dm : c.mx;
}
// per-thread counters -> one atomic per quantity per block into info[8] of the block's frame
__device__ __forceinline__ void ql_reduce(const ql_acc &c, unsigned long long *info)
{
	__shared__ unsigned long long red[QL_THREADS / 64][8];
	unsigned long long q[7] = { c.na, c.nb, c.both, c.close, c.sabs, c.ssq, c.mx };
#pragma unroll
	for (int i = 0; i < 7; i++)
		for (int o = 32; o; o >>= 1)
		{
			const unsigned long long u = __shfl_xor(q[i], o, 64);
			q[i] = i == 6 ? (u > q[i] ? u : q[i]) : q[i] + u;
		}
	if ((threadIdx.x & 63) == 0)
	{
#pragma unroll
		for (int i = 0; i < 7; i++) red[threadIdx.x >> 6][i] = q[i];
	}
	__syncthreads();
	const int t = threadIdx.x;
	if (t < 7)
	{
		unsigned long long v = red[0][t];
		for (int wv = 1; wv < QL_THREADS / 64; wv++) v = t == 6 ? (red[wv][t] > v ? red[wv][t] : v) : v + red[wv][t];
		if (t == 6) atomicMax(&info[t], v); else atomicAdd(&info[t], v);
	}
}
// a, b [frames][per_frame vectors] -> info [frames][8]; blockIdx.y is the frame
template <int N> __global__ __launch_bounds__(QL_THREADS) void k_depth_compare(const uint16_t *__restrict__ a, const uint16_t *__restrict__ b, unsigned per_frame, unsigned lo, unsigned hi, unsigned tol,
                                                                               unsigned long long *__restrict__ info)
{
	const size_t base = (size_t)blockIdx.y * per_frame;
	const ht_dwords<N> *A = (const ht_dwords<N> *)a + base, *Bv = (const ht_dwords<N> *)b + base;
	ql_acc c = { 0u, 0u, 0u, 0u, 0u, 0ull, 0ull };
	for (unsigned r = blockIdx.x * QL_THREADS + threadIdx.x; r < per_frame; r += gridDim.x * QL_THREADS)
	{
		const ht_dwords<N> x = A[r], y = Bv[r];
#pragma unroll
		for (int i = 0; i < N; i++) { ql_pixel(c, x.v[i] & 0xFFFFu, y.v[i] & 0xFFFFu, lo, hi, tol); ql_pixel(c, x.v[i] >> 16, y.v[i] >> 16, lo, hi, tol); }
	}
	ql_reduce(c, info + (size_t)blockIdx.y * 8);
}
template <> __global__ __launch_bounds__(QL_THREADS) void k_depth_compare<0>(const uint16_t *__restrict__ a, const uint16_t *__restrict__ b, unsigned per_frame, unsigned lo, unsigned hi, unsigned tol,
                                                                             unsigned long long *__restrict__ info)
{
	const size_t base = (size_t)blockIdx.y * per_frame;
	ql_acc c = { 0u, 0u, 0u, 0u, 0u, 0ull, 0ull };
	for (unsigned r = blockIdx.x * QL_THREADS + threadIdx.x; r < per_frame; r += gridDim.x * QL_THREADS) ql_pixel(c, a[base + r], b[base + r], lo, hi, tol);
	ql_reduce(c, info + (size_t)blockIdx.y * 8);
}

// ---- poses for the renderer --------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QL_THREADS) void k_pose_to_render(const ht_model_dev M, const float *__restrict__ poses, const float *__restrict__ cams, long long n, int com_poses, float *__restrict__ out)
{
	const long long idx = (long long)blockIdx.x * QL_THREADS + threadIdx.x;
	if (idx >= n) return;
	const long long f = idx / M.nb; const int b = (int)(idx - f * M.nb);
	const float *p = poses + idx * HT_POSE, *cam = cams + f * HT_CAM;
	v3 pos = load3(p); v4 q = load4(p + 3);
	if (!com_poses) pos = pos + qrot(q, load3(M.bodyc + b * HT_BC + HT_BC_COM));
	const unsigned *cw = (const unsigned *)cam + 5;
	const bool ident = (cw[0] | cw[1] | cw[2] | cw[3] | cw[4] | cw[5]) == 0u && cw[6] == 0x3F800000u;
	if (!ident)
	{
		const v4 qi = qconj(load4(cam + 8));
		pos = qrot(qi, pos - load3(cam + 5));
		q = qmul(qi, q);
	}
	float *o = out + idx * HT_POSE;
	o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
}

// ---- host: the tables --------------------------------------------------------------------------------------------------------------------------------------------
// The table a call names, checked: a built-in one of the context's model as ht_scale left it, or the caller's (ht_host.hpp: ht_kpfit.hip takes it too)
int ql_table_of(ht_ctx *ctx, const char *fn, int which, int K, const int *bones, const float *offsets, const int *rel, ql_table &t)
{
	const std::string f(fn);
	const int nb = ctx->model.nb, nj = ctx->model.nj;
	memset(&t, 0, sizeof t);
	if (which == HT_KP_FEATURE8)
	{
		static const int fbone[8] = { 1, 1, 1, 4, 7, 10, 13, 16 };
		if (!ht_joints_hand_layout(ctx->h_jointc.data(), nb, nj)) { ctx->err = f + ": HT_KP_FEATURE8 is for hand layouts (at least 17 bodies, fingers as chains of bones 5..16 on bone 1)"; return HT_ERR_ARG; }
		t.K = 8;
		for (int k = 0; k < 8; k++) { t.bone[k] = (unsigned char)fbone[k]; t.rel[k] = 1; for (int i = 0; i < 3; i++) t.off[3 * k + i] = ctx->kp_feature8[3 * k + i]; }
		return HT_OK;
	}
	if (which == HT_KP_SKELETON)
	{
		unsigned parents = 0u;
		int k = 1;      // entry 0: body 0's user origin (zeros)
		for (int j = 0; j < nj; j++, k++)
		{
			const float *c = &ctx->h_jointc[(size_t)j * HT_JC];
			const int rb0 = (int)c[HT_JC_RB0], rb1 = (int)c[HT_JC_RB1];
			if (rb0 < 0 || rb0 >= nb || rb1 < 0 || rb1 >= nb) { ctx->err = f + ": a joint of the model names a body it does not have"; return HT_ERR_STATE; }
			parents |= 1u << rb0;
			t.bone[k] = (unsigned char)rb1; for (int i = 0; i < 3; i++) t.off[3 * k + i] = c[HT_JC_P1 + i];
		}
		for (int b = 0; b < nb; b++) if (!((parents >> b) & 1u))
		{
			if (k >= HT_KP_MAX) { ctx->err = f + ": the model's skeleton has more than HT_KP_MAX keypoints"; return HT_ERR_STATE; }
			t.bone[k] = (unsigned char)b; for (int i = 0; i < 3; i++) t.off[3 * k + i] = ctx->h_bodyc[(size_t)b * HT_BC + HT_BC_COM + i];
			k++;
		}
		t.K = k;
		return HT_OK;
	}
	if (which != HT_KP_CALLER) { ctx->err = f + ": which must be HT_KP_FEATURE8, HT_KP_SKELETON or HT_KP_CALLER"; return HT_ERR_ARG; }
	if (K < 1 || K > HT_KP_MAX || !bones || !offsets || !rel) { ctx->err = f + ": a caller table has 1 to HT_KP_MAX entries: bones, offsets and rel"; return HT_ERR_ARG; }
	t.K = K;
	for (int k = 0; k < K; k++)
	{
		if (bones[k] < 0 || bones[k] >= nb) { ctx->err = f + ": bone " + std::to_string(bones[k]) + " of table entry " + std::to_string(k) + " is outside [0, nb)"; return HT_ERR_ARG; }
		if (rel[k] != 0 && rel[k] != 1) { ctx->err = f + ": rel is 0 (user frame) or 1 (centre-of-mass frame)"; return HT_ERR_ARG; }
		for (int i = 0; i < 3; i++) if (!isfinite(offsets[3 * k + i])) { ctx->err = f + ": offsets must be finite"; return HT_ERR_ARG; }
		t.bone[k] = (unsigned char)bones[k]; t.rel[k] = (unsigned char)rel[k];
		for (int i = 0; i < 3; i++) t.off[3 * k + i] = offsets[3 * k + i];
	}
	return HT_OK;
}
// whether any of the outputs overlaps an input or another output (the host forms can see that)
bool ql_any_overlap(const ql_buf *in, int nin, const ql_buf *out, int nout)
{
	for (int o = 0; o < nout; o++)
	{
		for (int i = 0; i < nin; i++) if (ht_ranges_overlap(in[i].p, in[i].bytes, out[o].p, out[o].bytes)) return true;
		for (int i = o + 1; i < nout; i++) if (ht_ranges_overlap(out[i].p, out[i].bytes, out[o].p, out[o].bytes)) return true;
	}
	return false;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int ht_keypoint_table(ht_ctx *ctx, int which, int *K, int *bones, float *offsets, int *rel)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx);
	if (which != HT_KP_FEATURE8 && which != HT_KP_SKELETON) { ctx->err = "ht_keypoint_table: which must be HT_KP_FEATURE8 or HT_KP_SKELETON"; return HT_ERR_ARG; }
	ql_table t;
	{ const int r = ql_table_of(ctx, "ht_keypoint_table", which, 0, nullptr, nullptr, nullptr, t); if (r) return r; }
	if (K) *K = t.K;
	for (int k = 0; k < t.K; k++)
	{
		if (bones) bones[k] = t.bone[k];
		if (rel) rel[k] = t.rel[k];
		if (offsets) for (int i = 0; i < 3; i++) offsets[3 * k + i] = t.off[3 * k + i];
	}
	return HT_OK;
}

static int kp_check(ht_ctx *ctx, const void *poses, int B, int flags, int which, int K, const int *bones, const float *offsets, const int *rel, const void *cams, const void *depth, int w, int h,
                    float near_tol, float far_tol, const void *pix, const void *zc, const void *vis, ql_table &t)
{
	CHECK_MODEL(ctx);
	if (!poses || B < 0) { ctx->err = "ht_keypoints: bad argument"; return HT_ERR_ARG; }
	if (flags & ~HT_KP_COM_POSES) { ctx->err = "ht_keypoints: unknown flags"; return HT_ERR_ARG; }
	{ const int r = ql_table_of(ctx, "ht_keypoints", which, K, bones, offsets, rel, t); if (r) return r; }
	if ((pix || zc || vis) && !cams) { ctx->err = "ht_keypoints: pix, zc and vis need cams"; return HT_ERR_ARG; }
	if (vis)
	{
		if (!depth) { ctx->err = "ht_keypoints: vis needs depth"; return HT_ERR_ARG; }
		if (!ht_frame_dims_ok(w, h)) { ctx->err = "ht_keypoints: w and h between 1 and 4096"; return HT_ERR_ARG; }
		if (!(isfinite(near_tol) && isfinite(far_tol) && near_tol >= 0.0f && far_tol >= 0.0f)) { ctx->err = "ht_keypoints: near_tol and far_tol must be finite and not negative"; return HT_ERR_ARG; }
	}
	return HT_OK;
}
static int kp_launch(ht_ctx *ctx, const ql_table &t, const float *d_poses, int B, int flags, const uint8_t *d_hands, const float *d_cams, const uint16_t *d_depth, int w, int h, float near_tol, float far_tol,
                     float *d_xyz, float *d_pix, float *d_zc, uint8_t *d_vis, hipStream_t s)
{
	const long long n = (long long)B * t.K;
	ht_prof_scope ps(ctx, "k_keypoints", s);
	hipLaunchKernelGGL(k_keypoints, dim3((unsigned)((n + QL_THREADS - 1) / QL_THREADS)), dim3(QL_THREADS), 0, s, ctx->model, t, d_poses, n, (flags & HT_KP_COM_POSES) ? 1 : 0, d_hands, d_cams,
	                   d_vis ? d_depth : nullptr, w, h, near_tol, far_tol, d_xyz, d_pix, d_zc, d_vis);
	return HT_OK;
}
extern "C" int ht_keypoints_dev(ht_ctx *ctx, const float *d_poses, int B, int flags, int which, int K, const int *bones, const float *offsets, const int *rel, const uint8_t *d_hands, const float *d_cams,
                                const uint16_t *d_depth, int w, int h, float near_tol, float far_tol, float *d_xyz, float *d_pix, float *d_zc, uint8_t *d_vis, void *stream)
{
	CHECK_READY(ctx);
	ql_table t;
	{ const int r = kp_check(ctx, d_poses, B, flags, which, K, bones, offsets, rel, d_cams, d_depth, w, h, near_tol, far_tol, d_pix, d_zc, d_vis, t); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	kp_launch(ctx, t, d_poses, B, flags, d_hands, d_cams, d_depth, w, h, near_tol, far_tol, d_xyz, d_pix, d_zc, d_vis, s);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_keypoints(ht_ctx *ctx, const float *poses, int B, int flags, int which, int K, const int *bones, const float *offsets, const int *rel, const uint8_t *hands, const float *cams,
                            const uint16_t *depth, int w, int h, float near_tol, float far_tol, float *xyz, float *pix, float *zc, uint8_t *vis)
{
	CHECK_READY(ctx);
	ql_table t;
	{ const int r = kp_check(ctx, poses, B, flags, which, K, bones, offsets, rel, cams, depth, w, h, near_tol, far_tol, pix, zc, vis, t); if (r) return r; }
	const size_t n = (size_t)B, nk = n * t.K, px = vis ? n * w * h : 0;
	const ql_buf in[4] = { { poses, n * ctx->model.nb * HT_POSE * sizeof(float) }, { hands, n }, { cams, n * HT_CAM * sizeof(float) }, { depth, px * sizeof(uint16_t) } };
	const ql_buf out[4] = { { xyz, nk * 3 * sizeof(float) }, { pix, nk * 2 * sizeof(float) }, { zc, nk * sizeof(float) }, { vis, nk } };
	if (ql_any_overlap(in, 4, out, 4)) { ctx->err = "ht_keypoints: an output overlaps an input or another output"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	ht_seg seg[8] = { { (void *)in[0].p, in[0].bytes, false }, { (void *)hands, n, false }, { (void *)cams, in[2].bytes, false }, { (void *)(vis ? depth : nullptr), in[3].bytes, false },
	                  { xyz, out[0].bytes, true }, { pix, out[1].bytes, true }, { zc, out[2].bytes, true }, { vis, out[3].bytes, true } };
	return ht_staged_call(ctx, seg, 8, [&](hipStream_t s)
	                      {
		                      kp_launch(ctx, t, (const float *)seg[0].dev, B, flags, (const uint8_t *)seg[1].dev, (const float *)seg[2].dev, (const uint16_t *)seg[3].dev, w, h, near_tol, far_tol,
		                                (float *)seg[4].dev, (float *)seg[5].dev, (float *)seg[6].dev, (uint8_t *)seg[7].dev, s);
		                      HIPCHK(ctx, hipGetLastError());
		                      return (int)HT_OK;
	                      });
}

static int ke_check(ht_ctx *ctx, const void *a, const void *b, int B, int K, const float *thr, int T, ql_thr &th)
{
	if (!a || !b || B < 0) { ctx->err = "ht_keypoint_errors: bad argument"; return HT_ERR_ARG; }
	if (K < 1 || K > HT_KP_MAX) { ctx->err = "ht_keypoint_errors: K between 1 and HT_KP_MAX"; return HT_ERR_ARG; }
	if (T < 0 || T > HT_KP_MAX_THR || (T > 0 && !thr)) { ctx->err = "ht_keypoint_errors: T between 0 and HT_KP_MAX_THR thresholds"; return HT_ERR_ARG; }
	memset(&th, 0, sizeof th);
	th.T = T;
	for (int t = 0; t < T; t++) th.v[t] = thr[t];
	return HT_OK;
}
static int ke_enqueue(ht_ctx *ctx, const float *d_a, const float *d_b, int B, int K, const ql_thr &th, float *d_dist, float *d_frame, double *d_sum_kp, int64_t *d_hits_kp, int64_t *d_hits_frame, hipStream_t s)
{
	if (d_sum_kp) HIPCHK(ctx, hipMemsetAsync(d_sum_kp, 0, (size_t)K * sizeof(double), s));
	if (d_hits_kp && th.T) HIPCHK(ctx, hipMemsetAsync(d_hits_kp, 0, (size_t)th.T * sizeof(int64_t), s));
	if (d_hits_frame && th.T) HIPCHK(ctx, hipMemsetAsync(d_hits_frame, 0, (size_t)th.T * sizeof(int64_t), s));
	if (B == 0) return HT_OK;
	ht_prof_scope ps(ctx, "k_kp_errors", s);
	hipLaunchKernelGGL(k_kp_errors, dim3((unsigned)(((long long)B + QL_THREADS - 1) / QL_THREADS)), dim3(QL_THREADS), 0, s, d_a, d_b, (long long)B, K, th, d_dist, d_frame, d_sum_kp,
	                   (unsigned long long *)d_hits_kp, (unsigned long long *)d_hits_frame);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_keypoint_errors_dev(ht_ctx *ctx, const float *d_a, const float *d_b, int B, int K, const float *thr, int T, float *d_dist, float *d_frame, double *d_sum_kp, int64_t *d_hits_kp,
                                      int64_t *d_hits_frame, void *stream)
{
	CHECK_READY(ctx);
	ql_thr th;
	{ const int r = ke_check(ctx, d_a, d_b, B, K, thr, T, th); if (r) return r; }
	if (B == 0) return HT_OK;
	return ke_enqueue(ctx, d_a, d_b, B, K, th, d_dist, d_frame, d_sum_kp, d_hits_kp, d_hits_frame, ht_user_stream(ctx, stream));
}
extern "C" int ht_keypoint_errors(ht_ctx *ctx, const float *a, const float *b, int B, int K, const float *thr, int T, float *dist, float *frame, double *sum_kp, int64_t *hits_kp, int64_t *hits_frame)
{
	CHECK_READY(ctx);
	ql_thr th;
	{ const int r = ke_check(ctx, a, b, B, K, thr, T, th); if (r) return r; }
	const size_t n = (size_t)B, nk = n * K;
	const ql_buf in[2] = { { a, nk * 3 * sizeof(float) }, { b, nk * 3 * sizeof(float) } };
	const ql_buf out[5] = { { dist, nk * sizeof(float) }, { frame, n * 2 * sizeof(float) }, { sum_kp, (size_t)K * sizeof(double) }, { hits_kp, (size_t)T * sizeof(int64_t) }, { hits_frame, (size_t)T * sizeof(int64_t) } };
	if (ql_any_overlap(in, 2, out, 5)) { ctx->err = "ht_keypoint_errors: an output overlaps an input or another output"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	ht_seg seg[7] = { { (void *)a, in[0].bytes, false }, { (void *)b, in[1].bytes, false }, { dist, out[0].bytes, true }, { frame, out[1].bytes, true }, { sum_kp, out[2].bytes, true },
	                  { T ? hits_kp : nullptr, out[3].bytes, true }, { T ? hits_frame : nullptr, out[4].bytes, true } };
	return ht_staged_call(ctx, seg, 7, [&](hipStream_t s)
	                      { return ke_enqueue(ctx, (const float *)seg[0].dev, (const float *)seg[1].dev, B, K, th, (float *)seg[2].dev, (float *)seg[3].dev, (double *)seg[4].dev, (int64_t *)seg[5].dev, (int64_t *)seg[6].dev, s); });
}

static int dc_check(ht_ctx *ctx, const char *fn, const void *a, const void *b, const void *info, int w, int h, int B, int lo, int hi, int tol)
{
	const std::string f(fn);
	if (!a || !b || !info || B < 0) { ctx->err = f + ": bad argument"; return HT_ERR_ARG; }
	if (!ht_frame_dims_ok(w, h)) { ctx->err = f + ": w and h between 1 and 4096"; return HT_ERR_ARG; }
	if (lo < 0 || hi > 65536 || lo >= hi) { ctx->err = f + ": the foreground range is 0 <= lo < hi <= 65536"; return HT_ERR_ARG; }
	if (tol < 0 || tol > 65535) { ctx->err = f + ": tol between 0 and 65535"; return HT_ERR_ARG; }
	return HT_OK;
}
static int dc_enqueue(ht_ctx *ctx, const uint16_t *d_a, const uint16_t *d_b, int w, int h, int B, int lo, int hi, int tol, int64_t *d_info, hipStream_t s)
{
	HIPCHK(ctx, hipMemsetAsync(d_info, 0, (size_t)B * 8 * sizeof(int64_t), s));
	ht_prof_scope ps(ctx, "k_depth_compare", s);
	ht_frame_vec_dispatch(ht_frame_vec_pixels((uintptr_t)d_a | (uintptr_t)d_b, w), [&](auto px)      // both inputs are loaded
	{
		const unsigned per_frame = ((unsigned)w / px) * (unsigned)h;
		const unsigned gx = (per_frame + 4 * QL_THREADS - 1) / (4 * QL_THREADS);      // about four loads of each input per thread
		for (int f0 = 0; f0 < B; f0 += 65535)      // blockIdx.y is the frame
		{
			const unsigned nf = (unsigned)(B - f0 < 65535 ? B - f0 : 65535);
			const size_t off = (size_t)f0 * w * h;
			hipLaunchKernelGGL(k_depth_compare<px / 2>, dim3(gx, nf), dim3(QL_THREADS), 0, s, d_a + off, d_b + off, per_frame, (unsigned)lo, (unsigned)hi, (unsigned)tol,
			                   (unsigned long long *)d_info + (size_t)f0 * 8);
		}
	});
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_depth_compare_dev(ht_ctx *ctx, const uint16_t *d_a, const uint16_t *d_b, int w, int h, int B, int lo, int hi, int tol, int64_t *d_info, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = dc_check(ctx, "ht_depth_compare", d_a, d_b, d_info, w, h, B, lo, hi, tol); if (r) return r; }
	if (B == 0) return HT_OK;
	return dc_enqueue(ctx, d_a, d_b, w, h, B, lo, hi, tol, d_info, ht_user_stream(ctx, stream));
}
extern "C" int ht_depth_compare(ht_ctx *ctx, const uint16_t *a, const uint16_t *b, int w, int h, int B, int lo, int hi, int tol, int64_t *info)
{
	CHECK_READY(ctx);
	{ const int r = dc_check(ctx, "ht_depth_compare", a, b, info, w, h, B, lo, hi, tol); if (r) return r; }
	const size_t bytes = (size_t)B * w * h * sizeof(uint16_t), ib = (size_t)B * 8 * sizeof(int64_t);
	if (ht_ranges_overlap(a, bytes, info, ib) || ht_ranges_overlap(b, bytes, info, ib)) { ctx->err = "ht_depth_compare: info overlaps a frame"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	ht_seg seg[3] = { { (void *)a, bytes, false }, { (void *)b, bytes, false }, { info, ib, true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return dc_enqueue(ctx, (const uint16_t *)seg[0].dev, (const uint16_t *)seg[1].dev, w, h, B, lo, hi, tol, (int64_t *)seg[2].dev, s); });
}

// The composite's own buffers: render poses [B][nb][7], and rendered frames [B][w * h] unless the caller takes them.  Never smaller; growing is one synchronising
// re-allocation, the replacement made first (dev_grow), before anything of the call is enqueued
static int quality_reserve(ht_ctx *ctx, size_t pose_floats, size_t frame_px)
{
	if (pose_floats <= ctx->quality_poses_cap && frame_px <= ctx->quality_frames_cap) return HT_OK;
	HIPCHK(ctx, ht_sync_all(ctx));
	{ const int r = dev_grow(ctx, &ctx->d_quality_poses, &ctx->quality_poses_cap, pose_floats); if (r) return r; }
	return dev_grow(ctx, &ctx->d_quality_frames, &ctx->quality_frames_cap, frame_px);
}
// The two composites differ in their renderer alone: the hulls (ht_pose_depth_residual) or the rasterised meshes at pixel offset 0 (ht_pose_mesh_residual)
static const char *pr_name(bool mesh) { return mesh ? "ht_pose_mesh_residual" : "ht_pose_depth_residual"; }
static int pr_check(ht_ctx *ctx, bool mesh, const void *poses, const void *cams, const void *depth, const void *info, int w, int h, int B, int flags, float far, int lo, int hi, int tol)
{
	const std::string fn = pr_name(mesh);
	CHECK_MODEL(ctx);
	if (!poses || !cams) { ctx->err = fn + ": bad argument"; return HT_ERR_ARG; }
	if (flags & ~HT_KP_COM_POSES) { ctx->err = fn + ": unknown flags"; return HT_ERR_ARG; }
	if (!(far > 0.0f) || !isfinite(far)) { ctx->err = fn + ": far must be positive and finite"; return HT_ERR_ARG; }
	if ((long long)B * ctx->model.nb > 0x7fffffffLL / HT_POSE) { ctx->err = fn + ": more than 2^31 pose floats in one call"; return HT_ERR_ARG; }
	{ const int r = dc_check(ctx, pr_name(mesh), depth, depth, info, w, h, B, lo, hi, tol); if (r) return r; }
	if (mesh && !ctx->d_mesh) { ctx->err = "the model file holds no subdivision meshes (bake it again)"; return HT_ERR_STATE; }
	return HT_OK;
}
static int pr_enqueue(ht_ctx *ctx, bool mesh, const float *d_poses, const float *d_cams, const uint16_t *d_depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *d_info,
                      uint16_t *d_rendered, hipStream_t s)
{
	const long long n = (long long)B * ctx->model.nb;
	uint16_t *frames = d_rendered ? d_rendered : ctx->d_quality_frames;
	{
		ht_prof_scope ps(ctx, "k_pose_to_render", s);
		hipLaunchKernelGGL(k_pose_to_render, dim3((unsigned)((n + QL_THREADS - 1) / QL_THREADS)), dim3(QL_THREADS), 0, s, ctx->model, d_poses, d_cams, n, (flags & HT_KP_COM_POSES) ? 1 : 0, ctx->d_quality_poses);
	}
	{
		const int r = mesh ? ht_raster_mesh_depth_dev(ctx, ctx->d_quality_poses, d_cams, w, h, far, 0.0f, B, frames, nullptr, s) : ht_render_depth_dev(ctx, ctx->d_quality_poses, d_cams, w, h, far, B, frames, nullptr, s);
		if (r) return r;
	}
	return dc_enqueue(ctx, d_depth, frames, w, h, B, lo, hi, tol, d_info, s);
}
static int pr_dev(ht_ctx *ctx, bool mesh, const float *d_poses, const float *d_cams, const uint16_t *d_depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *d_info,
                  uint16_t *d_rendered, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = pr_check(ctx, mesh, d_poses, d_cams, d_depth, d_info, w, h, B, flags, far, lo, hi, tol); if (r) return r; }
	if (B == 0) return HT_OK;
	{ const int r = quality_reserve(ctx, (size_t)B * ctx->model.nb * HT_POSE, d_rendered ? 0 : (size_t)B * w * h); if (r) return r; }
	return pr_enqueue(ctx, mesh, d_poses, d_cams, d_depth, w, h, B, flags, far, lo, hi, tol, d_info, d_rendered, ht_user_stream(ctx, stream));
}
static int pr_host(ht_ctx *ctx, bool mesh, const float *poses, const float *cams, const uint16_t *depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *info, uint16_t *rendered)
{
	CHECK_READY(ctx);
	{ const int r = pr_check(ctx, mesh, poses, cams, depth, info, w, h, B, flags, far, lo, hi, tol); if (r) return r; }
	const size_t n = (size_t)B, bytes = n * w * h * sizeof(uint16_t);
	const ql_buf in[3] = { { poses, n * ctx->model.nb * HT_POSE * sizeof(float) }, { cams, n * HT_CAM * sizeof(float) }, { depth, bytes } };
	const ql_buf out[2] = { { info, n * 8 * sizeof(int64_t) }, { rendered, bytes } };
	if (ql_any_overlap(in, 3, out, 2)) { ctx->err = std::string(pr_name(mesh)) + ": an output overlaps an input or another output"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	{ const int r = quality_reserve(ctx, n * ctx->model.nb * HT_POSE, rendered ? 0 : n * w * h); if (r) return r; }
	ht_seg seg[5] = { { (void *)poses, in[0].bytes, false }, { (void *)cams, in[1].bytes, false }, { (void *)depth, bytes, false }, { info, out[0].bytes, true }, { rendered, bytes, true } };
	return ht_staged_call(ctx, seg, 5, [&](hipStream_t s)
	                      { return pr_enqueue(ctx, mesh, (const float *)seg[0].dev, (const float *)seg[1].dev, (const uint16_t *)seg[2].dev, w, h, B, flags, far, lo, hi, tol, (int64_t *)seg[3].dev, (uint16_t *)seg[4].dev, s); });
}
extern "C" int ht_pose_depth_residual_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, const uint16_t *d_depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *d_info,
                                          uint16_t *d_rendered, void *stream)
{ return pr_dev(ctx, false, d_poses, d_cams, d_depth, w, h, B, flags, far, lo, hi, tol, d_info, d_rendered, stream); }
extern "C" int ht_pose_depth_residual(ht_ctx *ctx, const float *poses, const float *cams, const uint16_t *depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *info, uint16_t *rendered)
{ return pr_host(ctx, false, poses, cams, depth, w, h, B, flags, far, lo, hi, tol, info, rendered); }
extern "C" int ht_pose_mesh_residual_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, const uint16_t *d_depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *d_info,
                                         uint16_t *d_rendered, void *stream)
{ return pr_dev(ctx, true, d_poses, d_cams, d_depth, w, h, B, flags, far, lo, hi, tol, d_info, d_rendered, stream); }
extern "C" int ht_pose_mesh_residual(ht_ctx *ctx, const float *poses, const float *cams, const uint16_t *depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *info, uint16_t *rendered)
{ return pr_host(ctx, true, poses, cams, depth, w, h, B, flags, far, lo, hi, tol, info, rendered); }
