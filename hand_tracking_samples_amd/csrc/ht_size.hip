// ht_size.hip -- the hand's size from tracked frames: PhysModel::scale(s) is a uniform similarity about body 0's position, so a depth point y lies at distance
// s * dist(w + (y - w) / s) from the scaled hand (dist: the unscaled model's closest(), w: the wrist).  Size is a seventh degree of freedom beside ht_calib.hip's six,
// evaluated against the model the context already holds (an addition: every live application of the reference asks the user for the number).
//
// Reference computations:
//   PhysModel::scale(s)                          include/physmodel.h:196-219, :304-319   (what the estimate stands for; nothing here rebuilds a model)
//   PointCloud / FallsWithinRange / deprojectz   include/misc_image.h:409-417, :24, :48        (the cloud: k_calib_cloud's)
//   closest(rigidbodies, v), mostabove           include/physmodel.h:137-162, :127-131         (ca_closest, ht_calib_common.hpp)
// The semantics, the order of every sum included, are include/ht_mi355x.h's "the hand's size"; tests/size_ref.py restates them in numpy and the kernels equal it bit for
// bit, fp32 per point and float64 from the normal equations on (the library is built without contraction).
//
// Mapping.  The cloud, its counts and the float64 transforms are ht_calib.hip's buffers, filled by its k_calib_cloud (one transform a slot).  k_size_accum: k_calib_accum's
// block (256 threads a slot, the planes and the body table staged once, a lane a point at stride 256), the point pulled towards the wrist by 1 / s before closest() and
// the residual stretched by s after it; 37 float64 sums in registers, reduced by ca_reduce.  k_size_solve: 256 threads, a thread a slot.  PER_SLOT: a block takes 256
// slots, every thread solves its own damped 7 x 7 (or its scalar) and commits its scale and transform.  SHARED: one block; every thread factors its slots' 6 x 6 blocks
// and leaves the Schur pieces beside the slot's sums, seven lanes add a column each in slot order, lane 0 takes the scale's step, and every thread moves its slots' transforms.
// Every loop is bounded by a count known when it is entered; no lane waits for another but at the block's barriers; no floating-point atomic anywhere.
#include "ht_calib_common.hpp"

#define SZ_NSUM 37     // 28 of J J^T's upper triangle, 7 of J r, the truncated cost, the inliers
#define SZ_COST 35
#define SZ_INL 36
#define SZ_PART 56     // doubles a slot's partial takes: the sums, the point count (37), then the solve's pieces: z 40..45, v 46..51, a - c.z 52, h - c.v 53, the slot's flag 54
#define SZ_Z 40
#define SZ_V 46
#define SZ_SA 52
#define SZ_SH 53
#define SZ_FLAG 54
#define SZ_SOLVE_THREADS 256

// poses as k_calib_accum's; T [B][8]; sc [N]: the scales (first: scale0 instead, and block n writes sc[n]); part [B][SZ_PART]
__global__ __launch_bounds__(CA_THREADS) void k_size_accum(const ht_model_dev M, const float *__restrict__ poses, int pose_stride, const float4 *__restrict__ pts, int stride, const int *__restrict__ npts,
                                                           const double *__restrict__ T, double *__restrict__ sc, int per_slot, int first, float scale0, float max_dist, double *__restrict__ part)
{
	__shared__ __align__(16) float tab[HT_MAXNB * CA_BT];
	__shared__ double red[CA_THREADS / 64][SZ_NSUM];
	const int t = threadIdx.x, b = blockIdx.x;
	const int nb = M.nb;
	ca_stage(M, poses, pose_stride, b, tab);
	const double *Tb = T + (size_t)b * 8;
	const v3 tp = V3((float)Tb[0], (float)Tb[1], (float)Tb[2]);
	const v4 tq = V4((float)Tb[3], (float)Tb[4], (float)Tb[5], (float)Tb[6]);
	const double s = first ? (double)scale0 : sc[per_slot ? b : 0];
	if (first && t == 0 && (per_slot || b == 0)) sc[b] = s;
	const float inv = (float)(1.0 / s), sf = (float)s;
	const double md2 = (double)max_dist * (double)max_dist;
	const int n = npts[b];
	const float4 *src = pts + (size_t)b * stride;
	double acc[SZ_NSUM];
#pragma unroll
	for (int k = 0; k < SZ_NSUM; k++) acc[k] = 0.0;
	__syncthreads();
	const v3 wr = V3(tab[0], tab[1], tab[2]);      // body 0's position
	for (int i = t; i < n; i += CA_THREADS)
	{
		const float4 p = src[i];
		const v3 y = tp + qrot(tq, V3(p.x, p.y, p.z));
		const v3 e = y - wr;
		const v3 u = wr + e * inv;
		const v4 pl = ca_closest(tab, nb, u);
		const float r = sf * dot_plane(pl, u);
		const v3 nn = xyz(pl), m = cross(e, nn);
		const float J[7] = { nn.x, nn.y, nn.z, m.x, m.y, m.z, r - dot(nn, e) };
		const bool in = fabsf(r) <= max_dist;
		int k = 0;
#pragma unroll
		for (int i0 = 0; i0 < 7; i0++)
#pragma unroll
			for (int j0 = i0; j0 < 7; j0++, k++) acc[k] += in ? (double)J[i0] * (double)J[j0] : 0.0;
#pragma unroll
		for (int i0 = 0; i0 < 7; i0++) acc[28 + i0] += in ? (double)J[i0] * (double)r : 0.0;
		const double r2 = (double)r * (double)r;
		acc[SZ_COST] += r2 < md2 ? r2 : md2;
		acc[SZ_INL] += in ? 1.0 : 0.0;
	}
	ca_reduce<SZ_NSUM>(acc, red, part + (size_t)b * SZ_PART, n);
}

struct sz_step { double damping, min_points, lo, hi; int B, shared, free_pose, last; };
// entry (i, j), i <= j, of a 7 x 7 upper triangle stored row by row
__device__ __forceinline__ constexpr int sz_at(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }
__device__ __forceinline__ double sz_dot6(const double (&a)[6], const double (&b)[6]) { return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]; }
// s + s ds kept inside [lo, hi]
__device__ __forceinline__ double sz_clamped(double sn, const sz_step &o, int &flag)
{
	if (sn < o.lo) { flag |= HT_SIZE_CLAMPED; return o.lo; }
	if (sn > o.hi) { flag |= HT_SIZE_CLAMPED; return o.hi; }
	return sn;
}
// slot b's transform by d about body 0's position; false (T keeps its bits) unless every figure is finite
__device__ __forceinline__ bool sz_move(double *Ts, const double (&d)[6], const float *__restrict__ wrist)
{
	double n[7];
	bool ok = ca_candidate(Ts, d, (double)wrist[0], (double)wrist[1], (double)wrist[2], n);
#pragma unroll
	for (int i = 0; i < 6; i++) ok = ok && ca_finite(d[i]);
	if (ok)
	{
#pragma unroll
		for (int i = 0; i < 7; i++) Ts[i] = n[i];
	}
	return ok;
}
__device__ __forceinline__ void sz_slot_out(const double *Ts, float *__restrict__ T_out, unsigned *rec, double inliers, double cost, int flag)
{
#pragma unroll
	for (int i = 0; i < 7; i++) T_out[i] = (float)Ts[i];
	ca_store(rec + 0, inliers); ca_store(rec + 2, cost); ca_store(rec + 4, (double)flag);
}
__device__ __forceinline__ void sz_scale_out(unsigned *rec, double inliers, double points, double cost, double ds, double s, int flag)
{
	ca_store(rec + 0, inliers); ca_store(rec + 2, points); ca_store(rec + 4, cost); ca_store(rec + 6, fabs(ds)); ca_store(rec + 8, s); ca_store(rec + 10, (double)flag);
}

// part [B][SZ_PART] -> sc [N] and T [B][8] stepped (unless last), scale_out [N], T_out [B][7], row: [N][HT_SIZE_STATS] then [B][HT_SIZE_SLOT_STATS], as words.
// Body 0 of slot b at poses + b nb pose_stride
__global__ __launch_bounds__(SZ_SOLVE_THREADS) void k_size_solve(double *__restrict__ part, const float *__restrict__ poses, int pose_stride, int nb, const sz_step o, double *__restrict__ T,
                                                                 double *__restrict__ sc, float *__restrict__ scale_out, float *__restrict__ T_out, unsigned *__restrict__ row)
{
	__shared__ double sh[10];
	const int t = threadIdx.x, B = o.B;
	const double damp = 1.0 + o.damping;
	unsigned *srec = row + (size_t)(o.shared ? 1 : B) * HT_SIZE_STATS * 2;
	if (!o.shared)
	{
		const int b = blockIdx.x * SZ_SOLVE_THREADS + t;
		if (b >= B) return;
		const double *p = part + (size_t)b * SZ_PART;
		double S[SZ_NSUM + 1];
#pragma unroll
		for (int k = 0; k <= SZ_NSUM; k++) S[k] = p[k];
		double *Ts = T + (size_t)b * 8;
		const double s = sc[b];
		double ds = 0.0, sn = s;
		int flag = S[SZ_INL] < o.min_points ? HT_SIZE_FEW_INLIERS : 0, sflag = flag;
		if (!o.last && !flag)
		{
			bool ok;
			double d[7];
			if (o.free_pose)
			{
				double L[7][7], g[7];
#pragma unroll
				for (int i = 0; i < 7; i++)
				{
#pragma unroll
					for (int j = i; j < 7; j++) L[j][i] = S[sz_at(i, j)];
					L[i][i] = L[i][i] * damp; g[i] = -S[28 + i];
				}
				ok = ca_cholesky<7>(L);
				ca_substitute<7>(L, g, d);
			}
			else
			{
				ok = S[27] > 0.0;
				d[6] = -S[34] / (S[27] * damp);
			}
			const double c = s + s * d[6];
			ok = ok && ca_finite(d[6]) && ca_finite(c);
			if (ok && o.free_pose)
			{
				const double dd[6] = { d[0], d[1], d[2], d[3], d[4], d[5] };
				ok = sz_move(Ts, dd, poses + (size_t)b * (unsigned)nb * (unsigned)pose_stride);
			}
			if (ok) { ds = d[6]; sn = sz_clamped(c, o, sflag); sc[b] = sn; }
			else { flag |= HT_SIZE_BAD_PIVOT; sflag |= HT_SIZE_BAD_PIVOT; }
		}
		scale_out[b] = (float)sn;
		sz_scale_out(row + (size_t)b * HT_SIZE_STATS * 2, S[SZ_INL], S[SZ_NSUM], S[SZ_COST], ds, s, sflag);
		sz_slot_out(Ts, T_out + (size_t)b * 7, srec + (size_t)b * HT_SIZE_SLOT_STATS * 2, S[SZ_INL], S[SZ_COST], flag);
		return;
	}
	// SHARED.  1: every slot's Schur pieces
	for (int b = t; b < B; b += SZ_SOLVE_THREADS)
	{
		double *p = part + (size_t)b * SZ_PART;
		double z[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, v[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, sa = 0.0, sb = 0.0;
		int flag = p[SZ_INL] < o.min_points ? HT_SIZE_FEW_INLIERS : 0;
		if (!o.last && !flag)
		{
			bool ok;
			if (o.free_pose)
			{
				double L[6][6], c[6], g[6];
#pragma unroll
				for (int i = 0; i < 6; i++)
				{
#pragma unroll
					for (int j = i; j < 6; j++) L[j][i] = p[sz_at(i, j)];
					L[i][i] = L[i][i] * damp; c[i] = p[sz_at(i, 6)]; g[i] = p[28 + i];
				}
				ok = ca_cholesky<6>(L);
				ca_substitute<6>(L, c, z);
				ca_substitute<6>(L, g, v);
				sa = p[27] - sz_dot6(c, z); sb = p[34] - sz_dot6(c, v);
			}
			else { sa = p[27]; sb = p[34]; ok = sa > 0.0; }
			if (!(ok && ca_finite(sa) && ca_finite(sb))) flag |= HT_SIZE_BAD_PIVOT;
		}
#pragma unroll
		for (int i = 0; i < 6; i++) { p[SZ_Z + i] = z[i]; p[SZ_V + i] = v[i]; }
		p[SZ_SA] = sa; p[SZ_SH] = sb; p[SZ_FLAG] = (double)flag;
	}
	__syncthreads();
	// 2: the slots in slot order, a lane a column: S, H (the usable slots), inliers, points, cost (every slot), the usable slots, the slots with too few inliers
	if (t < 7)
	{
		const int col = t == 0 ? SZ_SA : t == 1 ? SZ_SH : t == 2 ? SZ_INL : t == 3 ? SZ_NSUM : t == 4 ? SZ_COST : SZ_FLAG;
		double v = 0.0;
		for (int b = 0; b < B; b++)
		{
			const double *p = part + (size_t)b * SZ_PART;
			const bool usable = p[SZ_FLAG] == 0.0;
			const double x = p[col];
			v += t < 2 ? (usable ? x : 0.0) : t == 5 ? (usable ? 1.0 : 0.0) : t == 6 ? (x == (double)HT_SIZE_FEW_INLIERS ? 1.0 : 0.0) : x;
		}
		sh[t] = v;
	}
	__syncthreads();
	if (t == 0)
	{
		const double s = sc[0];
		double ds = 0.0, sn = s;
		int flag = sh[5] != 0.0 ? 0 : sh[6] == (double)B ? HT_SIZE_FEW_INLIERS : HT_SIZE_BAD_PIVOT;      // no usable slot
		bool go = false;
		if (!o.last && !flag)
		{
			const double d = -sh[1] / (sh[0] * damp), c = s + s * d;
			if (sh[0] > 0.0 && ca_finite(d) && ca_finite(c)) { go = true; ds = d; sn = sz_clamped(c, o, flag); sc[0] = sn; }
			else flag |= HT_SIZE_BAD_PIVOT;
		}
		scale_out[0] = (float)sn;
		sz_scale_out(row, sh[2], sh[3], sh[4], ds, s, flag);
		sh[7] = ds; sh[8] = go ? 1.0 : 0.0;
	}
	__syncthreads();
	// 3: every slot's transform
	const double ds = sh[7];
	const bool go = sh[8] != 0.0;
	for (int b = t; b < B; b += SZ_SOLVE_THREADS)
	{
		const double *p = part + (size_t)b * SZ_PART;
		double *Ts = T + (size_t)b * 8;
		int flag = (int)p[SZ_FLAG];
		if (go && !flag && o.free_pose)
		{
			double d[6];
#pragma unroll
			for (int i = 0; i < 6; i++) d[i] = -(p[SZ_V + i] + p[SZ_Z + i] * ds);
			if (!sz_move(Ts, d, poses + (size_t)b * (unsigned)nb * (unsigned)pose_stride)) flag |= HT_SIZE_BAD_PIVOT;
		}
		sz_slot_out(Ts, T_out + (size_t)b * 7, srec + (size_t)b * HT_SIZE_SLOT_STATS * 2, p[SZ_INL], p[SZ_COST], flag);
	}
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int ht_size_default(ht_ctx *ctx, ht_size *o)
{
	if (!ctx || !o) return HT_ERR_ARG;
	ht_calib c; ht_calib_default(ctx, &c);
	o->range_lo = c.range_lo; o->range_hi = c.range_hi; o->fraction = c.fraction; o->max_dist = c.max_dist; o->damping = c.damping; o->min_points = c.min_points;
	o->mode = HT_SIZE_SHARED; o->free_pose = 1; o->iterations = 10; o->scale0 = 1.0f; o->scale_lo = 0.5f; o->scale_hi = 2.0f;
	return HT_OK;
}
struct sz_call { ht_size o; ca_call c; };      // c: the cloud's part of the call, as ht_calibrate_view checks and sizes it (c.N: scales)
// every refusal that needs no device, before anything grows or runs (a context that never came up answers them too)
int ht_size_check(ht_ctx *ctx, const char *fn, int which, const void *poses, const void *depth, const void *cams, int w, int h, int B, const ht_size *opt, const void *scale_out, const void *T_out, const void *stats,
                  sz_call &c)
{
	const std::string f = fn;
	if (!scale_out || !T_out || !stats) { ctx->err = f + ": scale_out [N], T_out [B][7] and stats [iterations + 1][HT_SIZE_ROW(N, B)] are needed"; return HT_ERR_ARG; }
	ht_size d; ht_size_default(ctx, &d);
	if (opt) d = *opt;
	if (d.mode != HT_SIZE_SHARED && d.mode != HT_SIZE_PER_SLOT) { ctx->err = f + ": a bad mode (HT_SIZE_SHARED or HT_SIZE_PER_SLOT)"; return HT_ERR_ARG; }
	if (d.free_pose != 0 && d.free_pose != 1) { ctx->err = f + ": a bad free_pose (0: the poses are trusted, 1: every slot may shift about its wrist)"; return HT_ERR_ARG; }
	ht_calib k;
	k.range_lo = d.range_lo; k.range_hi = d.range_hi; k.fraction = d.fraction; k.mode = d.mode == HT_SIZE_PER_SLOT ? HT_CALIB_PER_SLOT : HT_CALIB_RIG; k.iterations = d.iterations;
	k.max_dist = d.max_dist; k.damping = d.damping; k.min_points = d.min_points; k.centre[0] = k.centre[1] = k.centre[2] = 0.0f;
	{ const int r = ht_calib_check(ctx, fn, which, poses, depth, cams, w, h, B, &k, T_out, stats, c.c); if (r) return r; }
	if (!isfinite(d.scale0) || !isfinite(d.scale_lo) || !isfinite(d.scale_hi) || !(d.scale_lo > 0.0f) || !(d.scale_lo <= d.scale0) || !(d.scale0 <= d.scale_hi))
	{ ctx->err = f + ": a bad scale0, scale_lo or scale_hi (finite, 0 < scale_lo <= scale0 <= scale_hi)"; return HT_ERR_ARG; }
	c.o = d;
	return HT_OK;
}
static const size_t SZ_LDS_FIXED = sizeof(float) * HT_MAXNB * CA_BT + sizeof(double) * (CA_THREADS / 64) * SZ_NSUM + 64;
// the cloud's buffers (ht_calib_reserve) and this file's two, by the same rule: one synchronising re-allocation, the outgrown buffers dropped
static int size_reserve(ht_ctx *ctx, const char *fn, const sz_call &c, int B)
{
	{ const int r = ht_calib_reserve(ctx, fn, c.c, B, SZ_LDS_FIXED); if (r) return r; }
	if ((size_t)B <= ctx->size_B) return HT_OK;
	ht_device_guard dev_guard_(ctx->device);
	HIPCHK(ctx, ht_sync_all(ctx));
	double *part = nullptr, *s = nullptr;
	int r;
	if ((r = dev_alloc(ctx, &part, (size_t)B * SZ_PART)) || (r = dev_alloc(ctx, &s, (size_t)B))) return r;
	drop_alloc(ctx, ctx->d_size_part); drop_alloc(ctx, ctx->d_size_s);
	ctx->d_size_part = part; ctx->d_size_s = s; ctx->size_B = (size_t)B;
	return HT_OK;
}
static size_t size_row(const sz_call &c, int B) { return (size_t)HT_SIZE_ROW(c.c.N, B); }
// the launches, on s alone: the cloud, then iterations + 1 times the pair (accumulate, solve); the last pair evaluates the final state and steps nothing
static int size_enqueue(ht_ctx *ctx, const sz_call &c, int which, const float *d_poses, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, float *d_scale_out, float *d_T_out, double *d_stats,
                        hipStream_t s)
{
	const ht_size &o = c.o;
	const int per_slot = o.mode == HT_SIZE_PER_SLOT ? 1 : 0, stride = (int)ctx->calib_stride;
	const float *poses = d_poses ? d_poses : ctx->d_state[which];
	const int pose_stride = d_poses ? HT_POSE : HT_STATE_STRIDE;
	ht_calib_cloud(ctx, c.c, d_depth, d_cams, w, h, B, 1, s);
	const size_t dyn = (size_t)ctx->model.plane_off[ctx->model.nb] * sizeof(float4);
	static ht_lds_limit limit; limit.raise(dyn, k_size_accum);
	const unsigned blocks = per_slot ? (unsigned)((B + SZ_SOLVE_THREADS - 1) / SZ_SOLVE_THREADS) : 1u;
	for (int it = 0; it <= o.iterations; it++)
	{
		{
			ht_prof_scope ps(ctx, "k_size_accum", s);
			hipLaunchKernelGGL(k_size_accum, dim3((unsigned)B), dim3(CA_THREADS), dyn, s, ctx->model, poses, pose_stride, ctx->d_calib_pts, stride, ctx->d_calib_n, ctx->d_calib_T, ctx->d_size_s, per_slot,
			                   it == 0 ? 1 : 0, o.scale0, o.max_dist, ctx->d_size_part);
		}
		const sz_step st = { (double)o.damping, (double)o.min_points, (double)o.scale_lo, (double)o.scale_hi, B, per_slot ? 0 : 1, o.free_pose, it == o.iterations ? 1 : 0 };
		ht_prof_scope ps(ctx, "k_size_solve", s);
		hipLaunchKernelGGL(k_size_solve, dim3(blocks), dim3(SZ_SOLVE_THREADS), 0, s, ctx->d_size_part, poses, pose_stride, ctx->model.nb, st, ctx->d_calib_T, ctx->d_size_s, d_scale_out, d_T_out,
		                   (unsigned *)d_stats + (size_t)it * size_row(c, B) * 2);
	}
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_estimate_scale_dev(ht_ctx *ctx, int which, const float *d_poses, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, const ht_size *o, float *d_scale_out, float *d_T_out,
                                     double *d_stats, void *stream)
{
	if (!ctx) return HT_ERR_ARG;
	sz_call c;
	{ const int r = ht_size_check(ctx, "ht_estimate_scale_dev", which, d_poses, d_depth, d_cams, w, h, B, o, d_scale_out, d_T_out, d_stats, c); if (r) return r; }
	if (((uintptr_t)d_scale_out | (uintptr_t)d_T_out | (uintptr_t)d_stats) & 3) { ctx->err = "ht_estimate_scale_dev: d_scale_out, d_T_out and d_stats must be 4-byte aligned"; return HT_ERR_ARG; }
	{ const int r = size_reserve(ctx, "ht_estimate_scale_dev", c, B); if (r) return r; }
	ht_device_guard dev_guard_(ctx->device);
	return size_enqueue(ctx, c, which, d_poses, d_depth, d_cams, w, h, B, d_scale_out, d_T_out, d_stats, ht_user_stream(ctx, stream));
}
// the host form's staging plan (no device needed): inputs poses, depth, cams; outputs scale_out, T_out, stats
int ht_size_segments(const sz_call &c, int nb, const float *poses, const uint16_t *depth, const float *cams, int w, int h, int B, float *scale_out, float *T_out, double *stats, ht_seg *seg)
{
	seg[0] = ht_seg{ (void *)poses, (size_t)B * nb * HT_POSE * sizeof(float), false, nullptr };
	seg[1] = ht_seg{ (void *)depth, (size_t)B * w * h * sizeof(uint16_t), false, nullptr };
	seg[2] = ht_seg{ (void *)cams, (size_t)B * HT_CAM * sizeof(float), false, nullptr };
	seg[3] = ht_seg{ scale_out, (size_t)c.c.N * sizeof(float), true, nullptr };
	seg[4] = ht_seg{ T_out, (size_t)B * 7 * sizeof(float), true, nullptr };
	seg[5] = ht_seg{ stats, (size_t)(c.o.iterations + 1) * size_row(c, B) * sizeof(double), true, nullptr };
	return 6;
}
extern "C" int ht_estimate_scale(ht_ctx *ctx, int which, const float *poses, const uint16_t *depth, const float *cams, int w, int h, int B, const ht_size *o, float *scale_out, float *T_out, double *stats)
{
	if (!ctx) return HT_ERR_ARG;
	sz_call c;
	{ const int r = ht_size_check(ctx, "ht_estimate_scale", which, poses, depth, cams, w, h, B, o, scale_out, T_out, stats, c); if (r) return r; }
	ht_seg seg[6];
	const int n = ht_size_segments(c, ctx->model.nb, poses, depth, cams, w, h, B, scale_out, T_out, stats, seg);
	{
		const ql_buf in[3] = { { seg[0].host, seg[0].bytes }, { seg[1].host, seg[1].bytes }, { seg[2].host, seg[2].bytes } };
		const ql_buf out[3] = { { seg[3].host, seg[3].bytes }, { seg[4].host, seg[4].bytes }, { seg[5].host, seg[5].bytes } };
		if (ql_any_overlap(in, 3, out, 3)) { ctx->err = "ht_estimate_scale: an output overlaps an input or another output"; return HT_ERR_ARG; }
	}
	{ const int r = size_reserve(ctx, "ht_estimate_scale", c, B); if (r) return r; }
	ht_device_guard dev_guard_(ctx->device);
	return ht_staged_call(ctx, seg, n, [&](hipStream_t s)
	                      {
		                      return size_enqueue(ctx, c, which, (const float *)seg[0].dev, (const uint16_t *)seg[1].dev, (const float *)seg[2].dev, w, h, B, (float *)seg[3].dev, (float *)seg[4].dev,
		                                          (double *)seg[5].dev, s);
	                      });
}
