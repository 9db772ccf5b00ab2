// ht_calib.hip -- a view's extrinsics from the tracked hand: the view's depth pixels lie on the tracked model's surface, so the view's cloud is registered rigidly against
// the models of a batch of frames, a Gauss-Newton loop around the tracker's own closest() (an addition: the reference never calibrates anything).
//
// Reference computations:
//   PointCloud / FallsWithinRange / deprojectz   include/misc_image.h:409-417, :24, :48        (the cloud: ht_prepare.hpp's pieces, k_fuse_views' walk)
//   takesubsample (every fraction-th point)      include/physmodel.h:58-64
//   closest(rigidbodies, v), mostabove           include/physmodel.h:137-162, :127-131
// The semantics, the order of every sum included, are include/ht_mi355x.h's "a view's extrinsics"; tests/calib_ref.py restates them in numpy (closest() through the
// oracle's ho_closest) and the kernels equal it bit for bit, fp32 per point and float64 from the normal equations on (the library is built without contraction).
//
// Mapping.  k_calib_cloud: one block a slot, fv_emit's tile walk with a view that has neither pose nor plane; its first lanes widen the guess into the float64 T.
// k_calib_accum: one block of 256 threads a slot.  All face planes of the model go to LDS once and one body table (CA_BT floats a body, a lane a body), as k_split_model
// stages them; then a lane a point at stride 256 for both walks of closest(), keeping the winning plane and not only its distance.  The 29 float64 sums live in
// registers; a wave reduces them by a fixed xor butterfly (every lane ends with the same bits), the four waves meet through 4 x 29 doubles of LDS and 29 lanes add them as
// (w0 + w1) + (w2 + w3).  Partials go out per slot.  k_calib_solve: one block of 64 lanes a transform; a lane a sum adds the slots' partials in slot order (RIG) or
// takes its slot's, lane 0 runs the 6 x 6 Cholesky step unrolled in registers and commits T, the lanes write the record.  Every loop is bounded by a count known when
// it is entered; no lane waits for another but at the block's barriers; no floating-point atomic anywhere.
#include "ht_calib_common.hpp"

#define CA_NSUM 29     // 21 of J J^T's upper triangle, 6 of J r, the truncated cost, the inliers
#define CA_PART 32     // doubles a slot's partial takes: the sums, then the slot's point count

// depth [B][h][w], cams [B][12] -> pts [B][stride] in camera space, npts [B]; T [N][8]: the guess widened (N = B per slot, else slot 0's alone).  stride holds every
// point a frame can give, so nothing is cut
__global__ __launch_bounds__(FV_THREADS) void k_calib_cloud(const uint16_t *__restrict__ depth, const float *__restrict__ cams, int w, int h, float lo, float hi, int fraction, int per_slot,
                                                            float4 *__restrict__ pts, int stride, int *__restrict__ npts, double *__restrict__ T)
{
	const int b = blockIdx.x, t = threadIdx.x;
	const int npx = w * h;
	const float *cam = cams + (size_t)b * HT_CAM;
	fv_view c;
	c.fx = cam[0]; c.fy = cam[1]; c.cx = cam[2]; c.cy = cam[3]; c.dscale = cam[4];
	c.pos = V3(0, 0, 0); c.q = V4(0, 0, 0, 1); c.plane = V4(0, 0, 0, FLT_MAX); c.posed = false; c.mirror = false; c.bad = false;
	int nd = 0, nm = 0;
	const int total = fv_emit<false>(c, depth + (size_t)b * npx, npx, w, lo, hi, 0.0f, fraction, 0, stride, 0, pts + (size_t)b * stride, nd, nm);
	if (t == 0) { const int n = (total + fraction - 1) / fraction; npts[b] = n < stride ? n : stride; }
	if (t < 7 && (per_slot || b == 0)) T[(size_t)b * 8 + t] = (double)cam[5 + t];
}

// poses: body k of slot b at poses + (b nb + k) pose_stride (7: poses; HT_STATE_STRIDE: the slots' state).  part [B][CA_PART]
__global__ __launch_bounds__(CA_THREADS) void k_calib_accum(const ht_model_dev M, const float *__restrict__ poses, int pose_stride, const float4 *__restrict__ pts, int stride, const int *__restrict__ npts,
                                                            const double *__restrict__ T, int per_slot, float cx, float cy, float cz, float max_dist, double *__restrict__ part)
{
	__shared__ __align__(16) float tab[HT_MAXNB * CA_BT];
	__shared__ double red[CA_THREADS / 64][CA_NSUM];
	const int t = threadIdx.x, b = blockIdx.x;
	const int nb = M.nb;
	ca_stage(M, poses, pose_stride, b, tab);
	const double *Tb = T + (size_t)(per_slot ? b : 0) * 8;
	const v3 tp = V3((float)Tb[0], (float)Tb[1], (float)Tb[2]);
	const v4 tq = V4((float)Tb[3], (float)Tb[4], (float)Tb[5], (float)Tb[6]);
	const v3 c = V3(cx, cy, cz);
	const double md2 = (double)max_dist * (double)max_dist;
	const int n = npts[b];
	const float4 *src = pts + (size_t)b * stride;
	double acc[CA_NSUM];
#pragma unroll
	for (int k = 0; k < CA_NSUM; k++) acc[k] = 0.0;
	__syncthreads();
	for (int i = t; i < n; i += CA_THREADS)
	{
		const float4 p = src[i];
		const v3 x = tp + qrot(tq, V3(p.x, p.y, p.z));
		const v4 pl = ca_closest(tab, nb, x);
		const float r = dot_plane(pl, x);
		const v3 nn = xyz(pl), m = cross(x - c, nn);
		const float J[6] = { nn.x, nn.y, nn.z, m.x, m.y, m.z };
		const bool in = fabsf(r) <= max_dist;
		int k = 0;
#pragma unroll
		for (int i0 = 0; i0 < 6; i0++)
#pragma unroll
			for (int j0 = i0; j0 < 6; j0++, k++) acc[k] += in ? (double)J[i0] * (double)J[j0] : 0.0;
#pragma unroll
		for (int i0 = 0; i0 < 6; i0++) acc[21 + i0] += in ? (double)J[i0] * (double)r : 0.0;
		const double r2 = (double)r * (double)r;
		acc[27] += r2 < md2 ? r2 : md2;
		acc[28] += in ? 1.0 : 0.0;
	}
	ca_reduce<CA_NSUM>(acc, red, part + (size_t)b * CA_PART, n);
}

struct ca_step { double damping, min_points, cx, cy, cz; };
// part [B][CA_PART] -> T [N][8] stepped (unless last), T_out [N][7], row [N][HT_CALIB_STATS] as words.  Block = transform
__global__ __launch_bounds__(64) void k_calib_solve(const double *__restrict__ part, int B, int per_slot, const ca_step o, int last, double *__restrict__ T, float *__restrict__ T_out, unsigned *__restrict__ row)
{
	__shared__ double S[CA_PART];
	const int t = threadIdx.x, s = blockIdx.x;
	if (t <= CA_NSUM)
	{
		double v = part[(size_t)(per_slot ? s : 0) * CA_PART + t];
		if (!per_slot) for (int b = 1; b < B; b++) v += part[(size_t)b * CA_PART + t];
		S[t] = v;
	}
	__syncthreads();
	unsigned *rec = row + (size_t)s * HT_CALIB_STATS * 2;
	if (t < 21) ca_store(rec + 2 * (6 + t), S[t]);
	if (t != 0) return;
	double *Ts = T + (size_t)s * 8;
	double ndt = 0.0, ndw = 0.0;
	int flag = S[28] < o.min_points ? HT_CALIB_FEW_INLIERS : 0;
	if (!last && !flag)
	{
		double L[6][6], g[6], d[6], n[7];
		{
			int k = 0;
#pragma unroll
			for (int i = 0; i < 6; i++)
#pragma unroll
				for (int j = i; j < 6; j++, k++) L[j][i] = S[k];      // the lower triangle, A_ji = A_ij
		}
		const double scale = 1.0 + o.damping;
#pragma unroll
		for (int i = 0; i < 6; i++) { L[i][i] = L[i][i] * scale; g[i] = -S[21 + i]; }
		bool ok = ca_cholesky<6>(L);
		ca_substitute<6>(L, g, d);
		ok = ca_candidate(Ts, d, o.cx, o.cy, o.cz, n) && ok;
#pragma unroll
		for (int i = 0; i < 6; i++) ok = ok && ca_finite(d[i]);
		if (ok)
		{
#pragma unroll
			for (int i = 0; i < 7; i++) Ts[i] = n[i];
			ndt = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); ndw = sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]);
		}
		else flag |= HT_CALIB_BAD_PIVOT;
	}
	float *out = T_out + (size_t)s * 7;
#pragma unroll
	for (int i = 0; i < 7; i++) out[i] = (float)Ts[i];
	ca_store(rec + 0, S[28]); ca_store(rec + 2, S[CA_NSUM]); ca_store(rec + 4, S[27]); ca_store(rec + 6, ndt); ca_store(rec + 8, ndw); ca_store(rec + 10, (double)flag);
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int ht_calib_default(ht_ctx *ctx, ht_calib *o)
{
	if (!ctx || !o) return HT_ERR_ARG;
	o->range_lo = 0.1f; o->range_hi = ctx->par.drangey; o->fraction = ctx->par.subsample_fraction > 0 ? ctx->par.subsample_fraction : 1;      // ht_views_default's
	o->mode = HT_CALIB_RIG; o->iterations = 10; o->max_dist = 0.03f; o->damping = 1e-3f; o->min_points = 12;
	o->centre[0] = o->centre[1] = o->centre[2] = 0.0f;
	return HT_OK;
}
// every refusal that needs no device, before anything grows or runs (a context that never came up answers them too)
int ht_calib_check(ht_ctx *ctx, const char *fn, int which, const void *poses, const void *depth, const void *cams, int w, int h, int B, const ht_calib *opt, const void *T_out, const void *stats, ca_call &c)
{
	const std::string f = fn;
	if (!depth || !cams || !ht_frame_dims_ok(w, h)) { ctx->err = f + ": frames [B][h][w] and cameras [B][12] are needed, w and h between 1 and 4096"; return HT_ERR_ARG; }
	if (!T_out || !stats) { ctx->err = f + ": T_out [N][7] and stats [iterations + 1][N][HT_CALIB_STATS] are needed"; return HT_ERR_ARG; }
	if (which < 0 || which > 1) { ctx->err = f + ": which is 0 (handmodel) or 1 (othermodel)"; return HT_ERR_ARG; }
	if (B < 1 || B > (poses ? CA_MAX_B : ctx->B)) { ctx->err = f + (poses ? ": a bad batch (between 1 and 65535 slots of poses)" : ": batch exceeds the capacity given to ht_create (the model is the slots' state)"); return HT_ERR_ARG; }
	ht_calib d; ht_calib_default(ctx, &d);
	if (opt) d = *opt;
	if (!(d.range_lo >= 0.0f) || !(d.range_hi > d.range_lo) || !isfinite(d.range_hi)) { ctx->err = f + ": a bad range (0 <= range_lo < range_hi, finite)"; return HT_ERR_ARG; }
	if (d.fraction < 1) { ctx->err = f + ": a bad fraction (>= 1)"; return HT_ERR_ARG; }
	if (d.mode != HT_CALIB_RIG && d.mode != HT_CALIB_PER_SLOT) { ctx->err = f + ": a bad mode (HT_CALIB_RIG or HT_CALIB_PER_SLOT)"; return HT_ERR_ARG; }
	if (d.iterations < 0 || d.iterations > CA_MAX_ITER) { ctx->err = f + ": bad iterations (between 0 and 64)"; return HT_ERR_ARG; }
	if (!(d.max_dist > 0.0f) || !isfinite(d.max_dist)) { ctx->err = f + ": a bad max_dist (> 0, finite, metres)"; return HT_ERR_ARG; }
	if (!(d.damping >= 0.0f) || !isfinite(d.damping)) { ctx->err = f + ": a bad damping (>= 0, finite)"; return HT_ERR_ARG; }
	if (d.min_points < 0) { ctx->err = f + ": a bad min_points (>= 0)"; return HT_ERR_ARG; }
	if (!isfinite(d.centre[0]) || !isfinite(d.centre[1]) || !isfinite(d.centre[2])) { ctx->err = f + ": a bad centre (finite)"; return HT_ERR_ARG; }
	const long long per = ((long long)w * h + d.fraction - 1) / d.fraction;
	if (per > HT_POINTS_LIMIT) { ctx->err = f + ": this view can carry " + std::to_string(per) + " points a slot, a cloud holds at most 76800 (ht_reserve_points): raise the fraction"; return HT_ERR_ARG; }
	c.o = d; c.bound = (int)per; c.N = d.mode == HT_CALIB_PER_SLOT ? B : 1;
	return HT_OK;
}
static const size_t CA_LDS_FIXED = sizeof(float) * HT_MAXNB * CA_BT + sizeof(double) * (CA_THREADS / 64) * CA_NSUM + 64;
// what needs the device but launches nothing: the context's state, the kernel's LDS, and the buffers grown to this call (one synchronising re-allocation, as
// ht_reserve_points: nothing of the context's can still be reading the outgrown ones).  lds_fixed: the static LDS of the caller's accumulate kernel
int ht_calib_reserve(ht_ctx *ctx, const char *fn, const ca_call &c, int B, size_t lds_fixed)
{
	if (!ctx->ready) { ctx->err = "context not initialised (ht_create failed)"; return HT_ERR_STATE; }
	if (ctx->cnn_only) { ctx->err = std::string(fn) + ": this context was created without a hand model (CNN only)"; return HT_ERR_STATE; }
	if ((size_t)ctx->model.plane_off[ctx->model.nb] * sizeof(float4) + lds_fixed > 80 * 1024) { ctx->err = std::string(fn) + ": the model's face planes do not fit the kernel's LDS"; return HT_ERR_STATE; }
	const size_t stride = ((size_t)c.bound + 63) & ~(size_t)63;
	if ((size_t)B <= ctx->calib_B && stride <= ctx->calib_stride) return HT_OK;
	ht_device_guard dev_guard_(ctx->device);
	HIPCHK(ctx, ht_sync_all(ctx));
	const size_t nB = (size_t)B > ctx->calib_B ? (size_t)B : ctx->calib_B, ns = stride > ctx->calib_stride ? stride : ctx->calib_stride;
	float4 *pts = nullptr; int *n = nullptr; double *part = nullptr, *T = nullptr;
	int r;
	if ((r = dev_alloc(ctx, &pts, nB * ns))) return r;      // (a failure keeps the old, valid buffers; what was newly taken stays on the context's list until ht_destroy)
	if ((r = dev_alloc(ctx, &n, nB)) || (r = dev_alloc(ctx, &part, nB * CA_PART)) || (r = dev_alloc(ctx, &T, nB * 8))) return r;
	drop_alloc(ctx, ctx->d_calib_pts); drop_alloc(ctx, ctx->d_calib_n); drop_alloc(ctx, ctx->d_calib_part); drop_alloc(ctx, ctx->d_calib_T);
	ctx->d_calib_pts = pts; ctx->d_calib_n = n; ctx->d_calib_part = part; ctx->d_calib_T = T; ctx->calib_B = nB; ctx->calib_stride = ns;
	return HT_OK;
}
void ht_calib_cloud(ht_ctx *ctx, const ca_call &c, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, int per_slot, hipStream_t s)
{
	ht_prof_scope ps(ctx, "k_calib_cloud", s);
	hipLaunchKernelGGL(k_calib_cloud, dim3((unsigned)B), dim3(FV_THREADS), 0, s, d_depth, d_cams, w, h, c.o.range_lo, c.o.range_hi, c.o.fraction, per_slot, ctx->d_calib_pts, (int)ctx->calib_stride, ctx->d_calib_n,
	                   ctx->d_calib_T);
}
// the launches, on s alone: the cloud, then iterations + 1 times the pair (accumulate, solve); the last pair evaluates the final state and steps nothing
static int calib_enqueue(ht_ctx *ctx, const ca_call &c, int which, const float *d_poses, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, float *d_T_out, double *d_stats, hipStream_t s)
{
	const ht_calib &o = c.o;
	const int per_slot = o.mode == HT_CALIB_PER_SLOT ? 1 : 0, stride = (int)ctx->calib_stride;
	const float *poses = d_poses ? d_poses : ctx->d_state[which];
	const int pose_stride = d_poses ? HT_POSE : HT_STATE_STRIDE;
	ht_calib_cloud(ctx, c, d_depth, d_cams, w, h, B, per_slot, s);
	const size_t dyn = (size_t)ctx->model.plane_off[ctx->model.nb] * sizeof(float4);
	static ht_lds_limit limit; limit.raise(dyn, k_calib_accum);
	const ca_step st = { (double)o.damping, (double)o.min_points, (double)o.centre[0], (double)o.centre[1], (double)o.centre[2] };
	for (int it = 0; it <= o.iterations; it++)
	{
		{
			ht_prof_scope ps(ctx, "k_calib_accum", s);
			hipLaunchKernelGGL(k_calib_accum, dim3((unsigned)B), dim3(CA_THREADS), dyn, s, ctx->model, poses, pose_stride, ctx->d_calib_pts, stride, ctx->d_calib_n, ctx->d_calib_T, per_slot, o.centre[0], o.centre[1],
			                   o.centre[2], o.max_dist, ctx->d_calib_part);
		}
		ht_prof_scope ps(ctx, "k_calib_solve", s);
		hipLaunchKernelGGL(k_calib_solve, dim3((unsigned)c.N), dim3(64), 0, s, ctx->d_calib_part, B, per_slot, st, it == o.iterations ? 1 : 0, ctx->d_calib_T, d_T_out,
		                   (unsigned *)d_stats + (size_t)it * c.N * HT_CALIB_STATS * 2);
	}
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_calibrate_view_dev(ht_ctx *ctx, int which, const float *d_poses, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, const ht_calib *o, float *d_T_out, double *d_stats, void *stream)
{
	if (!ctx) return HT_ERR_ARG;
	ca_call c;
	{ const int r = ht_calib_check(ctx, "ht_calibrate_view_dev", which, d_poses, d_depth, d_cams, w, h, B, o, d_T_out, d_stats, c); if (r) return r; }
	if (((uintptr_t)d_T_out | (uintptr_t)d_stats) & 3) { ctx->err = "ht_calibrate_view_dev: d_T_out and d_stats must be 4-byte aligned"; return HT_ERR_ARG; }
	{ const int r = ht_calib_reserve(ctx, "ht_calibrate_view_dev", c, B, CA_LDS_FIXED); if (r) return r; }
	ht_device_guard dev_guard_(ctx->device);
	return calib_enqueue(ctx, c, which, d_poses, d_depth, d_cams, w, h, B, d_T_out, d_stats, ht_user_stream(ctx, stream));
}
// the host form's staging plan (no device needed): inputs poses, depth, cams; outputs T_out, stats
int ht_calib_segments(const ca_call &c, int nb, const float *poses, const uint16_t *depth, const float *cams, int w, int h, int B, float *T_out, double *stats, ht_seg *seg)
{
	seg[0] = ht_seg{ (void *)poses, (size_t)B * nb * HT_POSE * sizeof(float), false, nullptr };
	seg[1] = ht_seg{ (void *)depth, (size_t)B * w * h * sizeof(uint16_t), false, nullptr };
	seg[2] = ht_seg{ (void *)cams, (size_t)B * HT_CAM * sizeof(float), false, nullptr };
	seg[3] = ht_seg{ T_out, (size_t)c.N * 7 * sizeof(float), true, nullptr };
	seg[4] = ht_seg{ stats, (size_t)(c.o.iterations + 1) * c.N * HT_CALIB_STATS * sizeof(double), true, nullptr };
	return 5;
}
extern "C" int ht_calibrate_view(ht_ctx *ctx, int which, const float *poses, const uint16_t *depth, const float *cams, int w, int h, int B, const ht_calib *o, float *T_out, double *stats)
{
	if (!ctx) return HT_ERR_ARG;
	ca_call c;
	{ const int r = ht_calib_check(ctx, "ht_calibrate_view", which, poses, depth, cams, w, h, B, o, T_out, stats, c); if (r) return r; }
	ht_seg seg[5];
	const int n = ht_calib_segments(c, ctx->model.nb, poses, depth, cams, w, h, B, T_out, stats, seg);
	{
		const ql_buf in[3] = { { seg[0].host, seg[0].bytes }, { seg[1].host, seg[1].bytes }, { seg[2].host, seg[2].bytes } }, out[2] = { { seg[3].host, seg[3].bytes }, { seg[4].host, seg[4].bytes } };
		if (ql_any_overlap(in, 3, out, 2)) { ctx->err = "ht_calibrate_view: an output overlaps an input or the other output"; return HT_ERR_ARG; }
	}
	{ const int r = ht_calib_reserve(ctx, "ht_calibrate_view", c, B, CA_LDS_FIXED); if (r) return r; }
	ht_device_guard dev_guard_(ctx->device);
	return ht_staged_call(ctx, seg, n, [&](hipStream_t s)
	                      { return calib_enqueue(ctx, c, which, (const float *)seg[0].dev, (const uint16_t *)seg[1].dev, (const float *)seg[2].dev, w, h, B, (float *)seg[3].dev, (double *)seg[4].dev, s); });
}
