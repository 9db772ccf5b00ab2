// ht_kpfit.hip -- fit the hand to keypoint targets on the device: the constraint rows of a keypoint table against 3-D points and pixels, written from the slots' current
// state, and the step loop that solves them with PhysModel::FitPointCloud's own launch sequence on one stream (an addition).
//
// Reference computations:
//   ConstrainPositionNailed            third_party/physics.h:342-346 (slowfit nails the dragged bone with it, include/handtrack.h:809-810)
//   ConstrainAlongDirectionDeadzone    third_party/physics.h:332-340 (slowfit and MultiStepSim pull feature points onto camera rays, handtrack.h:672-673, 804-806)
//   DCamera::deprojectz                include/misc_image.h:48 (a pixel's ray)
//   the momenta zeroed after a step    include/handtrack.h:686-687
// The semantics are include/ht_mi355x.h's "keypoint fit"; tests/kpfit_ref.py restates the rows and residuals in numpy and the kernel equals it bit for bit (fp32, one
// rounding per operation in the written order: the library is built without contraction, division and sqrtf are correctly rounded).
//
// Mapping.  k_keypoint_rows is launch- and latency-bound: one wave per frame, one lane per keypoint (K <= HT_KP_MAX = 64), four frames a block.  The table comes by value in
// the kernel arguments, the kinds as a bit mask.  A lane places its keypoint from its bone's state, builds its three (point) or four (pixel: a dead-zone pair on each of the
// two axes across the ray) rows in registers, and the wave compacts the absent ones out with a prefix sum over the lanes' row counts (__shfl_up), in table order.  A row is
// four 16-byte stores into the caller-row buffer k_solve takes as rows_pre.  The same lanes' residuals go to resid when asked for; lanes below nb zero their body's momenta
// (the first launch of a call) or write its user pose (the last).  No LDS, no barrier.
#include <string.h>
#include <math.h>
#include "ht_host.hpp"

#define KF_THREADS 256
#define KF_FRAMES (KF_THREADS / 64)

struct kf_opts { float max_force, ray_radius, ray_force; };

__device__ __forceinline__ void kf_row(float4 *out, int i, float body, v3 p0, v3 p1, v3 n, float dist, float fmin, float fmax)
{
	out[4 * i + 0] = make_float4(-1.0f, body, p0.x, p0.y);
	out[4 * i + 1] = make_float4(p0.z, p1.x, p1.y, p1.z);
	out[4 * i + 2] = make_float4(n.x, n.y, n.z, dist);
	out[4 * i + 3] = make_float4(0.0f, fmin, fmax, 0.0f);
}
// state [B][nb][HT_STATE_STRIDE] of the model being fitted; xyz [B][K][3], pix [B][K][2], weights [B][K] (may be null: 1), cams [B][12]; rows [B][stride][HT_ROW] with
// n_rows [B] (null: no rows are written), resid + f * resid_stride [K] (null: none), poses [B][nb][7] user poses (null: none)
__global__ __launch_bounds__(KF_THREADS) void k_keypoint_rows(const float *__restrict__ bodyc, int nb, const ql_table T, unsigned long long kinds, float *__restrict__ state, int B,
                                                              const float *__restrict__ xyz, const float *__restrict__ pix, const float *__restrict__ weights, const float *__restrict__ cams,
                                                              const kf_opts o, int zero_momenta, float *__restrict__ rows, int stride, int *__restrict__ n_rows,
                                                              float *__restrict__ resid, int resid_stride, float *__restrict__ poses)
{
	const int lane = threadIdx.x & 63, f = blockIdx.x * KF_FRAMES + (threadIdx.x >> 6), K = T.K;
	if (f >= B) return;      // the whole wave
	float *st = state + (size_t)f * nb * HT_STATE_STRIDE;
	if (lane < nb)
	{
		float *s = st + lane * HT_STATE_STRIDE;
		if (poses)      // GetPoseUser (physmodel.h:434, physics.h:142), as k_output writes it
		{
			const v3 pu = apply(XF(load3(s), load4(s + 3)), -load3(bodyc + lane * HT_BC + HT_BC_COM));
			float *p = poses + ((size_t)f * nb + lane) * HT_POSE;
			p[0] = pu.x; p[1] = pu.y; p[2] = pu.z; p[3] = s[3]; p[4] = s[4]; p[5] = s[5]; p[6] = s[6];
		}
		if (zero_momenta) for (int k = 7; k < 13; k++) s[k] = 0.0f;      // no lane reads them
	}
	const bool live = lane < K, ray = live && ((kinds >> lane) & 1ull);
	bool present = false;
	float body = 0.0f, w = 1.0f, d0 = 0.0f, d1 = 0.0f;
	v3 off = V3(0, 0, 0), p0 = V3(0, 0, 0), dv = V3(0, 0, 0), ax = V3(0, 0, 0), ay = V3(0, 0, 0);
	if (live)
	{
		const int b = T.bone[lane];
		const size_t at = (size_t)f * K + lane;
		body = (float)b;
		off = load3(T.off + 3 * lane);
		if (!T.rel[lane]) off = off - load3(bodyc + b * HT_BC + HT_BC_COM);      // the states are centre-of-mass poses
		const float *p = st + b * HT_STATE_STRIDE;
		const v3 X = load3(p) + qrot(load4(p + 3), off);
		if (weights) w = weights[at];
		present = w > 0.0f;
		if (!ray)
		{
			p0 = load3(xyz + at * 3);
			present = present && isfinite(p0.x) && isfinite(p0.y) && isfinite(p0.z);
			dv = X - p0;
		}
		else
		{
			const float u = pix[at * 2], v = pix[at * 2 + 1];
			const float *cam = cams + (size_t)f * HT_CAM;
			present = present && isfinite(u) && isfinite(v);
			const v3 r = normalize(qrot(load4(cam + 8), V3((u - cam[2]) / cam[0], (v - cam[3]) / cam[1], 1.0f)));
			const v4 q = quat_from_to(V3(0, 0, 1), r);
			p0 = load3(cam + 5);
			ax = qxdir(q); ay = qydir(q);
			const v3 rel = X - p0;
			d0 = dot(rel, ax); d1 = dot(rel, ay);
		}
	}
	if (resid && live) resid[(size_t)f * resid_stride + lane] = !present ? -1.0f : ray ? sqrtf(d0 * d0 + d1 * d1) : sqrtf((dv.x * dv.x + dv.y * dv.y) + dv.z * dv.z);
	if (!rows) return;
	const int c = present ? (ray ? 4 : 3) : 0;
	int incl = c;
	for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
	const int first = incl - c, total = __shfl(incl, 63, 64);
	if (lane == 0) n_rows[f] = total;
	if (!c || first + c > stride) return;      // (the host has sized the stride for every keypoint of the table)
	float4 *out = reinterpret_cast<float4 *>(rows + ((size_t)f * stride + first) * HT_ROW);
	if (!ray)
	{
		const float fl = o.max_force * w;
		kf_row(out, 0, body, p0, off, V3(1, 0, 0), dv.x, -fl, fl);
		kf_row(out, 1, body, p0, off, V3(0, 1, 0), dv.y, -fl, fl);
		kf_row(out, 2, body, p0, off, V3(0, 0, 1), dv.z, -fl, fl);
	}
	else
	{
		const float fr = o.ray_force * w;
		kf_row(out, 0, body, p0, off, ax, d0 + o.ray_radius, 0.0f, fr);
		kf_row(out, 1, body, p0, off, ax, d0 - o.ray_radius, -fr, 0.0f);
		kf_row(out, 2, body, p0, off, ay, d1 + o.ray_radius, 0.0f, fr);
		kf_row(out, 3, body, p0, off, ay, d1 - o.ray_radius, -fr, 0.0f);
	}
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
struct kf_call { ql_table t; unsigned long long kinds; int rows; kf_opts o; int steps, keep_momenta; bool points, rays; };

extern "C" int ht_kpfit_default(ht_kpfit *o)
{
	if (!o) return HT_ERR_ARG;
	o->steps = 6; o->max_force = FLT_MAX; o->ray_radius = 0.01f; o->ray_force = 100000.0f; o->flags = 0;      // slowfit's figures (handtrack.h:786, 805; physics.h:284)
	return HT_OK;
}
// every refusal that needs no look at the host arrays' values, before anything grows or runs
static int kf_check(ht_ctx *ctx, int which_model, int B, int which, int K, const int *bones, const float *offsets, const int *rel, const int *kind, const void *xyz, const void *pix, const void *cams,
                    const ht_kpfit *opt, kf_call &c)
{
	CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (which_model < 0 || which_model > 1) { ctx->err = "ht_fit_keypoints: which_model is 0 (handmodel) or 1 (othermodel)"; return HT_ERR_ARG; }
	REFUSE_EXACT_SOLVER(ctx);
	{ const int r = ql_table_of(ctx, "ht_fit_keypoints", which, K, bones, offsets, rel, c.t); if (r) return r; }
	c.kinds = 0ull; c.rows = 0; c.points = c.rays = false;
	for (int k = 0; k < c.t.K; k++)
	{
		const int kd = kind ? kind[k] : 0;
		if (kd != 0 && kd != 1) { ctx->err = "ht_fit_keypoints: kind is 0 (a 3-D point) or 1 (a pixel)"; return HT_ERR_ARG; }
		if (kd) { c.kinds |= 1ull << k; c.rays = true; c.rows += 4; } else { c.points = true; c.rows += 3; }
	}
	if (c.rows > 5 * ctx->model.nb + 128) { ctx->err = "ht_fit_keypoints: the table's rows (3 a point, 4 a pixel) exceed the 5 * bodies + 128 caller rows a frame's scratch slot holds"; return HT_ERR_ARG; }
	if ((c.points && !xyz) || (c.rays && (!pix || !cams))) { ctx->err = "ht_fit_keypoints: point targets need xyz, pixel targets need pix and cams"; return HT_ERR_ARG; }
	ht_kpfit d; ht_kpfit_default(&d);
	if (opt) d = *opt;
	if (d.steps < 1 || d.steps > 64) { ctx->err = "ht_fit_keypoints: steps between 1 and 64"; return HT_ERR_ARG; }
	if (d.flags & ~HT_KPFIT_KEEP_MOMENTA) { ctx->err = "ht_fit_keypoints: unknown flags"; return HT_ERR_ARG; }
	if (isinf(d.max_force) && d.max_force > 0.0f) d.max_force = FLT_MAX;
	if (!(d.max_force > 0.0f) || !isfinite(d.max_force) || !(d.ray_radius >= 0.0f) || !isfinite(d.ray_radius) || !(d.ray_force > 0.0f) || !isfinite(d.ray_force))
	{ ctx->err = "ht_fit_keypoints: max_force > 0 (INFINITY: FLT_MAX), ray_radius >= 0 and ray_force > 0, all finite"; return HT_ERR_ARG; }
	c.o.max_force = d.max_force; c.o.ray_radius = d.ray_radius; c.o.ray_force = d.ray_force; c.steps = d.steps; c.keep_momenta = (d.flags & HT_KPFIT_KEEP_MOMENTA) ? 1 : 0;
	return HT_OK;
}
static void kf_launch(ht_ctx *ctx, const kf_call &c, int which_model, int B, const float *d_xyz, const float *d_pix, const float *d_w, const float *d_cams, int zero_momenta, bool rows, float *d_resid,
                      float *d_poses, hipStream_t s)
{
	ht_prof_scope ps(ctx, "k_keypoint_rows", s);
	hipLaunchKernelGGL(k_keypoint_rows, dim3((unsigned)((B + KF_FRAMES - 1) / KF_FRAMES)), dim3(KF_THREADS), 0, s, ctx->model.bodyc, ctx->model.nb, c.t, c.kinds, ctx->d_state[which_model], B, d_xyz, d_pix, d_w,
	                   d_cams, c.o, zero_momenta, rows ? ctx->d_user_lin : nullptr, ctx->user_lin_cap, ctx->d_user_n, d_resid, 2 * c.t.K, d_poses);
}
// The steps, on s alone: nothing is copied or waited for between them.  The row buffers have been reserved (ht_user_rows_reserve)
static int kf_enqueue(ht_ctx *ctx, const kf_call &c, int which_model, int B, const float *d_xyz, const float *d_pix, const float *d_w, const float *d_cams, float *d_poses, float *d_resid, hipStream_t s)
{
	HIPCHK(ctx, hipMemsetAsync(ctx->d_npts, 0, (size_t)B * sizeof(int), s));                               // no points: the cloud-row launch of a step leaves no rows
	HIPCHK(ctx, hipMemsetAsync(ctx->d_user_n + 3 * (size_t)ctx->B, 0, (size_t)B * sizeof(int), s));      // no angular rows of the caller's
	for (int st = 0; st < c.steps; st++)
	{
		kf_launch(ctx, c, which_model, B, d_xyz, d_pix, d_w, d_cams, !c.keep_momenta && st == 0, true, st == 0 ? d_resid : nullptr, nullptr, s);
		ht_fit_rows_enqueue(ctx, which_model, B, ctx->par.microforce, 0, c.keep_momenta ? 0 : 1, s);
	}
	if (d_resid || d_poses) kf_launch(ctx, c, which_model, B, d_xyz, d_pix, d_w, d_cams, 0, false, d_resid ? d_resid + c.t.K : nullptr, d_poses, s);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_fit_keypoints_dev(ht_ctx *ctx, int which_model, int B, int which, int K, const int *bones, const float *offsets, const int *rel, const int *kind, const float *d_xyz, const float *d_pix,
                                    const float *d_weights, const float *d_cams, const ht_kpfit *o, float *d_poses, float *d_resid, void *stream)
{
	CHECK_READY(ctx);
	kf_call c;
	{ const int r = kf_check(ctx, which_model, B, which, K, bones, offsets, rel, kind, d_xyz, d_pix, d_cams, o, c); if (r) return r; }
	{ const int r = ht_user_rows_reserve(ctx, c.rows, 1); if (r) return r; }
	return kf_enqueue(ctx, c, which_model, B, d_xyz, d_pix, d_weights, d_cams, d_poses, d_resid, ht_user_stream(ctx, stream));
}
extern "C" int ht_fit_keypoints(ht_ctx *ctx, int which_model, int B, int which, int K, const int *bones, const float *offsets, const int *rel, const int *kind, const float *xyz, const float *pix,
                                const float *weights, const float *cams, const ht_kpfit *o, float *poses, float *resid)
{
	CHECK_READY(ctx);
	kf_call c;
	{ const int r = kf_check(ctx, which_model, B, which, K, bones, offsets, rel, kind, xyz, pix, cams, o, c); if (r) return r; }
	const size_t n = (size_t)B, nk = n * c.t.K;
	if (weights) for (size_t i = 0; i < nk; i++) if (!(weights[i] >= 0.0f && weights[i] <= 1.0f)) { ctx->err = "ht_fit_keypoints: weights between 0 and 1"; return HT_ERR_ARG; }
	const ql_buf in[4] = { { c.points ? xyz : nullptr, nk * 3 * sizeof(float) }, { c.rays ? pix : nullptr, nk * 2 * sizeof(float) }, { weights, nk * sizeof(float) }, { c.rays ? cams : nullptr, n * HT_CAM * sizeof(float) } };
	const ql_buf out[2] = { { poses, n * ctx->model.nb * HT_POSE * sizeof(float) }, { resid, nk * 2 * sizeof(float) } };
	if (ql_any_overlap(in, 4, out, 2)) { ctx->err = "ht_fit_keypoints: an output overlaps an input or another output"; return HT_ERR_ARG; }
	{ const int r = ht_user_rows_reserve(ctx, c.rows, 1); if (r) return r; }
	ht_seg seg[6] = { { (void *)in[0].p, in[0].bytes, false }, { (void *)in[1].p, in[1].bytes, false }, { (void *)weights, in[2].bytes, false }, { (void *)in[3].p, in[3].bytes, false },
	                  { poses, out[0].bytes, true }, { resid, out[1].bytes, true } };
	return ht_staged_call(ctx, seg, 6, [&](hipStream_t s)
	                      { return kf_enqueue(ctx, c, which_model, B, (const float *)seg[0].dev, (const float *)seg[1].dev, (const float *)seg[2].dev, (const float *)seg[3].dev, (float *)seg[4].dev, (float *)seg[5].dev, s); });
}
