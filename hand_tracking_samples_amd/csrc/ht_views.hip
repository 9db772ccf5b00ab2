// ht_views.hip -- one hand from several depth views: the clouds of up to HT_VIEWS_MAX frames of a slot (cameras posed in one tracking space, an optional mirror plane a
// view) fused into the slot's prepared points, every point with the index of the ray source that saw it, and the fit that reads those sources (an addition).
//
// Reference computations:
//   PointCloud / FallsWithinRange / deprojectz   include/misc_image.h:409-417, :24, :48
//   PlaneSplit, Mirror, MirrorPlaneSplit         include/misc_image.h:462-485 ("mirrors to get some view of the back of an object", :404-406)
//   the mirror plane of a data set               include/dataset.h:24,45 (mplane, default (0,0,0,FLT_MAX) = none)
//   takesubsample (every fraction-th point)      include/physmodel.h:58-64, 120-126
//   CloudConstraint's ray origin                 include/physmodel.h:164-174 (k_view_rows, ht_cloud.hip)
// The semantics are include/ht_mi355x.h's "several views"; tests/views_ref.py restates them in numpy and the kernel equals it bit for bit (fp32, one rounding per
// operation in the written order: the library is built without contraction).
//
// Mapping.  k_fuse_views takes k_prepare's compaction (counts, a block-wide exclusive prefix, ordered emission) as its model, one block per (slot, view), but walks a
// frame once and with neighbouring lanes on neighbouring pixels: the frame goes by in tiles of 1024 pixels, thread t owns the four pixels [4 t, 4 t + 4) of the tile (a
// wave's loads fall into four cache lines instead of one line a lane), the block forms the prefix of the tile's kept pixels on top of the running count of the tiles
// before, and every thread emits its own in place: the order is the raster order whatever the arrival.  A view's first output index is the sum of the counts of the
// views before it; its block counts those views' pixels itself in a strided walk (a count needs no order), which keeps the launch free of any wait between blocks.
// A kept pixel is classified against the view's mirror plane before it is ranked, so direct and mirrored points interleave as they come; the coordinates, the plane
// distance and the pose are worked out for in-range pixels only, which are few.
#include <limits.h>
#include <string.h>
#include <math.h>
#include "ht_host.hpp"
#include "ht_prepare.hpp"

struct fv_opts { float lo, hi, eps; int fraction; };      // (fv_view, fv_side, fv_emit: ht_prepare.hpp, shared with k_calib_cloud)
__device__ __forceinline__ fv_view fv_load(const float *__restrict__ cam, const float *__restrict__ plane)
{
	fv_view c;
	c.fx = cam[0]; c.fy = cam[1]; c.cx = cam[2]; c.cy = cam[3]; c.dscale = cam[4];
	c.pos = load3(cam + 5); c.q = load4(cam + 8);
	c.posed = !(is_zero(c.pos) && c.q.x == 0.0f && c.q.y == 0.0f && c.q.z == 0.0f && c.q.w == 1.0f);
	c.plane = plane ? load4(plane) : V4(0, 0, 0, FLT_MAX);
	const bool none = is_zero(xyz(c.plane)) && c.plane.w == FLT_MAX;      // dataset.h:45
	c.bad = !none && (!(isfinite(c.plane.x) && isfinite(c.plane.y) && isfinite(c.plane.z) && isfinite(c.plane.w)) || is_zero(xyz(c.plane)));
	c.mirror = !none && !c.bad;
	return c;
}
// this thread's share of the pixels a view keeps, lanes on neighbouring pixels (the order does not matter to a count).  lo > hi: no pixel is in range (a bad plane)
template <bool MIRROR> __device__ __forceinline__ int fv_count(const fv_view &c, const uint16_t *__restrict__ src, int npx, int w, float lo, float hi, float eps)
{
	int cnt = 0;
	float4 p; float pd;
	for (int i = threadIdx.x; i < npx; i += FV_THREADS)
	{
		const float d = depth_metres(src[i], c.dscale);
		if (!MIRROR) cnt += depth_in_range(d, lo, hi) ? 1 : 0;
		else if (depth_in_range(d, lo, hi)) cnt += fv_side<true>(c, eps, i, w, d, p, pd) != 0 ? 1 : 0;
	}
	return cnt;
}
// the source origins of a view in tracking space: the camera's position, and its image in the mirror (the camera-space origin mirrored: n * (plane.w * -2), Mirror
// misc_image.h:477 on (0,0,0)); a view without a plane has the camera's position in both places
__device__ __forceinline__ void fv_origins(const fv_view &c, v3 &direct, v3 &mirrored)
{
	direct = c.pos;
	mirrored = c.pos;
	if (c.mirror) { const v3 m = xyz(c.plane) * (c.plane.w * -2.0f); mirrored = c.posed ? c.pos + qrot(c.q, m) : m; }
}

// depth [B][V][h][w], cams [B][V][12], planes [B][V][4] or null -> pts [B][stride] (written below `cap`), npts [B], per_source [B][2V], origins [B][2V][3] (may be null),
// table [B][2 HT_VIEWS_MAX][3] (the context's copy of the origins, read by k_view_rows), *cut += slots whose cloud did not fit `cap`.  Grid (B, V)
__global__ __launch_bounds__(FV_THREADS) void k_fuse_views(const uint16_t *__restrict__ depth, const float *__restrict__ cams, const float *__restrict__ planes, int w, int h, int V, const fv_opts o,
                                                           float4 *__restrict__ pts, int stride, int cap, int *__restrict__ npts, int *__restrict__ per_source, float *__restrict__ origins,
                                                           float *__restrict__ table, int *__restrict__ cut)
{
	const int b = blockIdx.x, v = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int npx = w * h;
	__shared__ int nsrc[2];
	if (t < 2) nsrc[t] = 0;
	// the views before this one: how many points each emits
	int base = 0;
	for (int u = 0; u < v; u++)
	{
		const size_t at = (size_t)b * V + u;
		const fv_view c = fv_load(cams + at * HT_CAM, planes ? planes + at * 4 : nullptr);
		const float lo = c.bad ? 1.0f : o.lo, hi = c.bad ? 0.0f : o.hi;
		const int cnt = c.mirror ? fv_count<true>(c, depth + at * npx, npx, w, lo, hi, o.eps) : fv_count<false>(c, depth + at * npx, npx, w, lo, hi, o.eps);
		int total;
		block_prefix256(cnt, lane, wave, total);
		base += (total + o.fraction - 1) / o.fraction;
		__syncthreads();      // the prefix's wave sums are free for the next view
	}
	const size_t at = (size_t)b * V + v;
	const fv_view c = fv_load(cams + at * HT_CAM, planes ? planes + at * 4 : nullptr);
	const float lo = c.bad ? 1.0f : o.lo, hi = c.bad ? 0.0f : o.hi;
	int nd = 0, nm = 0;
	const int total = c.mirror ? fv_emit<true>(c, depth + at * npx, npx, w, lo, hi, o.eps, o.fraction, base, cap, v, pts + (size_t)b * stride, nd, nm)
	                           : fv_emit<false>(c, depth + at * npx, npx, w, lo, hi, o.eps, o.fraction, base, cap, v, pts + (size_t)b * stride, nd, nm);
	if (nd) atomicAdd(&nsrc[0], nd);
	if (nm) atomicAdd(&nsrc[1], nm);
	__syncthreads();
	if (t < 2)
	{
		v3 od, om;
		fv_origins(c, od, om);
		const v3 og = t ? om : od;
		const size_t s = (size_t)b * 2 * V + 2 * v + t, ts = (size_t)b * 2 * HT_VIEWS_MAX + 2 * v + t;
		per_source[s] = nsrc[t];
		if (origins) { origins[3 * s] = og.x; origins[3 * s + 1] = og.y; origins[3 * s + 2] = og.z; }
		table[3 * ts] = og.x; table[3 * ts + 1] = og.y; table[3 * ts + 2] = og.z;
	}
	if (t == 0 && v == V - 1)
	{
		const int n = base + (total + o.fraction - 1) / o.fraction;
		npts[b] = n < cap ? n : cap;
		if (n > cap) atomicAdd(cut, 1);
	}
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int ht_views_default(ht_ctx *ctx, ht_views *o)
{
	if (!ctx || !o) return HT_ERR_ARG;
	o->range_lo = 0.1f; o->range_hi = ctx->par.drangey; o->fraction = ctx->par.subsample_fraction > 0 ? ctx->par.subsample_fraction : 1; o->mirror_eps = 0.02f;      // handtrack.h:703, PlaneSplit's default misc_image.h:462
	return HT_OK;
}
struct fv_call { fv_opts o; int bound; };      // bound: the most points a slot's fused cloud can have
// every refusal that needs no device, before anything grows or runs (a context that never came up answers them too)
static int fv_check(ht_ctx *ctx, const char *fn, const void *depth, const void *cams, int w, int h, int V, int B, const ht_views *opt, fv_call &c)
{
	const std::string f = fn;
	if (V < 1 || V > HT_VIEWS_MAX) { ctx->err = f + ": between 1 and HT_VIEWS_MAX = 4 views"; return HT_ERR_ARG; }
	if (!depth || !cams || !ht_frame_dims_ok(w, h)) { ctx->err = f + ": frames [B][V][h][w] and cameras [B][V][12] are needed, w and h between 1 and 4096"; return HT_ERR_ARG; }
	ht_views d; ht_views_default(ctx, &d);
	if (opt) d = *opt;
	if (!(d.range_lo >= 0.0f) || !(d.range_hi > d.range_lo) || !isfinite(d.range_hi)) { ctx->err = f + ": a bad range (0 <= range_lo < range_hi, finite)"; return HT_ERR_ARG; }
	if (d.fraction < 1) { ctx->err = f + ": a bad fraction (>= 1)"; return HT_ERR_ARG; }
	if (!(d.mirror_eps >= 0.0f) || !isfinite(d.mirror_eps)) { ctx->err = f + ": a bad mirror_eps (>= 0, finite)"; return HT_ERR_ARG; }
	CHECK_BATCH(ctx, B);
	c.o.lo = d.range_lo; c.o.hi = d.range_hi; c.o.eps = d.mirror_eps; c.o.fraction = d.fraction;
	const long long per = ((long long)w * h + d.fraction - 1) / d.fraction, all = per * V;
	c.bound = all > INT_MAX ? INT_MAX : (int)all;
	return HT_OK;
}
static int fv_buffers(ht_ctx *ctx)      // the context's table of origins, its per-source counts and its count of cut slots, once
{
	if (ctx->d_view_origins) return HT_OK;
	int r;
	if ((r = dev_alloc(ctx, &ctx->d_view_src, (size_t)ctx->B * 2 * HT_VIEWS_MAX + 1))) return r;
	if ((r = dev_alloc(ctx, &ctx->d_view_origins, (size_t)ctx->B * 2 * HT_VIEWS_MAX * 3))) return r;
	HIPCHK(ctx, hipMemset(ctx->d_view_origins, 0, (size_t)ctx->B * 2 * HT_VIEWS_MAX * 3 * sizeof(float)));
	return HT_OK;
}
// the launch, on s alone; cap: where a slot's cloud is cut (<= the context's point capacity, which has been reserved)
static int fv_enqueue(ht_ctx *ctx, const fv_call &c, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, int B, int cap, int *d_npoints, int *d_per_source,
                      float *d_origins, int *d_cut, hipStream_t s)
{
	int *cut = d_cut ? d_cut : ctx->d_view_src + (size_t)ctx->B * 2 * HT_VIEWS_MAX;
	HIPCHK(ctx, hipMemsetAsync(cut, 0, sizeof(int), s));
	{
		ht_prof_scope ps(ctx, "k_fuse_views", s);
		hipLaunchKernelGGL(k_fuse_views, dim3((unsigned)B, (unsigned)V), dim3(FV_THREADS), 0, s, d_depth, d_cams, d_planes, w, h, V, c.o, ctx->d_pts, ctx->model.pts_cap, cap, ctx->d_npts,
		                   d_per_source ? d_per_source : ctx->d_view_src, d_origins, ctx->d_view_origins, cut);
	}
	if (d_npoints) HIPCHK(ctx, hipMemcpyAsync(d_npoints, ctx->d_npts, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
	ctx->model.pts_bound = 0;      // no assumption about the cloud size, as after a stage call
	ctx->views_B = B;
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
// check + reserve (everything that can refuse or wait), then the launch: the update calls reserve before their first launch and enqueue behind the update
int ht_fuse_views_enqueue(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, int B, const ht_views *o, int *d_npoints, int *d_per_source,
                          float *d_origins, int *d_cut, hipStream_t s)
{
	fv_call c;
	{ const int r = fv_check(ctx, "ht_fuse_views_dev", d_depth, d_cams, w, h, V, B, o, c); if (r) return r; }
	return fv_enqueue(ctx, c, d_depth, d_cams, d_planes, w, h, V, B, c.bound, d_npoints, d_per_source, d_origins, d_cut, s);
}
int ht_fuse_views_reserve(ht_ctx *ctx, const char *fn, const void *depth, const void *cams, int w, int h, int V, int B, const ht_views *o)
{
	fv_call c;
	{ const int r = fv_check(ctx, fn, depth, cams, w, h, V, B, o, c); if (r) return r; }
	if (c.bound > HT_POINTS_LIMIT) { ctx->err = std::string(fn) + ": these views can carry " + std::to_string(c.bound) + " points a slot, the per-point arrays hold at most 76800 (ht_reserve_points): raise the fraction"; return HT_ERR_ARG; }
	if (!ctx->ready) { ctx->err = "context not initialised (ht_create failed)"; return HT_ERR_STATE; }
	CHECK_MODEL(ctx);
	ht_device_guard dev_guard_(ctx->device);
	int r;
	if ((r = fv_buffers(ctx)) || (r = ht_reserve_points_locked(ctx, c.bound < HT_MAXPTS ? HT_MAXPTS : c.bound))) return r;
	return HT_OK;
}
extern "C" int ht_fuse_views_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, int B, const ht_views *o, int *d_npoints, int *d_per_source,
                                 float *d_origins, int *d_cut, void *stream)
{
	if (!ctx) return HT_ERR_ARG;
	{ const int r = ht_fuse_views_reserve(ctx, "ht_fuse_views_dev", d_depth, d_cams, w, h, V, B, o); if (r) return r; }
	ht_device_guard dev_guard_(ctx->device);
	return ht_fuse_views_enqueue(ctx, d_depth, d_cams, d_planes, w, h, V, B, o, d_npoints, d_per_source, d_origins, d_cut, ht_user_stream(ctx, stream));
}
// a mirror plane of the host form: "none", or finite with a normal that is not zero
int ht_views_planes_ok(ht_ctx *ctx, const char *fn, const float *planes, size_t n)
{
	for (size_t i = 0; planes && i < n; i++)
	{
		const float *p = planes + 4 * i;
		if (p[0] == 0.0f && p[1] == 0.0f && p[2] == 0.0f && p[3] == FLT_MAX) continue;
		if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3])) || (p[0] == 0.0f && p[1] == 0.0f && p[2] == 0.0f))
		{ ctx->err = std::string(fn) + ": a mirror plane with a non-finite or zero normal that is not the \"none\" plane (0,0,0,FLT_MAX)"; return HT_ERR_ARG; }
	}
	return HT_OK;
}
extern "C" int ht_fuse_views(ht_ctx *ctx, const uint16_t *depth, const float *cams, const float *planes, int w, int h, int V, int B, const ht_views *o, float *points, int cap, int *npoints,
                             int *per_source, float *origins, int *cut)
{
	if (!ctx) return HT_ERR_ARG;
	fv_call c;
	{ const int r = fv_check(ctx, "ht_fuse_views", depth, cams, w, h, V, B, o, c); if (r) return r; }
	if (cap < 1 || (points && !npoints)) { ctx->err = "ht_fuse_views: cap >= 1, and npoints with points"; return HT_ERR_ARG; }
	const size_t n = (size_t)B, nv = n * V;
	{ const int r = ht_views_planes_ok(ctx, "ht_fuse_views", planes, nv); if (r) return r; }
	const ql_buf in[3] = { { depth, nv * w * h * sizeof(uint16_t) }, { cams, nv * HT_CAM * sizeof(float) }, { planes, nv * 4 * sizeof(float) } };
	const ql_buf out[5] = { { points, n * cap * 4 * sizeof(float) }, { npoints, n * sizeof(int) }, { per_source, nv * 2 * sizeof(int) }, { origins, nv * 6 * sizeof(float) }, { cut, sizeof(int) } };
	if (ql_any_overlap(in, 3, out, 5)) { ctx->err = "ht_fuse_views: an output overlaps an input or another output"; return HT_ERR_ARG; }
	const int need = c.bound < cap ? c.bound : cap;      // the cloud is cut at the caller's capacity
	if (need > HT_POINTS_LIMIT) { ctx->err = "ht_fuse_views: these views can carry more than the 76800 points a slot holds (ht_reserve_points) and cap admits them: raise the fraction or lower cap"; return HT_ERR_ARG; }
	CHECK_READY(ctx); CHECK_MODEL(ctx);
	{ int r; if ((r = fv_buffers(ctx)) || (r = ht_reserve_points_locked(ctx, need < HT_MAXPTS ? HT_MAXPTS : need))) return r; }
	ht_seg seg[7] = { { (void *)depth, in[0].bytes, false }, { (void *)cams, in[1].bytes, false }, { (void *)planes, in[2].bytes, false },
	                  { npoints, out[1].bytes, true }, { per_source, out[2].bytes, true }, { origins, out[3].bytes, true }, { cut, out[4].bytes, true } };
	const int r = ht_staged_call(ctx, seg, 7, [&](hipStream_t s)
	                             { return fv_enqueue(ctx, c, (const uint16_t *)seg[0].dev, (const float *)seg[1].dev, (const float *)seg[2].dev, w, h, V, B, need, (int *)seg[3].dev, (int *)seg[4].dev, (float *)seg[5].dev, (int *)seg[6].dev, s); });
	if (r) return r;
	if (points)      // the slots' clouds as they lie on the device, xyz and the source beside them
	{
		const size_t row = (size_t)need * sizeof(float4);
		HIPCHK(ctx, hipMemcpy2D(points, (size_t)cap * sizeof(float4), ctx->d_pts, (size_t)ctx->model.pts_cap * sizeof(float4), row, B, hipMemcpyDeviceToHost));
	}
	return HT_OK;
}

// ---- the rows and the fit ----------------------------------------------------------------------------------------------------------------------------------------
static int fit_views_check(ht_ctx *ctx, const char *fn, int which, int B, int passes)
{
	const std::string f = fn;
	if (which < 0 || which > 1) { ctx->err = f + ": which is 0 (handmodel) or 1 (othermodel)"; return HT_ERR_ARG; }
	if (passes < 1 || passes > 64) { ctx->err = f + ": passes between 1 and 64"; return HT_ERR_ARG; }
	CHECK_BATCH(ctx, B);
	if (!ctx->ready) { ctx->err = "context not initialised (ht_create failed)"; return HT_ERR_STATE; }
	CHECK_MODEL(ctx);
	REFUSE_EXACT_SOLVER(ctx);
	if (B > ctx->views_B) { ctx->err = f + ": slots [0,B) hold no fused cloud (ht_fuse_views first)"; return HT_ERR_STATE; }
	return HT_OK;
}
extern "C" int ht_stage_view_rows(ht_ctx *ctx, int which, int B, float *rows, int cap, int *nrows)
{
	if (!ctx) return HT_ERR_ARG;
	if (!rows || !nrows || cap < 1) { ctx->err = "ht_stage_view_rows: rows [B][cap][16] and nrows [B] are needed"; return HT_ERR_ARG; }
	{ const int r = fit_views_check(ctx, "ht_stage_view_rows", which, B, 1); if (r) return r; }
	ht_device_guard dev_guard_(ctx->device);
	hipStream_t s = ctx->stream;
	const int n = cap < ctx->model.pts_cap ? cap : ctx->model.pts_cap;
	HIPCHK(ctx, hipMemsetAsync(ctx->d_rows, 0, (size_t)B * ctx->model.pts_cap * HT_ROW * sizeof(float), s));
	ht_launch_cloud_rows_views(ctx->model, ctx->d_state[which], ctx->d_pts, ctx->d_npts, ctx->d_view_origins, ht_cloud_limits(ctx->par, CLOUD_FIT), ctx->d_rows, ctx->d_nrows, B, s);
	HIPCHK(ctx, hipMemcpy2DAsync(rows, (size_t)cap * HT_ROW * sizeof(float), ctx->d_rows, (size_t)ctx->model.pts_cap * HT_ROW * sizeof(float), (size_t)n * HT_ROW * sizeof(float), B, hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipMemcpyAsync(nrows, ctx->d_nrows, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
	return ht_sync_check(ctx, s);
}
extern "C" int ht_fit_views_dev(ht_ctx *ctx, int which, int B, int passes, float *d_poses, void *stream)
{
	if (!ctx) return HT_ERR_ARG;
	{ const int r = fit_views_check(ctx, "ht_fit_views_dev", which, B, passes); if (r) return r; }
	ht_device_guard dev_guard_(ctx->device);
	return ht_fit_views_enqueue(ctx, which, B, passes, d_poses, ht_user_stream(ctx, stream));
}
extern "C" int ht_fit_views(ht_ctx *ctx, int which, int B, int passes, float *poses)
{
	if (!ctx) return HT_ERR_ARG;
	{ const int r = fit_views_check(ctx, "ht_fit_views", which, B, passes); if (r) return r; }
	ht_device_guard dev_guard_(ctx->device);
	ht_seg seg[1] = { { poses, (size_t)B * ctx->model.nb * HT_POSE * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 1, [&](hipStream_t s) { return ht_fit_views_enqueue(ctx, which, B, passes, (float *)seg[0].dev, s); });
}

// ---- timing only (tools/bench_views.py): the yardsticks the calls above are measured beside, on device buffers, enqueued on `stream` and not waited for ---------------
// k_prepare_frame alone on B frames [B][h][w] with the tracker's range and fraction, into the slots' prepared points (what an update's input stage launches)
extern "C" int ht_debug_prepare_frames_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, void *stream)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	const int fr = ctx->par.subsample_fraction > 0 ? ctx->par.subsample_fraction : 1;
	const long long n = ((long long)w * h + fr - 1) / fr;
	if (!d_depth || !d_cams || !ht_frame_dims_ok(w, h) || n > HT_POINTS_LIMIT) return HT_ERR_ARG;
	{ int r; if ((r = fv_buffers(ctx)) || (r = ht_reserve_points_locked(ctx, n < HT_MAXPTS ? HT_MAXPTS : (int)n))) return r; }
	int *over = ctx->d_view_src + (size_t)ctx->B * 2 * HT_VIEWS_MAX;
	ht_launch_prepare_frame(d_depth, d_cams, w, h, ctx->par.drangey, fr, ctx->d_pts, ctx->d_npts, over, ctx->model.pts_cap, B, ht_user_stream(ctx, stream));
	ctx->model.pts_bound = 0; ctx->views_B = 0;
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
// one pass of ht_fit_rows' launch sequence (ht_fit_rows_enqueue) on model `which` against the slots' prepared points, without caller rows, the momenta kept
extern "C" int ht_debug_fit_rows_pass_dev(ht_ctx *ctx, int which, int B, void *stream)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (which < 0 || which > 1) return HT_ERR_ARG;
	REFUSE_EXACT_SOLVER(ctx);
	{ const int r = ht_user_rows_reserve(ctx, 1, 1); if (r) return r; }
	hipStream_t s = ht_user_stream(ctx, stream);
	HIPCHK(ctx, hipMemsetAsync(ctx->d_user_n, 0, 4 * (size_t)ctx->B * sizeof(int), s));
	ht_fit_rows_enqueue(ctx, which, B, ctx->par.microforce, 0, 0, s);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
