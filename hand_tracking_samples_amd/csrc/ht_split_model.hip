// ht_split_model.hip -- two hands that touch or cross: the foreground cells of a frame's quarter image go to the hand whose tracked model is nearer (an addition;
// DESIGN section 31).  The label image, info and masked frames have the shape of the blob split's (ht_split.hip, section 27), so k_split_write, k_split_cams, the
// hands staging and the flagged update follow unchanged.  W4 = w / 4, H4 = h / 4, sizes as ht_split_hands':
//   cell depth      Q[Y][X] = the minimum of the 4x4 block, (x*, y*) the first pixel of the block in raster order that attains it; foreground range_lo <= Q < range_hi
//   cell point      v = deprojectz((x*, y*), (float)Q * depth_scale) with the frame's camera (misc_image.h:48; focal, principal point, depth_scale: its pose is not used)
//   priors          poses [B][2][nb][7]: 0 the right hand, 1 the left hand in real space, centre-of-mass poses in the camera's own space.  The left one is mirrored into
//                   canonical space (section 26's pose mirror: sign bits) unless the caller says it is canonical already; with HT_SPLIT_USER_POSES pos += qrot(q, com[b])
//                   then, in canonical space, where com[b] is the body's
//   distances       d_R = dot(plane, (v, 1)), plane = closest(bodies at the right prior, v) (physmodel.h:137-162); d_L the same with the canonical left prior and the
//                   point (-v.x, v.y, v.z).  fp32, one IEEE operation after another in the reference's order (the library is built without contraction)
//   assignment      label 0 (right) iff d_R <= d_L, else 1; background (0xFFFF) when (d_L < d_R ? d_L : d_R) > max_dist
//   info [2][8]     count, label (0 or 1), sum_x, sum_y, min_x, min_y, max_x, max_y over the cells of each label; a hand of count < min_pixels is absent (0, 0xFFFF, 0, ...)
//   modes           HT_SPLIT_MODEL_ALWAYS: every frame as above.  HT_SPLIT_MODEL_MERGED: behind k_split_label, a frame takes the above iff the blob split found fewer
//                   than two components AND both hands come out present; otherwise what k_split_label wrote stands untouched
//
// Mapping.  k_split_model: one block of 512 threads per frame.  All face planes of the model go to LDS once (both hands read them: only the left hand's poses and
// points are mirrored), and one body table per hand (SM_BT floats per body, lane <-> (hand, body)).  The frame is walked in chunks of 512 cells in raster order, a thread
// a cell: Q and (x*, y*), the chunk's foreground cells compacted in raster order into a list (ballot + per-wave sums), then one lane per (cell, hand): the reference's
// two walks over the bodies as they are written (inner-sphere planes; then per body the outer-sphere test against the running minimum and its most-above face), the
// pair's two distances meet through one cross-lane exchange (the lanes of a pair are neighbours).  Labels wait as 2-bit codes in LDS until the frame's counts are
// known (MERGED may leave the blob split's standing); counts, sums and boxes by integer LDS atomics: order-free, exact.  Every loop is bounded by a count known when
// it is entered; no lane waits for another but at the block's barriers.  (The other route, ht_cloud.hip's closest_chunk in a header, was not taken: ht_cloud.hip stays
// as it is.)
#include <string.h>
#include "ht_host.hpp"

#define SM_THREADS 512
#define SM_MAXCELLS 19200
#define SM_BT 32      // floats per body-table entry: pos 0..2 | radius 3 | rinner 4 | invp 5..7 | RI columns 8..16 | RF columns 17..25 | first face, faces (as integers) 26, 27
#define SM_NONE 0xFFFFu
#define SM_SPLIT_FLAGS (HT_SPLIT_RIGHT_IS_LOW_X | HT_SPLIT_MIRROR_LEFT)

extern __shared__ __attribute__((aligned(16))) float4 sm_planes[];      // all face planes of the model

// closest(rigidbodies, v), physmodel.h:137-162, for one point by one lane against the bodies of `tab`: the distance of v above the plane it returns
__device__ __forceinline__ float sm_closest(const float *tab, int nb, v3 v)
{
	float dmin = dot_plane(V4(0, 0, 0, FLT_MAX), v);
	for (int b = 0; b < nb; b++)      // :141-150
	{
		const float *t = tab + b * SM_BT;
		const v3 pos = V3(t[0], t[1], t[2]);
		const v3 n = safenormalize(v - pos);
		const float d = dot_plane(V4(n, -dot(pos, n) - t[4]), v);
		if (d < dmin) dmin = d;
	}
	for (int b = 0; b < nb; b++)      // :151-160
	{
		const float *t = tab + b * SM_BT;
		const v3 pos = V3(t[0], t[1], t[2]);
		if (length(v - pos) - t[3] > dmin) continue;
		const v3 X = V3(t[8], t[9], t[10]), Y = V3(t[11], t[12], t[13]), Z = V3(t[14], t[15], t[16]);
		const v3 vl = V3(t[5], t[6], t[7]) + ((X * v.x + Y * v.y) + Z * v.z);      // pose.inverse() * v
		const float4 *pl = sm_planes + __float_as_int(t[26]);
		const int np = __float_as_int(t[27]);
		float4 f = pl[0];      // mostabove :127-131: std::max_element keeps the first maximum
		float best = dot_plane(V4(f.x, f.y, f.z, f.w), vl);
		for (int i = 1; i < np; i++)
		{
			const float4 g = pl[i];
			const float d = dot_plane(V4(g.x, g.y, g.z, g.w), vl);
			if (best < d) { best = d; f = g; }
		}
		const v3 FX = V3(t[17], t[18], t[19]), FY = V3(t[20], t[21], t[22]), FZ = V3(t[23], t[24], t[25]);
		const v3 n = (FX * f.x + FY * f.y) + FZ * f.z;      // Pose::TransformPlane, geometric.h:124
		const float d = dot_plane(V4(n, f.w - dot(pos, n)), v);
		if (d < dmin) dmin = d;
	}
	return dmin;
}

// poses: hand k of frame f at poses + ((2 f + k) nb + b) pose_stride (7: poses; HT_STATE_STRIDE: the slots' state).  merged: ncomp [B] holds k_split_label's counts and
// info / labels its results.  labels is never null; ncomp only in ALWAYS mode; source and dist may be
__global__ __launch_bounds__(SM_THREADS) void k_split_model(const ht_model_dev M, const uint16_t *__restrict__ depth, const float *__restrict__ cams, const float *__restrict__ poses, int pose_stride, int w, int h,
                                                            unsigned lo, unsigned hi, int min_pixels, float max_dist, int merged, int user_poses, int left_canonical, int wide,
                                                            int32_t *__restrict__ info, int32_t *__restrict__ ncomp, int32_t *__restrict__ source, float *__restrict__ dist, uint16_t *__restrict__ labels)
{
	__shared__ __align__(16) float tab[2][HT_MAXNB * SM_BT];
	__shared__ __align__(16) unsigned list[SM_THREADS];           // the chunk's foreground cells: thread | first minimal pixel << 9 | Q << 13
	__shared__ __align__(16) unsigned codes[SM_MAXCELLS / 16];    // 2 bits a cell: 0 background, 1 right, 2 left
	__shared__ __align__(16) int stats[2][8];
	__shared__ int wsum[SM_THREADS / 64];
	__shared__ int misc[8];
	const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, f = blockIdx.x;
	const unsigned W4 = (unsigned)w >> 2, H4 = (unsigned)h >> 2, n = W4 * H4;
	const int nb = M.nb;
	const float inf = __uint_as_float(0x7F800000u);
	if (merged && ncomp[f] >= 2)      // the blob split stands (the whole block leaves: nothing waits at a barrier)
	{
		if (t == 0 && source) source[f] = 0;
		if (dist) for (unsigned i = t; i < 2u * n; i += SM_THREADS) dist[(size_t)f * 2u * n + i] = inf;
		return;
	}
	{
		const int np = M.plane_off[nb];
		for (int i = (int)t; i < np; i += SM_THREADS) sm_planes[i] = M.planes[i];
	}
	if (t < 2u * HT_MAXNB && (int)(t & (HT_MAXNB - 1u)) < nb)
	{
		const unsigned k = t / HT_MAXNB; const int b = (int)(t & (HT_MAXNB - 1u));
		const unsigned *p = (const unsigned *)(poses + ((size_t)(2u * f + k) * (unsigned)nb + (unsigned)b) * (unsigned)pose_stride);
		const unsigned flip = (k && !left_canonical) ? 0x80000000u : 0u;
		v3 pos = V3(__uint_as_float(p[0] ^ flip), __uint_as_float(p[1]), __uint_as_float(p[2]));
		const v4 q = V4(__uint_as_float(p[3]), __uint_as_float(p[4] ^ flip), __uint_as_float(p[5] ^ flip), __uint_as_float(p[6]));
		const float *bc = M.bodyc + b * HT_BC;
		if (user_poses) pos = pos + qrot(q, V3(bc[HT_BC_COM], bc[HT_BC_COM + 1], bc[HT_BC_COM + 2]));
		const xf pi = inverse(XF(pos, q));
		const m3 ri = qmat(pi.q), rf = qmat(q);
		float *e = &tab[k][b * SM_BT];
		e[0] = pos.x; e[1] = pos.y; e[2] = pos.z; e[3] = bc[HT_BC_RADIUS]; e[4] = bc[HT_BC_RINNER];
		e[5] = pi.p.x; e[6] = pi.p.y; e[7] = pi.p.z;
		e[8] = ri.x.x; e[9] = ri.x.y; e[10] = ri.x.z; e[11] = ri.y.x; e[12] = ri.y.y; e[13] = ri.y.z; e[14] = ri.z.x; e[15] = ri.z.y; e[16] = ri.z.z;
		e[17] = rf.x.x; e[18] = rf.x.y; e[19] = rf.x.z; e[20] = rf.y.x; e[21] = rf.y.y; e[22] = rf.y.z; e[23] = rf.z.x; e[24] = rf.z.y; e[25] = rf.z.z;
		e[26] = __int_as_float(M.plane_off[b]); e[27] = __int_as_float(M.plane_off[b + 1] - M.plane_off[b]);
	}
	for (unsigned i = t; i < (n + 15u) / 16u; i += SM_THREADS) codes[i] = 0u;
	if (t < 16) (&stats[0][0])[t] = (t & 7u) == 4u || (t & 7u) == 5u ? 0x7fffffff : 0;
	const float *cam = cams + (size_t)f * HT_CAM;
	const float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], dscale = cam[4];
	const uint16_t *src = depth + (size_t)f * (unsigned)w * (unsigned)h;
	__syncthreads();
	for (unsigned base = 0; base < n; base += SM_THREADS)
	{
		// a thread a cell: Q, its first minimal pixel, foreground
		const unsigned i = base + t;
		unsigned m = 0x10000u, at = 0;
		if (i < n)
		{
			const unsigned Y = i / W4, X = i - Y * W4;
			const uint16_t *p = src + (size_t)(4u * Y) * (unsigned)w + 4u * X;
#pragma unroll
			for (unsigned r = 0; r < 4; r++)
			{
				unsigned px[4];
				if (wide) { const uint2 u = *(const uint2 *)(p + (size_t)r * (unsigned)w); px[0] = u.x & 0xFFFFu; px[1] = u.x >> 16; px[2] = u.y & 0xFFFFu; px[3] = u.y >> 16; }
				else { px[0] = p[(size_t)r * (unsigned)w]; px[1] = p[(size_t)r * (unsigned)w + 1]; px[2] = p[(size_t)r * (unsigned)w + 2]; px[3] = p[(size_t)r * (unsigned)w + 3]; }
#pragma unroll
				for (unsigned c = 0; c < 4; c++) if (px[c] < m) { m = px[c]; at = r * 4u + c; }
			}
		}
		const bool fg = i < n && m >= lo && m < hi;
		const unsigned long long bal = __ballot(fg);
		if (lane == 0) wsum[wave] = __popcll(bal);
		__syncthreads();
		int before = 0, total = 0;
#pragma unroll
		for (unsigned k = 0; k < SM_THREADS / 64; k++) { const int c = wsum[k]; if (k < wave) before += c; total += c; }
		if (fg) list[before + __popcll(bal & ((1ull << lane) - 1ull))] = t | (at << 9) | (m << 13);
		else if (i < n && dist) { dist[((size_t)f * n + i) * 2u] = inf; dist[((size_t)f * n + i) * 2u + 1u] = inf; }
		__syncthreads();
		// a lane a (cell, hand): lanes 2 c and 2 c + 1 carry cell c of the list
		for (unsigned p = t; p < 2u * (unsigned)total; p += SM_THREADS)
		{
			const unsigned e = list[p >> 1], k = p & 1u;
			const unsigned ci = base + (e & 511u), a = (e >> 9) & 15u, Q = e >> 13;
			const unsigned Y = ci / W4, X = ci - Y * W4;
			const float x = (float)(4u * X + (a & 3u)), y = (float)(4u * Y + (a >> 2));
			const float d = (float)Q * dscale;
			v3 v = V3(((x - cx) / fx) * d, ((y - cy) / fy) * d, 1.0f * d);
			if (k) v.x = -v.x;
			const float mine = sm_closest(tab[k], nb, v);
			const float other = __shfl_xor(mine, 1);
			if (!k)
			{
				const float dR = mine, dL = other;
				unsigned code = dR <= dL ? 1u : 2u;
				if ((dL < dR ? dL : dR) > max_dist) code = 0u;
				if (dist) { dist[((size_t)f * n + ci) * 2u] = dR; dist[((size_t)f * n + ci) * 2u + 1u] = dL; }
				if (code)
				{
					int *s = stats[code - 1u];
					atomicOr(&codes[ci >> 4], code << ((ci & 15u) * 2u));
					atomicAdd(&s[0], 1); atomicAdd(&s[2], (int)X); atomicAdd(&s[3], (int)Y);
					atomicMin(&s[4], (int)X); atomicMin(&s[5], (int)Y); atomicMax(&s[6], (int)X); atomicMax(&s[7], (int)Y);
				}
			}
		}
		__syncthreads();      // the list is free for the next chunk
	}
	if (t == 0)
	{
		const int r = stats[0][0] >= min_pixels, l = stats[1][0] >= min_pixels;
		misc[0] = r; misc[1] = l; misc[2] = !merged || (r && l);
	}
	__syncthreads();
	if (!misc[2]) { if (t == 0 && source) source[f] = 0; return; }      // MERGED and a hand would be absent: the blob split stands
	if (t < 16)
	{
		const unsigned k = t >> 3, e = t & 7u;
		info[(size_t)f * 16 + t] = misc[k] ? (e == 1 ? (int)k : stats[k][e]) : (e == 1 ? (int)SM_NONE : 0);
		if (t == 0 && source) source[f] = 1;
		if (t == 0 && !merged && ncomp) ncomp[f] = misc[0] + misc[1];
	}
	for (unsigned i = t; i < n; i += SM_THREADS)
	{
		const unsigned c = (codes[i >> 4] >> ((i & 15u) * 2u)) & 3u;
		labels[(size_t)f * n + i] = (uint16_t)(c ? c - 1u : SM_NONE);
	}
}

// ---- launch layer ------------------------------------------------------------------------------------------------------------------------------------------------
// LDS of a block: the kernel's own tables and the model's planes; two blocks must fit a CU's 160 KB
static const size_t SM_LDS_FIXED = sizeof(float) * 2 * HT_MAXNB * SM_BT + sizeof(unsigned) * SM_THREADS + sizeof(unsigned) * (SM_MAXCELLS / 16) + 64 + 32 + 32;
int ht_split_model_check(ht_ctx *ctx, const char *fn, float max_dist, int mode, int flags)
{
	const std::string f(fn);
	if (ctx->cnn_only) { ctx->err = f + ": this context was created without a hand model (CNN only)"; return HT_ERR_STATE; }
	if ((size_t)ctx->model.plane_off[ctx->model.nb] * sizeof(float4) + SM_LDS_FIXED > 80 * 1024) { ctx->err = f + ": the model's face planes do not fit the kernel's LDS"; return HT_ERR_STATE; }
	if (!(max_dist >= 0.0f)) { ctx->err = f + ": max_dist must be a distance in metres, +inf or FLT_MAX for none (not NaN, not negative)"; return HT_ERR_ARG; }
	if (mode != HT_SPLIT_MODEL_ALWAYS && mode != HT_SPLIT_MODEL_MERGED) { ctx->err = f + ": mode is HT_SPLIT_MODEL_ALWAYS or HT_SPLIT_MODEL_MERGED"; return HT_ERR_ARG; }
	if (flags & ~(SM_SPLIT_FLAGS | HT_SPLIT_USER_POSES)) { ctx->err = f + ": unknown flag bits"; return HT_ERR_ARG; }
	if (mode == HT_SPLIT_MODEL_ALWAYS && (flags & HT_SPLIT_RIGHT_IS_LOW_X)) { ctx->err = f + ": HT_SPLIT_RIGHT_IS_LOW_X means nothing in HT_SPLIT_MODEL_ALWAYS mode"; return HT_ERR_ARG; }
	return HT_OK;
}
// the split step of a model call: k_split_label first in MERGED mode (its counts into ncomp, never null then), then k_split_model
void ht_launch_split_model(ht_ctx *ctx, const uint16_t *depth, const float *cams, const float *poses, int pose_stride, int left_canonical, int w, int h, int B, unsigned lo, unsigned hi, unsigned max_step,
                           int min_pixels, float max_dist, int mode, int flags, int32_t *info, int32_t *ncomp, int32_t *source, float *dist, uint16_t *labels, hipStream_t s)
{
	const int merged = mode == HT_SPLIT_MODEL_MERGED;
	if (merged) { ht_prof_scope ps(ctx, "k_split_label", s); ht_launch_split_label(depth, w, h, B, lo, hi, max_step, min_pixels, flags & SM_SPLIT_FLAGS, info, ncomp, labels, s); }
	const size_t dyn = (size_t)ctx->model.plane_off[ctx->model.nb] * sizeof(float4);
	static ht_lds_limit limit; limit.raise(dyn, k_split_model);
	ht_prof_scope ps(ctx, "k_split_model", s);
	hipLaunchKernelGGL(k_split_model, dim3(B), dim3(SM_THREADS), dyn, s, ctx->model, depth, cams, poses, pose_stride, w, h, lo, hi, min_pixels, max_dist, merged, (flags & HT_SPLIT_USER_POSES) ? 1 : 0, left_canonical,
	                   ((uintptr_t)depth & 7) == 0 ? 1 : 0, info, ncomp, source, dist, labels);
}
// the label image and the blob split's counts of a call whose caller wants none: the context keeps them, grown to the largest call
static int split_model_reserve(ht_ctx *ctx, int w, int h, int B, bool want_labels, bool want_ncomp)
{
	const size_t cells = (size_t)B * (w / 4) * (h / 4);
	if ((want_labels && cells > ctx->split_labels_cap) || (want_ncomp && (size_t)B > ctx->model_ncomp_cap)) HIPCHK(ctx, ht_sync_all(ctx));
	if (want_labels) { const int r = dev_grow(ctx, &ctx->d_split_labels, &ctx->split_labels_cap, cells); if (r) return r; }
	if (want_ncomp) { const int r = dev_grow(ctx, &ctx->d_model_ncomp, &ctx->model_ncomp_cap, (size_t)B); if (r) return r; }
	return HT_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------------------------------------
// Every check runs before anything grows or launches.  B is not bounded by max_batch: no tracker slot, no weights.
static int split_model_check_call(ht_ctx *ctx, const void *in, const void *cams, const void *poses, const void *out, const void *info, int w, int h, int B, int range_lo, int range_hi, int min_pixels, int far,
                                  float max_dist, int mode, int flags)
{
	{ const int r = ht_split_model_check(ctx, "ht_split_hands_model", max_dist, mode, flags); if (r) return r; }
	if (!in || !cams || !poses || !out || !info || B < 0 || (B > 0x7fffffff / 24)) { ctx->err = "ht_split_hands_model: bad argument (depth, cams, poses, depth_out and info are required)"; return HT_ERR_ARG; }
	{ const int r = ht_split_check(ctx, "ht_split_hands_model", w, h, range_lo, range_hi, min_pixels, far, flags & SM_SPLIT_FLAGS); if (r) return r; }
	const size_t bytes = (size_t)B * w * h * sizeof(uint16_t);
	if (ht_ranges_overlap(in, bytes, out, 2 * bytes)) { ctx->err = "ht_split_hands_model: depth and depth_out must not overlap"; return HT_ERR_ARG; }
	return HT_OK;
}
extern "C" int ht_split_hands_model_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_poses, int w, int h, int B, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels,
                                        uint16_t far, float max_dist, int mode, int flags, uint16_t *d_depth_out, float *d_cams_out, int32_t *d_info, int32_t *d_n_components, int32_t *d_source, float *d_dist,
                                        uint16_t *d_label_img, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = split_model_check_call(ctx, d_depth, d_cams, d_poses, d_depth_out, d_info, w, h, B, range_lo, range_hi, min_pixels, far, max_dist, mode, flags); if (r) return r; }
	if (B == 0) return HT_OK;
	const bool need_ncomp = mode == HT_SPLIT_MODEL_MERGED && !d_n_components;
	{ const int r = split_model_reserve(ctx, w, h, B, !d_label_img, need_ncomp); if (r) return r; }
	if (!d_label_img) d_label_img = ctx->d_split_labels;
	hipStream_t s = ht_user_stream(ctx, stream);
	ht_launch_split_model(ctx, d_depth, d_cams, d_poses, HT_POSE, 0, w, h, B, range_lo, range_hi, max_step, min_pixels, max_dist, mode, flags, d_info, need_ncomp ? ctx->d_model_ncomp : d_n_components, d_source, d_dist,
	                      d_label_img, s);
	{ ht_prof_scope ps(ctx, "k_split_write", s); ht_launch_split_write(d_depth, d_label_img, d_info, w, h, B, far, flags & SM_SPLIT_FLAGS, d_depth_out, s); }
	if (d_cams_out) { ht_prof_scope ps(ctx, "k_split_cams", s); ht_launch_split_cams(d_cams, w, B, flags & SM_SPLIT_FLAGS, d_cams_out, s); }
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
// The host form: inputs and outputs through the context's staging (ht_staged_call), the same kernels
extern "C" int ht_split_hands_model(ht_ctx *ctx, const uint16_t *depth, const float *cams, const float *poses, int w, int h, int B, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far,
                                    float max_dist, int mode, int flags, uint16_t *depth_out, float *cams_out, int32_t *info, int32_t *n_components, int32_t *source, float *dist, uint16_t *labels)
{
	CHECK_READY(ctx);
	{ const int r = split_model_check_call(ctx, depth, cams, poses, depth_out, info, w, h, B, range_lo, range_hi, min_pixels, far, max_dist, mode, flags); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t bytes = (size_t)B * w * h * sizeof(uint16_t), cb = (size_t)B * HT_CAM * sizeof(float), cells = (size_t)B * (w / 4) * (h / 4);
	ht_seg seg[10] = { { (void *)depth, bytes, false }, { (void *)cams, cb, false }, { (void *)poses, (size_t)B * 2 * ctx->model.nb * HT_POSE * sizeof(float), false }, { depth_out, 2 * bytes, true },
	                   { cams_out, 2 * cb, true }, { info, (size_t)B * 16 * sizeof(int32_t), true }, { n_components, (size_t)B * sizeof(int32_t), true }, { source, (size_t)B * sizeof(int32_t), true },
	                   { dist, cells * 2 * sizeof(float), true }, { labels, cells * sizeof(uint16_t), true } };
	return ht_staged_call(ctx, seg, 10, [&](hipStream_t s)
	                      { return ht_split_hands_model_dev(ctx, (const uint16_t *)seg[0].dev, (const float *)seg[1].dev, (const float *)seg[2].dev, w, h, B, range_lo, range_hi, max_step, min_pixels, far, max_dist, mode,
	                                                        flags, (uint16_t *)seg[3].dev, (float *)seg[4].dev, (int32_t *)seg[5].dev, (int32_t *)seg[6].dev, (int32_t *)seg[7].dev, (float *)seg[8].dev,
	                                                        (uint16_t *)seg[9].dev, s); });
}
