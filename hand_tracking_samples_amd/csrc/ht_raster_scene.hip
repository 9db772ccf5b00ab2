// ht_raster_scene.hip -- scenes of up to four hands, each right or left, rasterised into one z-buffer over an optional background frame, with per-pixel hand and
// body labels, for a batch of frames.  The definition is the host's ht_model_raster_scene (ht_model_host.hip; include/ht_mi355x.h states it): both call ht_raster.hpp's
// functions, the per-triangle ones and the scene's (mirrored pose and principal point, column flip, limits, composite rule), so every output is bit-identical to the
// host's (tests/test_gpu_raster_scene.py).  DESIGN section 36.
//
// Mapping: k_raster_mesh's (ht_raster_mesh.hip), one block of four waves per (frame, band of rows), the band's z-buffer in LDS; the table entry, the pass over the
// triangles (rz_triangles) and the packers are the same functions of ht_raster_band.hpp, called here once per present instance.  What differs:
//   key        count << 16 | (instance * T + triangle), T the model's mesh triangles: the smallest key is the definition's winner (smallest count, then the lowest
//              instance, then the first in (body, triangle) order) whatever the order of arrival; instances * T <= 65535 keeps 0xffffffff for "nothing yet"
//   instances  walked one after another with ONE pose table in LDS, rebuilt behind a barrier (four tables would cost the second block per CU).  The flag of an
//              instance is uniform over the block, so the barriers and the wave walk's ballots stay block-uniform.  A left instance builds its table from the
//              mirrored pose, projects through the mirrored principal point and writes the z-buffer at column w-1-x, in the lane's walk and the wave's alike
//   write-out  four pixels per thread: the background read with the width the depth is written with, by the thread that writes the pixel (bg == depth composes in
//              place); hand and body decoded from the index; visible counted in registers, reduced over the wave, one integer atomic add per wave and instance
#include "ht_raster_band.hpp"

__global__ __launch_bounds__(RZ_THREADS) void k_raster_scene(const rz_model M, const float *__restrict__ poses, const unsigned char *__restrict__ hands, const float *__restrict__ cams, int H, int w, int h,
                                                             float F, float off, int f0, int bands, int rows, const uint16_t *bg, uint16_t *depth, int8_t *hand, int8_t *body, int *visible)
{
	__shared__ uint4 zb4[RZ_PIX / 4];
	__shared__ float tab[HT_MAXNB * 12];
	unsigned *zb = (unsigned *)zb4;
	const int t = threadIdx.x, lane = t & 63;
	const int frame = f0 + blockIdx.x / bands, band = blockIdx.x % bands;
	const int y0 = band * rows, y1 = min(h, y0 + rows) - 1, npx = (y1 - y0 + 1) * w;      // npx <= RZ_PIX (rz_band_rows)
	const int nb = M.nb, NT = M.ntri;
	const float *cam = cams + (size_t)frame * HT_CAM;
	const float fx = cam[0], fy = cam[1], cx = cam[2], py = cam[3], ds = cam[4];
	for (int i = t; i < (npx + 3) / 4; i += RZ_THREADS) zb4[i] = make_uint4(RZ_NONE, RZ_NONE, RZ_NONE, RZ_NONE);
	for (int inst = 0; inst < H; inst++)
	{
		const unsigned char flag = hands ? hands[(size_t)frame * H + inst] : (unsigned char)0;      // uniform over the block
		if (rz_scene_absent(flag)) continue;
		const bool left = rz_scene_left(flag);
		const float px = left ? rz_mirror_px(cx, w, off) : cx;
		__syncthreads();      // the instance before has read the table for the last time
		if (t < nb)
		{
			const float *g = poses + (((size_t)frame * H + inst) * nb + t) * HT_POSE;
			float p[HT_POSE] = { g[0], g[1], g[2], g[3], g[4], g[5], g[6] };
			if (left) { float m[HT_POSE]; rz_mirror_pose(p, m); for (int k = 0; k < HT_POSE; k++) p[k] = m[k]; }
			rz_table_put(tab + t * 12, p, M.com + 3 * t);
		}
		__syncthreads();      // the table stands (and, the first time, the z-buffer is cleared)
		rz_triangles(zb, M, tab, t, y0, y1, w, left, fx, fy, px, py, off, F, ds, (unsigned)(inst * NT));
	}
	__syncthreads();
	// write-out: the band's pixels are [o0, o0 + npx) of the batch, in groups of four aligned in the batch
	const bool has_bg = bg != nullptr;
	const unsigned short none = (unsigned short)(F / ds);
	const size_t o0 = ((size_t)frame * h + y0) * w;
	const size_t g0 = o0 >> 2, g1 = (o0 + npx - 1) >> 2;
	const bool vec = (((uintptr_t)depth | (uintptr_t)bg) & 7) == 0 && (((uintptr_t)hand | (uintptr_t)body) & 3) == 0;      // a caller's buffers may start anywhere: then pixel by pixel
	int seen[HT_SCENE_MAX_HANDS] = { 0, 0, 0, 0 };
	for (size_t g = g0 + t; g <= g1; g += RZ_THREADS)
	{
		const long long i0 = (long long)(4 * g) - (long long)o0;      // the group's first pixel in the band: -3 .. npx - 1
		const bool whole = vec && i0 >= 0 && i0 + 3 < npx;
		unsigned short under[4] = { none, none, none, none };
		if (has_bg)
		{
			if (whole)
			{
				const uint2 v = *(const uint2 *)(bg + 4 * g);
				under[0] = (unsigned short)v.x; under[1] = (unsigned short)(v.x >> 16); under[2] = (unsigned short)v.y; under[3] = (unsigned short)(v.y >> 16);
			}
			else
			{
#pragma unroll
				for (int j = 0; j < 4; j++) if (i0 + j >= 0 && i0 + j < npx) under[j] = bg[4 * g + j];
			}
		}
		unsigned key[4];
#pragma unroll
		for (int j = 0; j < 4; j++) key[j] = (i0 + j >= 0 && i0 + j < npx) ? zb[i0 + j] : RZ_NONE;
		unsigned short d[4] = { under[0], under[1], under[2], under[3] }; int hi[4] = { -1, -1, -1, -1 }, who[4] = { -1, -1, -1, -1 };
		if ((key[0] & key[1] & key[2] & key[3]) != RZ_NONE)      // most groups of a frame show no hand: nothing to decode
		{
#pragma unroll
			for (int j = 0; j < 4; j++)
			{
				const int n = (int)(key[j] >> 16), idx = (int)(key[j] & 0xffffu);
				const bool on = key[j] != RZ_NONE && rz_scene_wins(n, has_bg, under[j]);
				const int ih = (idx >= NT ? 1 : 0) + (idx >= 2 * NT ? 1 : 0) + (idx >= 3 * NT ? 1 : 0);      // idx / NT for at most four instances
				if (on) { d[j] = (unsigned short)n; hi[j] = ih; who[j] = body ? rz_body_of(M, idx - ih * NT) : 0; }
#pragma unroll
				for (int a = 0; a < HT_SCENE_MAX_HANDS; a++) seen[a] += hi[j] == a ? 1 : 0;
			}
		}
		if (whole)
		{
			*(uint2 *)(depth + 4 * g) = rz_pack_u16(d);
			if (hand) *(unsigned *)(hand + 4 * g) = rz_pack_i8(hi);
			if (body) *(unsigned *)(body + 4 * g) = rz_pack_i8(who);
		}
		else
		{
#pragma unroll
			for (int j = 0; j < 4; j++) if (i0 + j >= 0 && i0 + j < npx) { depth[4 * g + j] = d[j]; if (hand) hand[4 * g + j] = (int8_t)hi[j]; if (body) body[4 * g + j] = (int8_t)who[j]; }
		}
	}
	if (visible)      // uniform: every lane of every wave takes part in the reduction
	{
#pragma unroll
		for (int a = 0; a < HT_SCENE_MAX_HANDS; a++)
		{
			int s = seen[a];
			for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
			if (lane == 0 && a < H && s) atomicAdd(&visible[(size_t)frame * H + a], s);
		}
	}
}

// every check of both entries, before anything grows or launches; bg == depth exactly is the in-place composition, any other overlap among the buffers is refused
static int rs_check_args(ht_ctx *ctx, const float *poses, const unsigned char *hands, int H, const float *cams, int w, int h, float far, float off, int B, const uint16_t *bg, const uint16_t *depth,
                         const int8_t *hand, const int8_t *body, const int32_t *visible)
{
	if (H < 1 || H > HT_SCENE_MAX_HANDS) { ctx->err = "ht_raster_scene_depth: between 1 and HT_SCENE_MAX_HANDS instances a frame"; return HT_ERR_ARG; }
	{ const int r = rc_check_args(ctx, "ht_raster_scene_depth", poses, cams, depth, w, h, far, B, off >= 0.0f && off <= 1.0f); if (r) return r; }
	if (!ctx->d_mesh) { ctx->err = "the model file holds no subdivision meshes (bake it again)"; return HT_ERR_STATE; }
	if (!rz_scene_fits(H, ctx->rec.mesh_off[ctx->model.nb])) { ctx->err = "ht_raster_scene_depth: instances times mesh triangles exceed 65535 (the z-buffer keeps a 16-bit index)"; return HT_ERR_STATE; }
	const size_t npx = (size_t)B * w * h, nb = (size_t)ctx->model.nb;
	const struct { const void *p; size_t bytes; } buf[8] = { { depth, npx * sizeof(uint16_t) }, { hand, npx }, { body, npx }, { visible, (size_t)B * H * sizeof(int32_t) },      // the outputs first
	                                                         { bg == depth ? nullptr : bg, npx * sizeof(uint16_t) }, { poses, (size_t)B * H * nb * HT_POSE * sizeof(float) },
	                                                         { hands, (size_t)B * H }, { cams, (size_t)B * HT_CAM * sizeof(float) } };
	for (int i = 0; i < 4; i++) for (int j = i + 1; j < 8; j++)
		if (ht_ranges_overlap(buf[i].p, buf[i].bytes, buf[j].p, buf[j].bytes)) { ctx->err = "ht_raster_scene_depth: the buffers overlap (only bg == depth, exactly, composes in place)"; return HT_ERR_ARG; }
	return HT_OK;
}

extern "C" int ht_raster_scene_depth_dev(ht_ctx *ctx, const float *d_poses, const uint8_t *d_hands, int H, const float *d_cams, int w, int h, float far, float pixel_offset, int B, const uint16_t *d_bg,
                                         uint16_t *d_depth, int8_t *d_hand, int8_t *d_body, int32_t *d_visible, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = rs_check_args(ctx, d_poses, d_hands, H, d_cams, w, h, far, pixel_offset, B, d_bg, d_depth, d_hand, d_body, d_visible); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const rz_model m = rz_model_of(ctx);
	if (d_visible) HIPCHK(ctx, hipMemsetAsync(d_visible, 0, (size_t)B * H * sizeof(int32_t), s));
	const int rows = rz_band_rows(w, h), bands = (h + rows - 1) / rows;
	const int per = INT_MAX / bands;      // frames per launch (grid size limit)
	for (int f0 = 0; f0 < B; f0 += per)
		hipLaunchKernelGGL(k_raster_scene, dim3(min(per, B - f0) * bands), dim3(RZ_THREADS), 0, s, m, d_poses, d_hands, d_cams, H, w, h, far, pixel_offset, f0, bands, rows, d_bg, d_depth, d_hand, d_body,
		                   (int *)d_visible);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

// The synchronous form: everything staged through the context's buffer (ht_staged_call; no tracker slot is used, so B is not bounded by max_batch).  The staging's
// segments are 256-byte aligned, so the write-out takes its vector path; bg == depth on the host becomes two segments, which is the same composition.
extern "C" int ht_raster_scene_depth(ht_ctx *ctx, const float *poses, const uint8_t *hands, int H, const float *cams, int w, int h, float far, float pixel_offset, int B, const uint16_t *bg,
                                     uint16_t *depth, int8_t *hand, int8_t *body, int32_t *visible)
{
	CHECK_READY(ctx);
	{ const int r = rs_check_args(ctx, poses, hands, H, cams, w, h, far, pixel_offset, B, bg, depth, hand, body, visible); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t nb = (size_t)ctx->model.nb, npx = (size_t)B * w * h;
	ht_seg seg[8] = { { (void *)poses, (size_t)B * H * nb * HT_POSE * sizeof(float), false }, { (void *)hands, (size_t)B * H, false }, { (void *)cams, (size_t)B * HT_CAM * sizeof(float), false },
	                  { (void *)bg, npx * sizeof(uint16_t), false }, { depth, npx * sizeof(uint16_t), true }, { hand, npx, true }, { body, npx, true }, { visible, (size_t)B * H * sizeof(int32_t), true } };
	return ht_staged_call(ctx, seg, 8, [&](hipStream_t s)
	                      { return ht_raster_scene_depth_dev(ctx, (const float *)seg[0].dev, (const uint8_t *)seg[1].dev, H, (const float *)seg[2].dev, w, h, far, pixel_offset, B, (const uint16_t *)seg[3].dev,
	                                                         (uint16_t *)seg[4].dev, (int8_t *)seg[5].dev, (int8_t *)seg[6].dev, (int32_t *)seg[7].dev, s); });
}
