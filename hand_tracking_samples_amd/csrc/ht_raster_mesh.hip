// ht_raster_mesh.hip -- the hand's subdivision surface rasterised on the device: a forward z-buffer over the meshes ht_render_mesh_depth ray-casts, for a
// batch of frames.  The definition is the host's ht_model_raster_mesh (ht_model_host.hip; include/ht_mi355x.h states it): both call ht_raster.hpp's set-up,
// coverage and depth functions, so a frame is bit-identical to the host's (tests/test_gpu_raster_mesh.py).  DESIGN section 35.
//
// Mapping: one block of four waves per (frame, band of rows).  The band's z-buffer lives in LDS, one 32-bit key per pixel: count << 16 | global triangle index,
// 0xffffffff for "nothing yet".  The smallest key is the definition's winner (smallest count, then the first in (body, triangle) order), and atomicMin makes
// the result independent of the order of arrival.
//   prologue   the z-buffer cleared; thread b < nb: R = qmat(q_b) and up_b = pos_b - R com_b into LDS
//   triangles  thread t takes triangles t, t + 256, ...: corners from the mesh rows on the device (ht_mesh_upload's, 48 of each row's 64 bytes), set-up,
//              its pixel rectangle clipped to the band; a small rectangle is walked by the lane alone, a large one (RZ_BIG pixels or more: a hand close
//              to the camera) by the whole wave, one column per lane
//   write-out  the band is contiguous in the frame: four pixels per thread as one 8-byte depth store and one 4-byte body store, where the alignment allows
// The table entry, the triangles stage (rz_triangles, with the pixel test and both walks) and the packers are ht_raster_band.hpp's, shared with k_raster_scene; the
// prologue and the write-out loop are here.
#include "ht_raster_band.hpp"

__global__ __launch_bounds__(RZ_THREADS) void k_raster_mesh(const rz_model M, const float *__restrict__ poses, const float *__restrict__ cams, int w, int h, float F, float off,
                                                            int f0, int bands, int rows, uint16_t *__restrict__ depth, int8_t *__restrict__ body)
{
	__shared__ uint4 zb4[RZ_PIX / 4];
	__shared__ float tab[HT_MAXNB * 12];
	unsigned *zb = (unsigned *)zb4;
	const int t = threadIdx.x;
	const int frame = f0 + blockIdx.x / bands, band = blockIdx.x % bands;
	const int y0 = band * rows, y1 = min(h, y0 + rows) - 1, npx = (y1 - y0 + 1) * w;      // npx <= RZ_PIX (rz_band_rows)
	const int nb = M.nb;
	const float *cam = cams + (size_t)frame * HT_CAM;
	const float fx = cam[0], fy = cam[1], px = cam[2], py = cam[3], ds = cam[4];
	for (int i = t; i < (npx + 3) / 4; i += RZ_THREADS) zb4[i] = make_uint4(RZ_NONE, RZ_NONE, RZ_NONE, RZ_NONE);
	if (t < nb) rz_table_put(tab + t * 12, poses + ((size_t)frame * nb + t) * HT_POSE, M.com + 3 * t);
	__syncthreads();
	rz_triangles(zb, M, tab, t, y0, y1, w, false, fx, fy, px, py, off, F, ds, 0u);
	__syncthreads();
	// write-out: the band's pixels are [o0, o0 + npx) of the batch, in groups of four aligned in the batch
	const unsigned short bg = (unsigned short)(F / ds);
	const size_t o0 = ((size_t)frame * h + y0) * w;
	const size_t g0 = o0 >> 2, g1 = (o0 + npx - 1) >> 2;
	const bool vec = ((uintptr_t)depth & 7) == 0 && ((uintptr_t)body & 3) == 0;      // a caller's buffers may start anywhere: then pixel by pixel
	for (size_t g = g0 + t; g <= g1; g += RZ_THREADS)
	{
		const long long i0 = (long long)(4 * g) - (long long)o0;      // the group's first pixel in the band: -3 .. npx - 1
		unsigned short d[4]; int who[4];
#pragma unroll
		for (int j = 0; j < 4; j++)
		{
			const long long i = i0 + j;
			const unsigned key = (i >= 0 && i < npx) ? zb[i] : RZ_NONE;
			d[j] = key == RZ_NONE ? bg : (unsigned short)(key >> 16);
			who[j] = key == RZ_NONE ? -1 : (body ? rz_body_of(M, (int)(key & 0xffffu)) : 0);
		}
		if (vec && i0 >= 0 && i0 + 3 < npx)
		{
			*(uint2 *)(depth + 4 * g) = rz_pack_u16(d);
			if (body) *(unsigned *)(body + 4 * g) = rz_pack_i8(who);
		}
		else
		{
#pragma unroll
			for (int j = 0; j < 4; j++) if (i0 + j >= 0 && i0 + j < npx) { depth[4 * g + j] = d[j]; if (body) body[4 * g + j] = (int8_t)who[j]; }
		}
	}
}

static int rz_check_args(ht_ctx *ctx, const void *poses, const void *cams, const void *depth, int w, int h, float far, float off, int B)
{
	{ const int r = rc_check_args(ctx, "ht_raster_mesh_depth", poses, cams, depth, w, h, far, B, off >= 0.0f && off <= 1.0f); if (r) return r; }
	if (!ctx->d_mesh) { ctx->err = "the model file holds no subdivision meshes (bake it again)"; return HT_ERR_STATE; }
	if (ctx->rec.mesh_off[ctx->model.nb] >= 65535) { ctx->err = "ht_raster_mesh_depth: the model has 65535 or more mesh triangles (the z-buffer keeps a 16-bit triangle index)"; return HT_ERR_STATE; }
	return HT_OK;
}

extern "C" int ht_raster_mesh_depth_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int w, int h, float far, float pixel_offset, int B, uint16_t *d_depth, int8_t *d_body, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = rz_check_args(ctx, d_poses, d_cams, d_depth, w, h, far, pixel_offset, B); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const rz_model m = rz_model_of(ctx);
	const int rows = rz_band_rows(w, h), bands = (h + rows - 1) / rows;
	const int per = INT_MAX / bands;      // frames per launch (grid size limit)
	for (int f0 = 0; f0 < B; f0 += per)
		hipLaunchKernelGGL(k_raster_mesh, dim3(min(per, B - f0) * bands), dim3(RZ_THREADS), 0, s, m, d_poses, d_cams, w, h, far, pixel_offset, f0, bands, rows, d_depth, d_body);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

extern "C" int ht_raster_mesh_depth(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, float far, float pixel_offset, int B, uint16_t *depth, int8_t *body)
{
	CHECK_READY(ctx);
	{ const int r = rz_check_args(ctx, poses, cams, depth, w, h, far, pixel_offset, B); if (r) return r; }
	if (B == 0) return HT_OK;
	return rc_render_sync(ctx, poses, cams, w, h, B, depth, body, [&](const float *d_poses, const float *d_cams, uint16_t *d_depth, int8_t *d_body, hipStream_t s)
	                      { return ht_raster_mesh_depth_dev(ctx, d_poses, d_cams, w, h, far, pixel_offset, B, d_depth, d_body, s); });
}
