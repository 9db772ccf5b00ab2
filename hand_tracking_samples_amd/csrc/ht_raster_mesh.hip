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
#include "ht_raster_band.hpp"

// pixel (x, y) of the band (row y0 first) against triangle `key16`
__device__ __forceinline__ void rz_pixel(unsigned *zb, const rz_tri &T, int x, int y, int y0, int w, float fx, float fy, float px, float py, float off, float F, float ds, unsigned key16)
{
	if (!rz_inside(T, x, y)) return;
	const int n = rz_count(T, rz_ray(x, off, px, fx), rz_ray(y, off, py, fy), F, ds);
	if (n >= 0) atomicMin(&zb[(y - y0) * w + x], ((unsigned)n << 16) | key16);
}

__global__ __launch_bounds__(RZ_THREADS) void k_raster_mesh(const rz_model M, const float *__restrict__ poses, const float *__restrict__ cams, int w, int h, float F, float off,
                                                            int f0, int bands, int rows, uint16_t *__restrict__ depth, int8_t *__restrict__ body)
{
	__shared__ uint4 zb4[RZ_PIX / 4];
	__shared__ float tab[HT_MAXNB * 12];
	unsigned *zb = (unsigned *)zb4;
	const int t = threadIdx.x, lane = t & 63;
	const int frame = f0 + blockIdx.x / bands, band = blockIdx.x % bands;
	const int y0 = band * rows, y1 = min(h, y0 + rows) - 1, npx = (y1 - y0 + 1) * w;      // npx <= RZ_PIX (rz_band_rows)
	const int nb = M.nb;
	const float *cam = cams + (size_t)frame * HT_CAM;
	const float fx = cam[0], fy = cam[1], px = cam[2], py = cam[3], ds = cam[4];
	for (int i = t; i < (npx + 3) / 4; i += RZ_THREADS) zb4[i] = make_uint4(RZ_NONE, RZ_NONE, RZ_NONE, RZ_NONE);
	if (t < nb)
	{
		const float *p = poses + ((size_t)frame * nb + t) * HT_POSE;
		const m3 R = qmat(V4(p[3], p[4], p[5], p[6]));
		const v3 up = V3(p[0], p[1], p[2]) - mul(R, V3(M.com[3 * t], M.com[3 * t + 1], M.com[3 * t + 2]));
		float *e = tab + t * 12;
		e[0] = R.x.x; e[1] = R.x.y; e[2] = R.x.z; e[3] = R.y.x; e[4] = R.y.y; e[5] = R.y.z; e[6] = R.z.x; e[7] = R.z.y; e[8] = R.z.z; e[9] = up.x; e[10] = up.y; e[11] = up.z;
	}
	__syncthreads();
	for (int base = 0; base < M.ntri; base += RZ_THREADS)      // uniform over the block: the wave's ballots and shuffles below see every lane
	{
		const int k = base + t;
		rz_tri T = {};
		int x0 = 0, x1 = -1, ya = 0, yb = -1;
		bool live = k < M.ntri;
		if (live)
		{
			const float *e = tab + rz_body_of(M, k) * 12;
			m3 R; R.x = V3(e[0], e[1], e[2]); R.y = V3(e[3], e[4], e[5]); R.z = V3(e[6], e[7], e[8]);
			const float4 *row = M.rows + 4 * (size_t)k;
			const float4 q0 = row[0], q1 = row[1], q2 = row[2];
			live = rz_setup(R, V3(e[9], e[10], e[11]), V3(q0.x, q0.y, q0.z), V3(q1.x, q1.y, q1.z), V3(q2.x, q2.y, q2.z), fx, fy, px, py, off, T);
			if (live)
			{
				rz_rect(T, x0, x1, ya, yb);
				x0 = max(x0, 0); x1 = min(x1, w - 1); ya = max(ya, y0); yb = min(yb, y1);
				live = x0 <= x1 && ya <= yb;
			}
		}
		const bool big = live && (x1 - x0 + 1) * (yb - ya + 1) >= RZ_BIG;      // at most 4096 * 4096: fits
		if (live && !big)
			for (int y = ya; y <= yb; y++) for (int x = x0; x <= x1; x++) rz_pixel(zb, T, x, y, y0, w, fx, fy, px, py, off, F, ds, (unsigned)k);
		unsigned long long bm = __ballot(big);
		while (bm)
		{
			const int j = __ffsll((long long)bm) - 1;
			bm &= bm - 1ull;
			rz_tri S;
			S.X[0] = __shfl(T.X[0], j); S.X[1] = __shfl(T.X[1], j); S.X[2] = __shfl(T.X[2], j);
			S.Y[0] = __shfl(T.Y[0], j); S.Y[1] = __shfl(T.Y[1], j); S.Y[2] = __shfl(T.Y[2], j);
			S.N.x = __shfl(T.N.x, j); S.N.y = __shfl(T.N.y, j); S.N.z = __shfl(T.N.z, j); S.k = __shfl(T.k, j);
			const int sx0 = __shfl(x0, j), sx1 = __shfl(x1, j), sya = __shfl(ya, j), syb = __shfl(yb, j);
			const unsigned key16 = (unsigned)(k - lane + j);
			for (int y = sya; y <= syb; y++) for (int x = sx0 + lane; x <= sx1; x += 64) rz_pixel(zb, S, x, y, y0, w, fx, fy, px, py, off, F, ds, key16);
		}
	}
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
			*(uint2 *)(depth + 4 * g) = make_uint2((unsigned)d[0] | ((unsigned)d[1] << 16), (unsigned)d[2] | ((unsigned)d[3] << 16));
			if (body) *(unsigned *)(body + 4 * g) = (unsigned)(who[0] & 0xff) | ((unsigned)(who[1] & 0xff) << 8) | ((unsigned)(who[2] & 0xff) << 16) | ((unsigned)(who[3] & 0xff) << 24);
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
