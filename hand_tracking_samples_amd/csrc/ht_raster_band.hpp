// ht_raster_band.hpp -- what the two z-buffer kernels share on the device (k_raster_mesh, ht_raster_mesh.hip; k_raster_scene, ht_raster_scene.hip): the band of
// rows a block owns, the model as a kernel argument, the body of a triangle, a body's entry of the block's pose table, the pixel test, the pass over the model's
// triangles (set-up, clip to the band, lane walk and wave walk) and the write-out's two packers.  Each kernel keeps its own write-out loop.
#pragma once
#include <string.h>
#include "ht_render_common.hpp"
#include "ht_raster.hpp"

#define RZ_THREADS 256
#define RZ_PIX 19200            // pixels of a band's z-buffer: 76800 bytes of LDS, two blocks per CU (320 x 60, 640 x 30, 4096 x 4)
#define RZ_BIG 64               // rectangles of this many pixels or more are walked by the wave
#define RZ_NONE 0xffffffffu

struct rz_model
{
	const float4 *rows;         // [t][4]: p0 p1 p2 plane (the plane is not read here)
	int nb, ntri;
	int tri_off[HT_MAXNB + 1];
	float com[HT_MAXNB * 3];
};

__host__ __device__ __forceinline__ int rz_band_rows(int w, int h)      // rows per band: as few bands as fit RZ_PIX, of equal height
{
	const int most = RZ_PIX / w, bands = (h + most - 1) / most;
	return (h + bands - 1) / bands;
}

__device__ __forceinline__ int rz_body_of(const rz_model &M, int k)
{
	int b = 0;
	for (int i = 1; i < M.nb; i++) b += k >= M.tri_off[i] ? 1 : 0;
	return b;
}

// A body's entry of the block's pose table, twelve floats: R = qmat(q) and up = pos - R com, from the body's 7-float pose p (a left instance's: the mirrored one)
__device__ __forceinline__ void rz_table_put(float *e, const float *p, const float *com)
{
	const m3 R = qmat(V4(p[3], p[4], p[5], p[6]));
	const v3 up = V3(p[0], p[1], p[2]) - mul(R, V3(com[0], com[1], com[2]));
	e[0] = R.x.x; e[1] = R.x.y; e[2] = R.x.z; e[3] = R.y.x; e[4] = R.y.y; e[5] = R.y.z; e[6] = R.z.x; e[7] = R.z.y; e[8] = R.z.z; e[9] = up.x; e[10] = up.y; e[11] = up.z;
}
__device__ __forceinline__ void rz_table_get(const float *e, m3 &R, v3 &up) { R.x = V3(e[0], e[1], e[2]); R.y = V3(e[3], e[4], e[5]); R.z = V3(e[6], e[7], e[8]); up = V3(e[9], e[10], e[11]); }

// pixel (x, y) of a layer against triangle `key16`, written at column `rz_scene_column` of the band (row y0 first); left == false: the layer's own column
__device__ __forceinline__ void rz_pixel(unsigned *zb, const rz_tri &T, int x, int y, int y0, int w, bool left, float fx, float fy, float px, float py, float off, float F, float ds, unsigned key16)
{
	if (!rz_inside(T, x, y)) return;
	const int n = rz_count(T, rz_ray(x, off, px, fx), rz_ray(y, off, py, fy), F, ds);
	if (n >= 0) atomicMin(&zb[(y - y0) * w + rz_scene_column(x, w, left)], ((unsigned)n << 16) | key16);
}

// The model's triangles at the poses of `tab` into the band's z-buffer (rows y0 .. y1), with keys count << 16 | key0 + triangle.  Thread t takes triangles t, t + 256, ...:
// corners from the mesh rows, set-up, its pixel rectangle (in the layer's columns; the band's rows are the layer's rows) clipped to the band; a small rectangle is walked
// by the lane alone, one of RZ_BIG pixels or more by the whole wave, one column per lane.  Every thread of the block calls this, with the same key0 and left.
__device__ __forceinline__ void rz_triangles(unsigned *zb, const rz_model &M, const float *tab, int t, int y0, int y1, int w, bool left, float fx, float fy, float px, float py, float off, float F, float ds,
                                             unsigned key0)
{
	const int lane = t & 63;
	for (int base = 0; base < M.ntri; base += RZ_THREADS)      // uniform over the block: the wave's ballots and shuffles below see every lane
	{
		const int k = base + t;
		rz_tri T = {};
		int x0 = 0, x1 = -1, ya = 0, yb = -1;
		bool live = k < M.ntri;
		if (live)
		{
			m3 R; v3 up;
			rz_table_get(tab + rz_body_of(M, k) * 12, R, up);
			const float4 *row = M.rows + 4 * (size_t)k;
			const float4 q0 = row[0], q1 = row[1], q2 = row[2];
			live = rz_setup(R, up, V3(q0.x, q0.y, q0.z), V3(q1.x, q1.y, q1.z), V3(q2.x, q2.y, q2.z), fx, fy, px, py, off, T);
			if (live)
			{
				rz_rect(T, x0, x1, ya, yb);
				x0 = max(x0, 0); x1 = min(x1, w - 1); ya = max(ya, y0); yb = min(yb, y1);
				live = x0 <= x1 && ya <= yb;
			}
		}
		const bool big = live && (x1 - x0 + 1) * (yb - ya + 1) >= RZ_BIG;      // at most 4096 * 4096: fits
		if (live && !big)
			for (int y = ya; y <= yb; y++) for (int x = x0; x <= x1; x++) rz_pixel(zb, T, x, y, y0, w, left, fx, fy, px, py, off, F, ds, key0 + (unsigned)k);
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
			const unsigned key16 = key0 + (unsigned)(k - lane + j);
			for (int y = sya; y <= syb; y++) for (int x = sx0 + lane; x <= sx1; x += 64) rz_pixel(zb, S, x, y, y0, w, left, fx, fy, px, py, off, F, ds, key16);
		}
	}
}

// the write-out's packers: four pixels' counts as one 8-byte store, four labels (-1 = none) as one 4-byte store
__device__ __forceinline__ uint2 rz_pack_u16(const unsigned short *d) { return make_uint2((unsigned)d[0] | ((unsigned)d[1] << 16), (unsigned)d[2] | ((unsigned)d[3] << 16)); }
__device__ __forceinline__ unsigned rz_pack_i8(const int *v) { return (unsigned)(v[0] & 0xff) | ((unsigned)(v[1] & 0xff) << 8) | ((unsigned)(v[2] & 0xff) << 16) | ((unsigned)(v[3] & 0xff) << 24); }

// the model of a context as the kernels take it
static inline rz_model rz_model_of(const ht_ctx *ctx)
{
	rz_model m;
	memset(&m, 0, sizeof m);
	m.rows = ctx->d_mesh; m.nb = ctx->model.nb;
	ht_mesh_args(ctx, m.com, m.tri_off); m.ntri = m.tri_off[m.nb];
	return m;
}
