// ht_raster_band.hpp -- what the two z-buffer kernels share on the device (k_raster_mesh, ht_raster_mesh.hip; k_raster_scene, ht_raster_scene.hip): the band of
// rows a block owns, the model as a kernel argument and the body of a triangle.
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

// the model of a context as the kernels take it
static inline rz_model rz_model_of(const ht_ctx *ctx)
{
	rz_model m;
	memset(&m, 0, sizeof m);
	m.rows = ctx->d_mesh; m.nb = ctx->model.nb;
	ht_mesh_args(ctx, m.com, m.tri_off); m.ntri = m.tri_off[m.nb];
	return m;
}
