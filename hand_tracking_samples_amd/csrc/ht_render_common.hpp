// ht_render_common.hpp -- the frame the two depth renderers stand in (ht_render.hip: the hulls, ht_render_mesh.hip: the subdivision meshes): the tile
// mapping, the per-body LDS table of poses, the ray and frame helpers, the pixel store, the launch loop and the synchronous entries' staging.
// What a kernel does with a tile (the hulls' sphere cull and ConvexHitCheck, the meshes' triangle rejection and PolyHitCheck) stays in its file.
//
// Mapping: one block of four waves per 16 pixel tiles of one frame; one wave per 16x4 tile, one lane per pixel.
#pragma once
#include <limits.h>
#include "ht_device.hpp"
#include "ht_host.hpp"

#define RC_W 16                 // tile: 16 x 4 pixels per wave
#define RC_H 4
#define RC_THREADS 256
#define RC_TILES 16             // tiles per block (4 per wave)
#define RC_TAB 32               // floats per body-table entry

// Body-table entry, the frame {p, q} of body b (the hulls: the centre-of-mass pose; the meshes: the mesh pose U_b):
// p 0..2 | invp 3..5 (= qrot(qconj(q), -p)) | RI columns 6..14 (qmat(qconj(q))) | RF columns 15..23 (qmat(q)) | a0 24..26 (the origin in the body's frame) |
// 28 first row | 29 number of rows (hull planes or triangles, as integers).  Slots 27 and 30 belong to the kernel that writes them (named there); 31 is unused.
#define RC_A0 24
#define RC_ROW0 28
#define RC_NROWS 29

typedef const __attribute__((address_space(4))) float *rc_cptr;       // read-only for the kernel's lifetime: uniform reads become scalar loads

__device__ __forceinline__ v3 rc_to_local(const float *t, v3 w)      // pose.inverse() * w = apply(inverse(pose), w) (geometric.h:119,122)
{
	const v3 X = V3(t[6], t[7], t[8]), Y = V3(t[9], t[10], t[11]), Z = V3(t[12], t[13], t[14]);
	return V3(t[3], t[4], t[5]) + ((X * w.x + Y * w.y) + Z * w.z);
}
__device__ __forceinline__ v3 rc_to_world(const float *t, v3 v)      // pose * v = apply(pose, v)
{
	const v3 X = V3(t[15], t[16], t[17]), Y = V3(t[18], t[19], t[20]), Z = V3(t[21], t[22], t[23]);
	return V3(t[0], t[1], t[2]) + ((X * v.x + Y * v.y) + Z * v.z);
}
__device__ __forceinline__ v3 rc_dir(float x, float y, float fx, float fy, float px, float py) { return V3((x - px) / fx, (y - py) / fy, 1.0f); }
__device__ __forceinline__ v3 rc_far(float x, float y, float fx, float fy, float px, float py, float F) { return V3((x - px) / fx * F, (y - py) / fy * F, F); }      // deprojectz(float2(x, y), F), misc_image.h:48

// slots 0..26 of entry e from the frame's position and orientation
__device__ __forceinline__ void rc_fill_frame(float *e, v3 p, v4 q)
{
	const v4 qc = qconj(q);
	const v3 invp = qrot(qc, -p);
	const m3 ri = qmat(qc), rf = qmat(q);
	e[0] = p.x; e[1] = p.y; e[2] = p.z; e[3] = invp.x; e[4] = invp.y; e[5] = invp.z;
	e[6] = ri.x.x; e[7] = ri.x.y; e[8] = ri.x.z; e[9] = ri.y.x; e[10] = ri.y.y; e[11] = ri.y.z; e[12] = ri.z.x; e[13] = ri.z.y; e[14] = ri.z.z;
	e[15] = rf.x.x; e[16] = rf.x.y; e[17] = rf.x.z; e[18] = rf.y.x; e[19] = rf.y.y; e[20] = rf.y.z; e[21] = rf.z.x; e[22] = rf.z.y; e[23] = rf.z.z;
	const v3 a0 = rc_to_local(e, V3(0.0f, 0.0f, 0.0f));
	e[RC_A0] = a0.x; e[RC_A0 + 1] = a0.y; e[RC_A0 + 2] = a0.z;
}

// The largest |far point| over the image's four corner pixels, sampled at pixel + off: it bounds the magnitude of every point on a ray of the frame.
// One expression serves both kernels bit for bit.  The hulls pass off = 0: x + 0.0f is x in float for the non-negative pixel coordinates here, and
// their earlier dir * F had the far point's three floats, 1.0f * F being F.
__device__ __forceinline__ float rc_corner_bound(int w, int h, float off, float fx, float fy, float px, float py, float F)
{
	float L = 0.0f;
	for (int k = 0; k < 4; k++)
	{
		const float cx = ((k & 1) ? (float)(w - 1) : 0.0f) + off, cy = ((k & 2) ? (float)(h - 1) : 0.0f) + off;
		L = fmaxf(L, length(rc_far(cx, cy, fx, fy, px, py, F)));
	}
	return L;
}

__host__ __device__ __forceinline__ int rc_tiles_across(int w) { return (w + RC_W - 1) / RC_W; }
__host__ __device__ __forceinline__ int rc_ntiles(int w, int h) { return rc_tiles_across(w) * ((h + RC_H - 1) / RC_H); }

struct rc_tile
{
	int x0, y0, x, y;           // the tile's first pixel, this lane's pixel
	bool valid;                 // the lane's pixel lies inside the frame
	float xa, xb, ya, yb;       // the tile's corner samples, clipped to the frame, at pixel + off
};
// tile number `tile` (< rc_ntiles(w, h)) of a w x h frame, as lane `lane` of its wave sees it
__device__ __forceinline__ rc_tile rc_tile_decode(int tile, int lane, int w, int h, float off)
{
	const int txn = rc_tiles_across(w);
	rc_tile T;
	T.x0 = (tile % txn) * RC_W; T.y0 = (tile / txn) * RC_H;
	T.x = T.x0 + (lane & (RC_W - 1)); T.y = T.y0 + lane / RC_W;
	T.valid = T.x < w && T.y < h;
	T.xa = (float)T.x0 + off; T.xb = (float)min(T.x0 + RC_W - 1, w - 1) + off; T.ya = (float)T.y0 + off; T.yb = (float)min(T.y0 + RC_H - 1, h - 1) + off;
	return T;
}

// a valid lane's pixel: the impact's depth in the camera's units, and the body that was hit (-1: none) where the caller asked for labels
__device__ __forceinline__ void rc_store_pixel(uint16_t *__restrict__ depth, int8_t *__restrict__ body, int frame, int w, int h, const rc_tile &T, float z, float ds, int who)
{
	const size_t o = ((size_t)frame * h + T.y) * w + T.x;
	depth[o] = (unsigned short)(z / ds);
	if (body) body[o] = (int8_t)who;
}

// ---- host ----

// launch(blocks, f0, groups) over the B frames of w x h pixels, as many frames per launch as the grid size limit allows
template <class F> static inline void rc_launch_frames(int w, int h, int B, F launch)
{
	const int groups = (rc_ntiles(w, h) + RC_TILES - 1) / RC_TILES;
	const int per = INT_MAX / groups;      // frames per launch (grid size limit)
	for (int f0 = 0; f0 < B; f0 += per) launch(min(per, B - f0) * groups, f0, groups);
}

// the checks both entries of a renderer share; off_ok: the mesh renderer's pixel offset lies in [0, 1]
static inline int rc_check_args(ht_ctx *ctx, const char *name, const void *poses, const void *cams, const void *depth, int w, int h, float far, int B, bool off_ok = true)
{
	if (!poses || !cams || !depth || !ht_frame_dims_ok(w, h) || !(far > 0.0f) || !off_ok || B < 0) { ctx->err = std::string(name) + ": bad argument"; return HT_ERR_ARG; }
	CHECK_MODEL(ctx);
	return HT_OK;
}

// A renderer's synchronous entry: poses, cameras, frames and labels staged through the context's buffer (ht_staged_call; the renderers use no tracker slot, so B
// is not bounded by max_batch).  dev(d_poses, d_cams, d_depth, d_body, stream) is its _dev entry.
template <class F> static inline int rc_render_sync(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, int B, uint16_t *depth, int8_t *body, F dev)
{
	const size_t nb = (size_t)ctx->model.nb, npx = (size_t)B * w * h;
	ht_seg seg[4] = { { (void *)poses, (size_t)B * nb * HT_POSE * sizeof(float), false }, { (void *)cams, (size_t)B * HT_CAM * sizeof(float), false },
	                  { depth, npx * sizeof(uint16_t), true }, { body, npx, true } };
	return ht_staged_call(ctx, seg, 4, [&](hipStream_t s) { return dev((const float *)seg[0].dev, (const float *)seg[1].dev, (uint16_t *)seg[2].dev, (int8_t *)seg[3].dev, s); });
}
