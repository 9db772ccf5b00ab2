// ht_render.hip -- synthetic depth frames on the device: the application's software rasteriser FakeDepth for a batch of frames.
//
// Reference computations:
//   FakeDepth                      synthetic-hand-tracker/synthetic-tracker.cpp:69-76 (one HitCheck per pixel, the ray from the origin to deprojectz(p, 4.0))
//   PhysModel::HitCheck            include/physmodel.h:287-294 (every body in order, each starting from the impact the earlier ones left)
//   ConvexHitCheck                 third_party/geometric.h:275-302
// The host statement of the same arithmetic is ht_model_hitcheck (ht_model_host.hip); every expression below has its tree, so a frame is
// bit-identical to the host's (tests/test_gpu_render.py).
//
// Mapping: one block of four waves per 16 pixel tiles of one frame; one wave per 16x4 tile, one lane per pixel.
//   prologue  lane b < nb: body b's inverse pose, the ray origin in its frame (the same for every pixel) and its cull radius, into an LDS table
//   cull      lane b < nb tests body b's widened bounding sphere against the tile's frustum (four planes through the origin spanned by the
//             tile's corner rays); __ballot gives the wave-uniform set of bodies that can be hit.  A culled body is a provable miss for every
//             pixel of the tile, so skipping it leaves HitCheck's result unchanged (DESIGN section 17 has the argument).
//   hit loop  bodies of the set in ascending order (= the reference's order among the bodies that can change the result); per body the
//             hull planes in stored order with the reference's early exit.  The plane index is wave-uniform, so the plane arrives through a
//             scalar load (or from LDS in the HT_RENDER_LDS measurement build).
// A tile whose set is empty writes the far point's depth (most tiles of a 320x240 frame).
#include <limits.h>
#include <string.h>
#include "ht_device.hpp"
#include "ht_host.hpp"

#define RT_W 16                 // tile: 16 x 4 pixels per wave
#define RT_H 4
#define RT_THREADS 256
#define RT_TILES 16             // tiles per block (4 per wave)
#define RT_TAB 32               // floats per body-table entry

// pos 0..2 | invp 3..5 (= qrot(qconj(q), -pos)) | RI columns 6..14 (qmat(qconj(q))) | RF columns 15..23 (qmat(q)) | a0 24..26 (the origin in the body's frame) |
// 27 cull radius | 28 first plane | 29 number of planes (as integers)
struct rt_model
{
	const float4 *planes;
	int nb;
	int plane_off[HT_MAXNB + 1];
	float rad[HT_MAXNB];        // farthest vertex of the hull planes' polytope from the centre of mass
	float hin[HT_MAXNB];        // nearest hull plane from the centre of mass (<= 0: the body is never culled)
};

__device__ __forceinline__ v3 rt_to_local(const float *t, v3 w)      // pose.inverse() * w = apply(inverse(pose), w) (geometric.h:119,122)
{
	const v3 X = V3(t[6], t[7], t[8]), Y = V3(t[9], t[10], t[11]), Z = V3(t[12], t[13], t[14]);
	return V3(t[3], t[4], t[5]) + ((X * w.x + Y * w.y) + Z * w.z);
}
__device__ __forceinline__ v3 rt_to_world(const float *t, v3 v)      // pose * v = apply(pose, v)
{
	const v3 X = V3(t[15], t[16], t[17]), Y = V3(t[18], t[19], t[20]), Z = V3(t[21], t[22], t[23]);
	return V3(t[0], t[1], t[2]) + ((X * v.x + Y * v.y) + Z * v.z);
}
__device__ __forceinline__ v3 rt_dir(float x, float y, float fx, float fy, float px, float py) { return V3((x - px) / fx, (y - py) / fy, 1.0f); }

typedef const __attribute__((address_space(4))) float *rt_cptr;       // read-only for the kernel's lifetime: uniform reads become scalar loads

template <bool LDS_PLANES>
__global__ __launch_bounds__(RT_THREADS) void k_render_depth(const rt_model M, const float *__restrict__ poses, const float *__restrict__ cams, int w, int h, float F,
                                                             int f0, int groups, uint16_t *__restrict__ depth, int8_t *__restrict__ body)
{
	__shared__ float tab[HT_MAXNB * RT_TAB];
	extern __shared__ __attribute__((aligned(16))) float4 s_rt_planes[];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int frame = f0 + blockIdx.x / groups, g = blockIdx.x % groups;
	const int nb = M.nb;
	const float *cam = cams + (size_t)frame * HT_CAM;
	const float fx = cam[0], fy = cam[1], px = cam[2], py = cam[3], ds = cam[4];
	if (LDS_PLANES) { const int np = M.plane_off[nb]; for (int i = t; i < np; i += RT_THREADS) s_rt_planes[i] = M.planes[i]; }
	if (t < nb)
	{
		const float *p = poses + ((size_t)frame * nb + t) * HT_POSE;
		const v3 pos = V3(p[0], p[1], p[2]); const v4 q = V4(p[3], p[4], p[5], p[6]);
		const v4 qc = qconj(q);
		const v3 invp = qrot(qc, -pos);
		const m3 ri = qmat(qc), rf = qmat(q);
		float *e = tab + t * RT_TAB;
		e[0] = pos.x; e[1] = pos.y; e[2] = pos.z; e[3] = invp.x; e[4] = invp.y; e[5] = invp.z;
		e[6] = ri.x.x; e[7] = ri.x.y; e[8] = ri.x.z; e[9] = ri.y.x; e[10] = ri.y.y; e[11] = ri.y.z; e[12] = ri.z.x; e[13] = ri.z.y; e[14] = ri.z.z;
		e[15] = rf.x.x; e[16] = rf.x.y; e[17] = rf.x.z; e[18] = rf.y.x; e[19] = rf.y.y; e[20] = rf.y.z; e[21] = rf.z.x; e[22] = rf.z.y; e[23] = rf.z.z;
		const v3 a0 = rt_to_local(e, V3(0.0f, 0.0f, 0.0f));
		e[24] = a0.x; e[25] = a0.y; e[26] = a0.z;
		// cull radius: every point ConvexHitCheck computes lies within tau of the segment and within tau of every plane's half-space, with
		// tau <= (4 n + 32) u L, L = the largest coordinate magnitude on the way (the farthest image corner's far point plus the body's distance
		// from the origin); doubled for safety.  DESIGN section 17.
		float L = 0.0f;
		for (int k = 0; k < 4; k++)
		{
			const float cx = (k & 1) ? (float)(w - 1) : 0.0f, cy = (k & 2) ? (float)(h - 1) : 0.0f;
			L = fmaxf(L, length(rt_dir(cx, cy, fx, fy, px, py) * F));
		}
		L += length(pos);
		const int n = M.plane_off[t + 1] - M.plane_off[t];
		const float tau = 2.0f * (float)(4 * n + 32) * 5.9604645e-8f * L;
		const float r = M.rad[t], hi = M.hin[t];
		e[27] = hi > 0.0f && isfinite(L) ? (r * (1.0f + tau / hi) * 1.0001f + tau) : INFINITY;
		e[28] = __int_as_float(M.plane_off[t]); e[29] = __int_as_float(n);
	}
	__syncthreads();
	const int txn = (w + RT_W - 1) / RT_W, ntiles = txn * ((h + RT_H - 1) / RT_H);
	for (int i = wave; i < RT_TILES; i += RT_THREADS / 64)
	{
		const int tile = g * RT_TILES + i;
		if (tile >= ntiles) break;
		const int x0 = (tile % txn) * RT_W, y0 = (tile / txn) * RT_H;
		const int x = x0 + (lane & (RT_W - 1)), y = y0 + lane / RT_W;
		const bool valid = x < w && y < h;
		// ---- cull: lane b tests body b's sphere against the tile's four side planes ----
		bool keep = false;
		if (lane < nb)
		{
			const float xa = (float)x0, xb = (float)min(x0 + RT_W - 1, w - 1), ya = (float)y0, yb = (float)min(y0 + RT_H - 1, h - 1);
			const v3 c[4] = { rt_dir(xa, ya, fx, fy, px, py), rt_dir(xb, ya, fx, fy, px, py), rt_dir(xb, yb, fx, fy, px, py), rt_dir(xa, yb, fx, fy, px, py) };
			const v3 mid = rt_dir(0.5f * (xa + xb), 0.5f * (ya + yb), fx, fy, px, py);
			const float *e = tab + lane * RT_TAB;
			const v3 C = V3(e[0], e[1], e[2]);
			const float R = e[27];
			keep = true;
#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				v3 nrm = cross(c[k], c[(k + 1) & 3]);
				const float nl = length(nrm);
				if (!(nl > 0.0f)) continue;      // a tile one pixel wide or tall: that side is no plane
				if (dot(nrm, mid) < 0.0f) nrm = -nrm;
				if (dot(nrm, C) < -R * nl) keep = false;
			}
		}
		unsigned long long mask = __ballot(keep);
		// ---- HitCheck(origin, far) over the bodies that can be hit ----
		const v3 far = V3(((float)x - px) / fx * F, ((float)y - py) / fy * F, F);      // deprojectz(float2(x, y), F), misc_image.h:48
		v3 impact = far;
		int who = -1;
		while (mask)
		{
			const int b = __ffsll((long long)mask) - 1;
			mask &= mask - 1ull;
			const float *e = tab + b * RT_TAB;
			const int p0 = __builtin_amdgcn_readfirstlane(__float_as_int(e[28])), np = __builtin_amdgcn_readfirstlane(__float_as_int(e[29]));
			v3 a = V3(e[24], e[25], e[26]), c = rt_to_local(e, impact);
			bool live = valid, hit = valid;
			const rt_cptr P = (rt_cptr)(const float *)(M.planes + p0);
			for (int k = 0; k < np; k++)      // ConvexHitCheck geometric.h:275-297
			{
				const float4 pl = LDS_PLANES ? s_rt_planes[p0 + k] : make_float4(P[4 * k], P[4 * k + 1], P[4 * k + 2], P[4 * k + 3]);
				if (live)
				{
					const v4 plane = V4(pl.x, pl.y, pl.z, pl.w);
					const float d0 = dot_plane(plane, a), d1 = dot_plane(plane, c);
					if (d0 >= 0 && d1 >= 0) { hit = false; live = false; }
					else if (!(d0 <= 0 && d1 <= 0))
					{
						const v3 xp = a + ((c - a) * d0) / (d0 - d1);
						if (d0 >= 0) a = xp; else c = xp;
					}
				}
				if (__ballot(live) == 0ull) break;
			}
			if (hit) { impact = rt_to_world(e, a); who = b; }
		}
		if (valid)
		{
			const size_t o = ((size_t)frame * h + y) * w + x;
			depth[o] = (unsigned short)(impact.z / ds);
			if (body) body[o] = (int8_t)who;
		}
	}
}

// Per-body radii of the context's current model (after ht_scale), from the hull planes themselves (the collision vertices are not the planes' polytope:
// the planes may lie outside them): the farthest vertex of the polytope {x : dot_plane(p, x) <= 0 for every plane p} from the centre of mass, by
// enumerating the feasible intersections of three planes in double, and the nearest plane.  Derived once per model state (about 50 ms for the hand).
static void rt_fill_model(ht_ctx *ctx, rt_model &m)
{
	memset(&m, 0, sizeof m);
	m.planes = ctx->model.planes; m.nb = ctx->model.nb;
	for (int b = 0; b <= m.nb; b++) m.plane_off[b] = ctx->model.plane_off[b];
	const std::vector<float4> &P = ctx->h_planes;
	const bool same = ctx->render_planes.size() == P.size() && ctx->render_radii.size() == 2 * (size_t)m.nb && (P.empty() || !memcmp(ctx->render_planes.data(), P.data(), P.size() * sizeof(float4)));
	if (!same)
	{
		ctx->render_radii.assign(2 * (size_t)m.nb, 0.0f);
		for (int b = 0; b < m.nb; b++)
		{
			const int p0 = m.plane_off[b], n = m.plane_off[b + 1] - p0;
			std::vector<double> pl((size_t)4 * n);
			double hmin = INFINITY;
			for (int i = 0; i < n; i++)
			{
				const float4 &q = P[(size_t)p0 + i];
				const double nl = sqrt((double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z);
				pl[4 * i] = q.x; pl[4 * i + 1] = q.y; pl[4 * i + 2] = q.z; pl[4 * i + 3] = q.w;
				hmin = fmin(hmin, (nl > 0.0 && fabs(nl - 1.0) <= 1e-5) ? -(double)q.w / nl : -1.0);      // the tolerance argument takes unit normals: a body with others is never culled
			}
			double r = 0.0; int nvert = 0;
			for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++) for (int k = j + 1; k < n; k++)
			{
				const double *A = &pl[4 * i], *B = &pl[4 * j], *Cc = &pl[4 * k];
				const double cx = B[1] * Cc[2] - B[2] * Cc[1], cy = B[2] * Cc[0] - B[0] * Cc[2], cz = B[0] * Cc[1] - B[1] * Cc[0];      // B x C
				const double det = A[0] * cx + A[1] * cy + A[2] * cz;
				if (fabs(det) < 1e-12) continue;
				// x = (-a.w (B x C) - b.w (C x A) - c.w (A x B)) / det
				const double ax = Cc[1] * A[2] - Cc[2] * A[1], ay = Cc[2] * A[0] - Cc[0] * A[2], az = Cc[0] * A[1] - Cc[1] * A[0];
				const double bx = A[1] * B[2] - A[2] * B[1], by = A[2] * B[0] - A[0] * B[2], bz = A[0] * B[1] - A[1] * B[0];
				const double x = -(A[3] * cx + B[3] * ax + Cc[3] * bx) / det, y = -(A[3] * cy + B[3] * ay + Cc[3] * by) / det, z = -(A[3] * cz + B[3] * az + Cc[3] * bz) / det;
				const double d2 = x * x + y * y + z * z;
				if (d2 <= r * r) continue;
				bool in = true;
				for (int l = 0; l < n && in; l++) in = pl[4 * l] * x + pl[4 * l + 1] * y + pl[4 * l + 2] * z + pl[4 * l + 3] <= 1e-7;
				if (in) { r = sqrt(d2); nvert++; }
			}
			const bool ok = nvert > 0 && hmin > 0.0 && hmin < INFINITY;
			ctx->render_radii[2 * b] = ok ? (float)(r * (1.0 + 1e-4) + 1e-6) : INFINITY;
			ctx->render_radii[2 * b + 1] = ok ? (float)(hmin * (1.0 - 1e-6)) : -1.0f;
		}
		ctx->render_planes = P;
	}
	for (int b = 0; b < m.nb; b++) { m.rad[b] = ctx->render_radii[2 * b]; m.hin[b] = ctx->render_radii[2 * b + 1]; }
}

static int rt_check_args(ht_ctx *ctx, const void *poses, const void *cams, const void *depth, int w, int h, float far, int B)
{
	if (!poses || !cams || !depth || w < 1 || h < 1 || w > 4096 || h > 4096 || !(far > 0.0f) || B < 0) { ctx->err = "ht_render_depth: bad argument"; return HT_ERR_ARG; }
	if (ctx->cnn_only) { ctx->err = "this context was created without a hand model (CNN only)"; return HT_ERR_STATE; }
	return HT_OK;
}

extern "C" int ht_render_depth_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int w, int h, float far, int B, uint16_t *d_depth, int8_t *d_body, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = rt_check_args(ctx, d_poses, d_cams, d_depth, w, h, far, B); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	rt_model m; rt_fill_model(ctx, m);
	const int ntiles = ((w + RT_W - 1) / RT_W) * ((h + RT_H - 1) / RT_H), groups = (ntiles + RT_TILES - 1) / RT_TILES;
	const bool lds = ht_tuning_int("HT_RENDER_LDS", 0) != 0;      // measurement builds only: the planes from LDS instead of scalar loads
	const size_t shm = lds ? (size_t)m.plane_off[m.nb] * sizeof(float4) : 0;
	const int per = INT_MAX / groups;      // frames per launch (grid size limit)
	for (int f0 = 0; f0 < B; f0 += per)
	{
		const int n = min(per, B - f0);
		if (lds) hipLaunchKernelGGL(k_render_depth<true>, dim3(n * groups), dim3(RT_THREADS), shm, s, m, d_poses, d_cams, w, h, far, f0, groups, d_depth, d_body);
		else hipLaunchKernelGGL(k_render_depth<false>, dim3(n * groups), dim3(RT_THREADS), 0, s, m, d_poses, d_cams, w, h, far, f0, groups, d_depth, d_body);
	}
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

// the synchronous variant stages through one device buffer of its own, grown to the largest call (the renderer uses no tracker slot: B is not bounded by max_batch)
extern "C" int ht_render_depth(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, float far, int B, uint16_t *depth, int8_t *body)
{
	CHECK_READY(ctx);
	{ const int r = rt_check_args(ctx, poses, cams, depth, w, h, far, B); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t nb = (size_t)ctx->model.nb, npx = (size_t)B * w * h;
	const size_t o_cams = ((size_t)B * nb * HT_POSE * sizeof(float) + 255) & ~(size_t)255, o_depth = (o_cams + (size_t)B * HT_CAM * sizeof(float) + 255) & ~(size_t)255;
	const size_t o_body = (o_depth + npx * sizeof(uint16_t) + 255) & ~(size_t)255, bytes = o_body + (body ? npx : 0);
	{ const int r = dev_grow(ctx, &ctx->d_render, &ctx->render_cap, bytes); if (r) return r; }
	char *base = ctx->d_render;
	float *d_poses = (float *)base, *d_cams = (float *)(base + o_cams);
	uint16_t *d_depth = (uint16_t *)(base + o_depth); int8_t *d_body = body ? (int8_t *)(base + o_body) : nullptr;
	hipStream_t s = ctx->stream;
	HIPCHK(ctx, hipMemcpyAsync(d_poses, poses, (size_t)B * nb * HT_POSE * sizeof(float), hipMemcpyHostToDevice, s));
	HIPCHK(ctx, hipMemcpyAsync(d_cams, cams, (size_t)B * HT_CAM * sizeof(float), hipMemcpyHostToDevice, s));
	{ const int r = ht_render_depth_dev(ctx, d_poses, d_cams, w, h, far, B, d_depth, d_body, s); if (r) return r; }
	HIPCHK(ctx, hipMemcpyAsync(depth, d_depth, npx * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
	if (body) HIPCHK(ctx, hipMemcpyAsync(body, d_body, npx, hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipStreamSynchronize(s));
	return HT_OK;
}
