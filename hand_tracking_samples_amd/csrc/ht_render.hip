// ht_render.hip -- synthetic depth frames on the device: the application's software rasteriser FakeDepth for a batch of frames.
//
// Reference computations:
//   FakeDepth                      synthetic-hand-tracker/synthetic-tracker.cpp:69-76 (one HitCheck per pixel, the ray from the origin to deprojectz(p, 4.0))
//   PhysModel::HitCheck            include/physmodel.h:287-294 (every body in order, each starting from the impact the earlier ones left)
//   ConvexHitCheck                 third_party/geometric.h:275-302
// The host statement of the same arithmetic is ht_model_hitcheck (ht_model_host.hip); every expression below has its tree, so a frame is
// bit-identical to the host's (tests/test_gpu_render.py).
//
// Mapping: ht_render_common.hpp's (one wave per 16x4 tile, one lane per pixel; the body table of poses in LDS).
//   prologue  lane b < nb: body b's frame at its centre-of-mass pose and its cull radius into the table
//   cull      lane b < nb tests body b's widened bounding sphere against the tile's frustum (four planes through the origin spanned by the
//             tile's corner rays); __ballot gives the wave-uniform set of bodies that can be hit.  A culled body is a provable miss for every
//             pixel of the tile, so skipping it leaves HitCheck's result unchanged (DESIGN section 17 has the argument).
//   hit loop  bodies of the set in ascending order (= the reference's order among the bodies that can change the result); per body the
//             hull planes in stored order with the reference's early exit.  The plane index is wave-uniform, so the plane arrives through a
//             scalar load.
// A tile whose set is empty writes the far point's depth (most tiles of a 320x240 frame).
#include <string.h>
#include "ht_render_common.hpp"

#define RT_CULL 27              // table slot: the body's cull radius

struct rt_model
{
	const float4 *planes;
	int nb;
	int plane_off[HT_MAXNB + 1];
	float rad[HT_MAXNB];        // farthest vertex of the hull planes' polytope from the centre of mass
	float hin[HT_MAXNB];        // nearest hull plane from the centre of mass (<= 0: the body is never culled)
};

__global__ __launch_bounds__(RC_THREADS) void k_render_depth(const rt_model M, const float *__restrict__ poses, const float *__restrict__ cams, int w, int h, float F,
                                                             int f0, int groups, uint16_t *__restrict__ depth, int8_t *__restrict__ body)
{
	__shared__ float tab[HT_MAXNB * RC_TAB];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int frame = f0 + blockIdx.x / groups, g = blockIdx.x % groups;
	const int nb = M.nb;
	const float *cam = cams + (size_t)frame * HT_CAM;
	const float fx = cam[0], fy = cam[1], px = cam[2], py = cam[3], ds = cam[4];
	if (t < nb)
	{
		const float *p = poses + ((size_t)frame * nb + t) * HT_POSE;
		const v3 pos = V3(p[0], p[1], p[2]); const v4 q = V4(p[3], p[4], p[5], p[6]);
		float *e = tab + t * RC_TAB;
		rc_fill_frame(e, pos, q);
		// cull radius: every point ConvexHitCheck computes lies within tau of the segment and within tau of every plane's half-space, with
		// tau <= (4 n + 32) u L, L = the largest coordinate magnitude on the way (the farthest image corner's far point plus the body's distance
		// from the origin); doubled for safety.  DESIGN section 17.
		const float L = rc_corner_bound(w, h, 0.0f, fx, fy, px, py, F) + length(pos);
		const int n = M.plane_off[t + 1] - M.plane_off[t];
		const float tau = 2.0f * (float)(4 * n + 32) * 5.9604645e-8f * L;
		const float r = M.rad[t], hi = M.hin[t];
		e[RT_CULL] = hi > 0.0f && isfinite(L) ? (r * (1.0f + tau / hi) * 1.0001f + tau) : INFINITY;
		e[RC_ROW0] = __int_as_float(M.plane_off[t]); e[RC_NROWS] = __int_as_float(n);
	}
	__syncthreads();
	const int ntiles = rc_ntiles(w, h);
	for (int i = wave; i < RC_TILES; i += RC_THREADS / 64)
	{
		const int tile = g * RC_TILES + i;
		if (tile >= ntiles) break;
		const rc_tile T = rc_tile_decode(tile, lane, w, h, 0.0f);
		const bool valid = T.valid;
		// ---- cull: lane b tests body b's sphere against the tile's four side planes ----
		bool keep = false;
		if (lane < nb)
		{
			const float xa = T.xa, xb = T.xb, ya = T.ya, yb = T.yb;
			const v3 c[4] = { rc_dir(xa, ya, fx, fy, px, py), rc_dir(xb, ya, fx, fy, px, py), rc_dir(xb, yb, fx, fy, px, py), rc_dir(xa, yb, fx, fy, px, py) };
			const v3 mid = rc_dir(0.5f * (xa + xb), 0.5f * (ya + yb), fx, fy, px, py);
			const float *e = tab + lane * RC_TAB;
			const v3 C = V3(e[0], e[1], e[2]);
			const float R = e[RT_CULL];
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
		const v3 far = rc_far((float)T.x, (float)T.y, fx, fy, px, py, F);
		v3 impact = far;
		int who = -1;
		while (mask)
		{
			const int b = __ffsll((long long)mask) - 1;
			mask &= mask - 1ull;
			const float *e = tab + b * RC_TAB;
			const int p0 = __builtin_amdgcn_readfirstlane(__float_as_int(e[RC_ROW0])), np = __builtin_amdgcn_readfirstlane(__float_as_int(e[RC_NROWS]));
			v3 a = V3(e[RC_A0], e[RC_A0 + 1], e[RC_A0 + 2]), c = rc_to_local(e, impact);
			bool live = valid, hit = valid;
			const rc_cptr P = (rc_cptr)(const float *)(M.planes + p0);
			for (int k = 0; k < np; k++)      // ConvexHitCheck geometric.h:275-297
			{
				const v4 plane = V4(P[4 * k], P[4 * k + 1], P[4 * k + 2], P[4 * k + 3]);
				if (live)
				{
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
			if (hit) { impact = rc_to_world(e, a); who = b; }
		}
		if (valid) rc_store_pixel(depth, body, frame, w, h, T, impact.z, ds, who);
	}
}

// Per-body radii of the context's current model (after ht_scale), from the hull planes themselves (the collision vertices are not the planes' polytope:
// the planes may lie outside them): the farthest vertex of the polytope {x : dot_plane(p, x) <= 0 for every plane p} from the centre of mass, by
// enumerating the feasible intersections of three planes in double, and the nearest plane.  Derived once per model state (about 50 ms for the hand): again when
// the record's generation has moved (ht_scale).
static void rt_fill_model(ht_ctx *ctx, rt_model &m)
{
	memset(&m, 0, sizeof m);
	m.planes = ctx->model.planes; m.nb = ctx->model.nb;
	for (int b = 0; b <= m.nb; b++) m.plane_off[b] = ctx->model.plane_off[b];
	if (ctx->render_radii.size() != 2 * (size_t)m.nb || ctx->render_gen != ctx->rec.gen)
	{
		std::vector<float4> P(ctx->rec.planes.size() / 4);      // the record's planes, for the time of the derivation
		if (!P.empty()) memcpy(P.data(), ctx->rec.planes.data(), P.size() * sizeof(float4));
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
		ctx->render_gen = ctx->rec.gen;
	}
	for (int b = 0; b < m.nb; b++) { m.rad[b] = ctx->render_radii[2 * b]; m.hin[b] = ctx->render_radii[2 * b + 1]; }
}

extern "C" int ht_render_depth_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int w, int h, float far, int B, uint16_t *d_depth, int8_t *d_body, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = rc_check_args(ctx, "ht_render_depth", d_poses, d_cams, d_depth, w, h, far, B); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	rt_model m; rt_fill_model(ctx, m);
	rc_launch_frames(w, h, B, [&](int blocks, int f0, int groups) { hipLaunchKernelGGL(k_render_depth, dim3(blocks), dim3(RC_THREADS), 0, s, m, d_poses, d_cams, w, h, far, f0, groups, d_depth, d_body); });
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

extern "C" int ht_render_depth(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, float far, int B, uint16_t *depth, int8_t *body)
{
	CHECK_READY(ctx);
	{ const int r = rc_check_args(ctx, "ht_render_depth", poses, cams, depth, w, h, far, B); if (r) return r; }
	if (B == 0) return HT_OK;
	return rc_render_sync(ctx, poses, cams, w, h, B, depth, body, [&](const float *d_poses, const float *d_cams, uint16_t *d_depth, int8_t *d_body, hipStream_t s)
	                      { return ht_render_depth_dev(ctx, d_poses, d_cams, w, h, far, B, d_depth, d_body, s); });
}
