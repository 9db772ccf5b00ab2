// ht_render_mesh.hip -- synthetic depth frames of the hand's subdivision surface on the device: the software statement of the application's default
// depth source (the fake hand's sdmeshes drawn and read back, synthetic-tracker.cpp:164-165) for a batch of frames.
//
// Reference computations:
//   PhysModel::GetMeshes(true)     include/physmodel.h:295-303 (sdmeshes[b] at Pose{PositionUser, orientation})
//   PolyHitCheck / PolyPlane       third_party/geometric.h:247-273 (front faces only, the winding test on the whole segment)
//   deprojectz                     include/misc_image.h:48
// The definition is the host's ht_model_render_mesh (ht_model_host.hip): every triangle of every body against the whole segment, the smallest
// d0 / (d0 - d1) wins, the first in (body, triangle) order on a tie.  Every expression below has the host's tree, so a frame is bit-identical to it
// (tests/test_gpu_render_mesh.py).
//
// Mapping: ht_render_common.hpp's (one wave per 16x4 tile, one lane per pixel; the body table of poses in LDS).
//   prologue  lane b < nb: the frame of the mesh pose U_b = {pos - qrot(q, com), q} and the margins' magnitude bound into the table
//   triangles per body (all of them: a bound of a whole body is not exact, see below), 64 triangles at a time, lane j tests triangle j against the TILE: front face (d0 > 0, which no pixel changes),
//             the far points of the tile's four corner rays all in front of the plane, or all four corner rays outside one edge's plane.  d1 and the
//             determinants are affine in the pixel, so their extremes over the tile are at its corners (DESIGN section 19 has the margins).
//             __ballot gives the triangles that can be a candidate for some pixel.
//   pixels    those triangles in stored order with wave-uniform indices (corners and plane arrive as scalar loads): PolyHitCheck per lane.
#include <string.h>
#include "ht_render_common.hpp"
#include "ht_model_build.hpp"

#define RM_LB 30                // table slot: the magnitude bound of the margins
#define RM_U 5.9604645e-8f      // 2^-24

struct rm_model
{
	const float4 *rows;         // [t][4]: p0 p1 p2 plane
	int nb;
	int tri_off[HT_MAXNB + 1];
	float rad[HT_MAXNB];        // farthest mesh corner from the centre of mass
	float com[HT_MAXNB * 3];
};

__device__ __forceinline__ v3 rm_v3(float4 q) { return V3(q.x, q.y, q.z); }

__global__ __launch_bounds__(RC_THREADS) void k_render_mesh(const rm_model M, const float *__restrict__ poses, const float *__restrict__ cams, int w, int h, float F, float off,
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
		const v4 q = V4(p[3], p[4], p[5], p[6]);
		const v3 pos = V3(p[0], p[1], p[2]), com = V3(M.com[3 * t], M.com[3 * t + 1], M.com[3 * t + 2]);
		const v3 up = pos - qrot(q, com);
		float *e = tab + t * RC_TAB;
		rc_fill_frame(e, up, q);
		// Lb bounds the magnitude of every point and difference the triangle tests form: the farthest image corner's far point, the mesh frame's distance
		// from the origin, the mesh's extent.  The margins of the tile tests are multiples of u Lb.
		const float L = rc_corner_bound(w, h, off, fx, fy, px, py, F);
		const float r = M.rad[t];
		const float Lb = (L + length(up)) + (length(com) + r);
		e[RM_LB] = Lb;
		e[RC_ROW0] = __int_as_float(M.tri_off[t]); e[RC_NROWS] = __int_as_float(M.tri_off[t + 1] - M.tri_off[t]);
	}
	__syncthreads();
	const int ntiles = rc_ntiles(w, h);
	for (int i = wave; i < RC_TILES; i += RC_THREADS / 64)
	{
		const int tile = g * RC_TILES + i;
		if (tile >= ntiles) break;
		const rc_tile T = rc_tile_decode(tile, lane, w, h, off);
		const bool valid = T.valid;
		// Every body goes to the triangle tests: no bound of a body is exact here.  The float determinants of a triangle seen nearly edge-on pass for rays far from it
		// (a stray pixel of the definition, 0.45 m from a hand at 2.6 m in tests/test_gpu_render_mesh.py), so a sphere about the mesh drops candidates the host keeps.
		unsigned long long mask = nb >= 64 ? ~0ull : (1ull << nb) - 1ull;
		const v3 far = rc_far((float)T.x + off, (float)T.y + off, fx, fy, px, py, F);
		float best = INFINITY;
		int bb = -1, bk = -1;
		while (mask)
		{
			const int b = __ffsll((long long)mask) - 1;
			mask &= mask - 1ull;
			const float *e = tab + b * RC_TAB;
			const int t0 = __builtin_amdgcn_readfirstlane(__float_as_int(e[RC_ROW0])), nt = __builtin_amdgcn_readfirstlane(__float_as_int(e[RC_NROWS]));
			const float Lb = e[RM_LB];
			const v3 a = V3(e[RC_A0], e[RC_A0 + 1], e[RC_A0 + 2]), c = rc_to_local(e, far), D = c - a;
			// the tile's corner rays in the mesh's frame: far points and directions (the pixel's own expressions at the corner pixels)
			v3 cc[4], cd[4];
#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				cc[k] = rc_to_local(e, rc_far((k == 1 || k == 2) ? T.xb : T.xa, (k >= 2) ? T.yb : T.ya, fx, fy, px, py, F));
				cd[k] = cc[k] - a;
			}
			for (int j0 = 0; j0 < nt; j0 += 64)
			{
				// ---- triangles against the tile: lane j takes triangle j0 + j ----
				const int kk = min(j0 + lane, nt - 1);
				const float4 *row = M.rows + 4 * (size_t)(t0 + kk);
				const float4 q0 = row[0], q1 = row[1], q2 = row[2], pl = row[3];
				const v4 P = V4(pl.x, pl.y, pl.z, pl.w);
				bool live = j0 + lane < nt && dot_plane(P, a) > 0;      // the definition's d0, bit for bit: the same for every pixel
				{
					const float md = 128.0f * RM_U * (Lb + fabsf(P.w));
					bool front = true;      // every corner's far point in front of the plane by the margin: d1 < 0 at no pixel
#pragma unroll
					for (int k = 0; k < 4; k++) front = front && dot_plane(P, cc[k]) >= md;
					if (front) live = false;
				}
				const v3 A[3] = { rm_v3(q0) - a, rm_v3(q1) - a, rm_v3(q2) - a };
				const float len[3] = { length(A[0]), length(A[1]), length(A[2]) };
#pragma unroll
				for (int s = 0; s < 3; s++)
				{
					const int s1 = (s + 1) % 3;
					const v3 n = cross(A[s1], A[s]);      // determinant(A[s1], A[s], d) = dot(d, n)
					const float me = 256.0f * RM_U * (len[s1] * len[s]) * Lb;
					bool out = true;        // every corner ray outside this edge's plane by the margin: the determinant is < 0 at every pixel
#pragma unroll
					for (int k = 0; k < 4; k++) out = out && dot(n, cd[k]) < -me;
					if (out) live = false;
				}
				unsigned long long tm = __ballot(live);
				// ---- PolyHitCheck per pixel, the surviving triangles in stored order ----
				while (tm)
				{
					const int j = __ffsll((long long)tm) - 1;
					tm &= tm - 1ull;
					const int k = j0 + j;
					const rc_cptr S = (rc_cptr)(const float *)(M.rows + 4 * (size_t)(t0 + k));
					const v4 plane = V4(S[12], S[13], S[14], S[15]);
					const float d0 = dot_plane(plane, a), d1 = dot_plane(plane, c);
					bool hit = valid && d0 > 0 && d1 < 0;
					if (__ballot(hit) == 0ull) continue;
					const v3 p0 = V3(S[0], S[1], S[2]), p1 = V3(S[4], S[5], S[6]), p2 = V3(S[8], S[9], S[10]);
					const v3 e0 = p0 - a, e1 = p1 - a, e2 = p2 - a;
					{ m3 m; m.x = e1; m.y = e0; m.z = D; hit = hit && determinant(m) >= 0; }
					if (__ballot(hit) == 0ull) continue;
					{ m3 m; m.x = e2; m.y = e1; m.z = D; hit = hit && determinant(m) >= 0; }
					if (__ballot(hit) == 0ull) continue;
					{ m3 m; m.x = e0; m.y = e2; m.z = D; hit = hit && determinant(m) >= 0; }
					if (__ballot(hit) == 0ull) continue;
					const float tt = d0 / (d0 - d1);
					if (hit && tt < best) { best = tt; bb = b; bk = k; }
				}
			}
		}
		if (valid)
		{
			v3 impact = far;
			if (bb >= 0)      // the winner's impact, PolyHitCheck's own expression from the same d0 and d1
			{
				const float *e = tab + bb * RC_TAB;
				const float4 pl = M.rows[4 * (size_t)(__float_as_int(e[RC_ROW0]) + bk) + 3];
				const v4 plane = V4(pl.x, pl.y, pl.z, pl.w);
				const v3 a = V3(e[RC_A0], e[RC_A0 + 1], e[RC_A0 + 2]), c = rc_to_local(e, far);
				const float d0 = dot_plane(plane, a), d1 = dot_plane(plane, c);
				impact = rc_to_world(e, a + ((c - a) * d0) / (d0 - d1));
			}
			rc_store_pixel(depth, body, frame, w, h, T, impact.z, ds, bb);
		}
	}
}

// rows and radii of the context's current meshes (after ht_scale): called by the model loader and by ht_scale, which have waited for the renders in flight
int ht_mesh_upload(ht_ctx *ctx)
{
	const ht_model_rec &rec = ctx->rec;
	const int nb = ctx->model.nb; const size_t nt = rec.corners.size() / 9;
	ctx->mesh_rad.assign((size_t)nb, 0.0f);
	if (!nt) return HT_OK;
	for (int b = 0; b < nb; b++)
	{
		const float *com = &rec.bodyc[(size_t)b * HT_BC + HT_BC_COM];
		double r2 = 0.0;
		for (int k = rec.mesh_off[b]; k < rec.mesh_off[b + 1]; k++) for (int i = 0; i < 3; i++)
		{
			const float *p = &rec.corners[(size_t)9 * k + 3 * i];
			const double dx = (double)p[0] - com[0], dy = (double)p[1] - com[1], dz = (double)p[2] - com[2];
			r2 = fmax(r2, dx * dx + dy * dy + dz * dz);
		}
		ctx->mesh_rad[b] = (float)(sqrt(r2) * (1.0 + 1e-6) + 1e-7);
	}
	if (!ctx->d_mesh) { const int r = dev_alloc(ctx, &ctx->d_mesh, nt * 4); if (r) return r; }
	HIPCHK(ctx, hipMemcpy(ctx->d_mesh, rec.rows.data(), rec.rows.size() * sizeof(float), hipMemcpyHostToDevice));
	return HT_OK;
}

static int rm_check_args(ht_ctx *ctx, const void *poses, const void *cams, const void *depth, int w, int h, float far, float off, int B)
{
	{ const int r = rc_check_args(ctx, "ht_render_mesh_depth", poses, cams, depth, w, h, far, B, off >= 0.0f && off <= 1.0f); if (r) return r; }
	if (!ctx->d_mesh) { ctx->err = "the model file holds no subdivision meshes (bake it again)"; return HT_ERR_STATE; }
	return HT_OK;
}

extern "C" int ht_render_mesh_depth_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int w, int h, float far, float pixel_offset, int B, uint16_t *d_depth, int8_t *d_body, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = rm_check_args(ctx, d_poses, d_cams, d_depth, w, h, far, pixel_offset, B); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	rm_model m;
	memset(&m, 0, sizeof m);
	m.rows = ctx->d_mesh; m.nb = ctx->model.nb;
	ht_mesh_args(ctx, m.com, m.tri_off);
	for (int b = 0; b < m.nb; b++) m.rad[b] = ctx->mesh_rad[b];
	rc_launch_frames(w, h, B, [&](int blocks, int f0, int groups) { hipLaunchKernelGGL(k_render_mesh, dim3(blocks), dim3(RC_THREADS), 0, s, m, d_poses, d_cams, w, h, far, pixel_offset, f0, groups, d_depth, d_body); });
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

extern "C" int ht_render_mesh_depth(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, float far, float pixel_offset, int B, uint16_t *depth, int8_t *body)
{
	CHECK_READY(ctx);
	{ const int r = rm_check_args(ctx, poses, cams, depth, w, h, far, pixel_offset, B); if (r) return r; }
	if (B == 0) return HT_OK;
	return rc_render_sync(ctx, poses, cams, w, h, B, depth, body, [&](const float *d_poses, const float *d_cams, uint16_t *d_depth, int8_t *d_body, hipStream_t s)
	                      { return ht_render_mesh_depth_dev(ctx, d_poses, d_cams, w, h, far, pixel_offset, B, d_depth, d_body, s); });
}
