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
// Mapping: ht_render.hip's.  One block of four waves per 16 tiles of one frame; one wave per 16x4 tile, one lane per pixel.
//   prologue  lane b < nb: the mesh pose U_b = {pos - qrot(q, com), q}, its inverse and the ray origin in its frame, into an LDS table
//   triangles per body (all of them: a bound of a whole body is not exact, see below), 64 triangles at a time, lane j tests triangle j against the TILE: front face (d0 > 0, which no pixel changes),
//             the far points of the tile's four corner rays all in front of the plane, or all four corner rays outside one edge's plane.  d1 and the
//             determinants are affine in the pixel, so their extremes over the tile are at its corners (DESIGN section 19 has the margins).
//             __ballot gives the triangles that can be a candidate for some pixel.
//   pixels    those triangles in stored order with wave-uniform indices (corners and plane arrive as scalar loads): PolyHitCheck per lane.
#include <limits.h>
#include <string.h>
#include "ht_device.hpp"
#include "ht_host.hpp"
#include "ht_model_build.hpp"

#define RM_W 16                 // tile: 16 x 4 pixels per wave
#define RM_H 4
#define RM_THREADS 256
#define RM_TILES 16             // tiles per block (4 per wave)
#define RM_TAB 32               // floats per body-table entry
#define RM_U 5.9604645e-8f      // 2^-24

// U.p 0..2 | invp 3..5 (= qrot(qconj(q), -U.p)) | RI columns 6..14 (qmat(qconj(q))) | RF columns 15..23 (qmat(q)) | a0 24..26 (the origin in the mesh's frame) |
// 27 unused | 28 first triangle | 29 number of triangles (as integers) | 30 magnitude bound of the margins
struct rm_model
{
	const float4 *rows;         // [t][4]: p0 p1 p2 plane
	int nb;
	int tri_off[HT_MAXNB + 1];
	float rad[HT_MAXNB];        // farthest mesh corner from the centre of mass
	float com[HT_MAXNB * 3];
};

__device__ __forceinline__ v3 rm_to_local(const float *t, v3 w)      // U.inverse() * w = apply(inverse(U), w) (geometric.h:119,122)
{
	const v3 X = V3(t[6], t[7], t[8]), Y = V3(t[9], t[10], t[11]), Z = V3(t[12], t[13], t[14]);
	return V3(t[3], t[4], t[5]) + ((X * w.x + Y * w.y) + Z * w.z);
}
__device__ __forceinline__ v3 rm_to_world(const float *t, v3 v)      // U * v = apply(U, v)
{
	const v3 X = V3(t[15], t[16], t[17]), Y = V3(t[18], t[19], t[20]), Z = V3(t[21], t[22], t[23]);
	return V3(t[0], t[1], t[2]) + ((X * v.x + Y * v.y) + Z * v.z);
}
__device__ __forceinline__ v3 rm_dir(float x, float y, float fx, float fy, float px, float py) { return V3((x - px) / fx, (y - py) / fy, 1.0f); }
__device__ __forceinline__ v3 rm_far(float x, float y, float fx, float fy, float px, float py, float F) { return V3((x - px) / fx * F, (y - py) / fy * F, F); }      // deprojectz(float2(x, y), F)
__device__ __forceinline__ v3 rm_v3(float4 q) { return V3(q.x, q.y, q.z); }

typedef const __attribute__((address_space(4))) float *rm_cptr;       // read-only for the kernel's lifetime: uniform reads become scalar loads

__global__ __launch_bounds__(RM_THREADS) void k_render_mesh(const rm_model M, const float *__restrict__ poses, const float *__restrict__ cams, int w, int h, float F, float off,
                                                            int f0, int groups, uint16_t *__restrict__ depth, int8_t *__restrict__ body)
{
	__shared__ float tab[HT_MAXNB * RM_TAB];
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
		const v4 qc = qconj(q);
		const v3 invp = qrot(qc, -up);
		const m3 ri = qmat(qc), rf = qmat(q);
		float *e = tab + t * RM_TAB;
		e[0] = up.x; e[1] = up.y; e[2] = up.z; e[3] = invp.x; e[4] = invp.y; e[5] = invp.z;
		e[6] = ri.x.x; e[7] = ri.x.y; e[8] = ri.x.z; e[9] = ri.y.x; e[10] = ri.y.y; e[11] = ri.y.z; e[12] = ri.z.x; e[13] = ri.z.y; e[14] = ri.z.z;
		e[15] = rf.x.x; e[16] = rf.x.y; e[17] = rf.x.z; e[18] = rf.y.x; e[19] = rf.y.y; e[20] = rf.y.z; e[21] = rf.z.x; e[22] = rf.z.y; e[23] = rf.z.z;
		const v3 a0 = rm_to_local(e, V3(0.0f, 0.0f, 0.0f));
		e[24] = a0.x; e[25] = a0.y; e[26] = a0.z;
		// Lb bounds the magnitude of every point and difference the triangle tests form: the farthest image corner's far point, the mesh frame's distance
		// from the origin, the mesh's extent.  The margins of the tile tests are multiples of u Lb.
		float L = 0.0f;
		for (int k = 0; k < 4; k++)
		{
			const float cx = ((k & 1) ? (float)(w - 1) : 0.0f) + off, cy = ((k & 2) ? (float)(h - 1) : 0.0f) + off;
			L = fmaxf(L, length(rm_far(cx, cy, fx, fy, px, py, F)));
		}
		const float r = M.rad[t];
		const float Lb = (L + length(up)) + (length(com) + r);
		e[30] = Lb;
		e[28] = __int_as_float(M.tri_off[t]); e[29] = __int_as_float(M.tri_off[t + 1] - M.tri_off[t]);
	}
	__syncthreads();
	const int txn = (w + RM_W - 1) / RM_W, ntiles = txn * ((h + RM_H - 1) / RM_H);
	for (int i = wave; i < RM_TILES; i += RM_THREADS / 64)
	{
		const int tile = g * RM_TILES + i;
		if (tile >= ntiles) break;
		const int x0 = (tile % txn) * RM_W, y0 = (tile / txn) * RM_H;
		const int x = x0 + (lane & (RM_W - 1)), y = y0 + lane / RM_W;
		const bool valid = x < w && y < h;
		const float xa = (float)x0 + off, xb = (float)min(x0 + RM_W - 1, w - 1) + off, ya = (float)y0 + off, yb = (float)min(y0 + RM_H - 1, h - 1) + off;
		// Every body goes to the triangle tests: no bound of a body is exact here.  The float determinants of a triangle seen nearly edge-on pass for rays far from it
		// (a stray pixel of the definition, 0.45 m from a hand at 2.6 m in tests/test_gpu_render_mesh.py), so a sphere about the mesh drops candidates the host keeps.
		unsigned long long mask = nb >= 64 ? ~0ull : (1ull << nb) - 1ull;
		const v3 far = rm_far((float)x + off, (float)y + off, fx, fy, px, py, F);
		float best = INFINITY;
		int bb = -1, bk = -1;
		while (mask)
		{
			const int b = __ffsll((long long)mask) - 1;
			mask &= mask - 1ull;
			const float *e = tab + b * RM_TAB;
			const int t0 = __builtin_amdgcn_readfirstlane(__float_as_int(e[28])), nt = __builtin_amdgcn_readfirstlane(__float_as_int(e[29]));
			const float Lb = e[30];
			const v3 a = V3(e[24], e[25], e[26]), c = rm_to_local(e, far), D = c - a;
			// the tile's corner rays in the mesh's frame: far points and directions (the pixel's own expressions at the corner pixels)
			v3 cc[4], cd[4];
#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				cc[k] = rm_to_local(e, rm_far((k == 1 || k == 2) ? xb : xa, (k >= 2) ? yb : ya, fx, fy, px, py, F));
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
					const rm_cptr S = (rm_cptr)(const float *)(M.rows + 4 * (size_t)(t0 + k));
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
				const float *e = tab + bb * RM_TAB;
				const float4 pl = M.rows[4 * (size_t)(__float_as_int(e[28]) + bk) + 3];
				const v4 plane = V4(pl.x, pl.y, pl.z, pl.w);
				const v3 a = V3(e[24], e[25], e[26]), c = rm_to_local(e, far);
				const float d0 = dot_plane(plane, a), d1 = dot_plane(plane, c);
				impact = rm_to_world(e, a + ((c - a) * d0) / (d0 - d1));
			}
			const size_t o = ((size_t)frame * h + y) * w + x;
			depth[o] = (unsigned short)(impact.z / ds);
			if (body) body[o] = (int8_t)bb;
		}
	}
}

// rows and radii of the context's current meshes (after ht_scale): called by the model loader and by ht_scale, which have waited for the renders in flight
int ht_mesh_upload(ht_ctx *ctx)
{
	const int nb = ctx->model.nb;
	const size_t nt = ctx->h_mesh_corners.size() / 9;
	ctx->mesh_rad.assign((size_t)nb, 0.0f);
	if (!nt) return HT_OK;
	std::vector<float> rows(nt * 16);
	ht_mesh_rows(ctx->h_mesh_corners.data(), nt, rows.data());
	for (int b = 0; b < nb; b++)
	{
		const float *com = &ctx->h_bodyc[(size_t)b * HT_BC + HT_BC_COM];
		double r2 = 0.0;
		for (int k = ctx->mesh_off[b]; k < ctx->mesh_off[b + 1]; k++) for (int i = 0; i < 3; i++)
		{
			const float *p = &ctx->h_mesh_corners[(size_t)9 * k + 3 * i];
			const double dx = (double)p[0] - com[0], dy = (double)p[1] - com[1], dz = (double)p[2] - com[2];
			r2 = fmax(r2, dx * dx + dy * dy + dz * dz);
		}
		ctx->mesh_rad[b] = (float)(sqrt(r2) * (1.0 + 1e-6) + 1e-7);
	}
	if (!ctx->d_mesh) { const int r = dev_alloc(ctx, &ctx->d_mesh, nt * 4); if (r) return r; }
	HIPCHK(ctx, hipMemcpy(ctx->d_mesh, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
	return HT_OK;
}

static int rm_check_args(ht_ctx *ctx, const void *poses, const void *cams, const void *depth, int w, int h, float far, float off, int B)
{
	if (!poses || !cams || !depth || w < 1 || h < 1 || w > 4096 || h > 4096 || !(far > 0.0f) || !(off >= 0.0f && off <= 1.0f) || B < 0) { ctx->err = "ht_render_mesh_depth: bad argument"; return HT_ERR_ARG; }
	if (ctx->cnn_only) { ctx->err = "this context was created without a hand model (CNN only)"; return HT_ERR_STATE; }
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
	for (int b = 0; b <= m.nb; b++) m.tri_off[b] = ctx->mesh_off[b];
	for (int b = 0; b < m.nb; b++) { m.rad[b] = ctx->mesh_rad[b]; for (int i = 0; i < 3; i++) m.com[3 * b + i] = ctx->h_bodyc[(size_t)b * HT_BC + HT_BC_COM + i]; }
	const int ntiles = ((w + RM_W - 1) / RM_W) * ((h + RM_H - 1) / RM_H), groups = (ntiles + RM_TILES - 1) / RM_TILES;
	const int per = INT_MAX / groups;      // frames per launch (grid size limit)
	for (int f0 = 0; f0 < B; f0 += per)
	{
		const int n = min(per, B - f0);
		hipLaunchKernelGGL(k_render_mesh, dim3(n * groups), dim3(RM_THREADS), 0, s, m, d_poses, d_cams, w, h, far, pixel_offset, f0, groups, d_depth, d_body);
	}
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

// the synchronous variant stages through ht_render_depth's buffer (both are synchronous on the context's stream; B is not bounded by max_batch)
extern "C" int ht_render_mesh_depth(ht_ctx *ctx, const float *poses, const float *cams, int w, int h, float far, float pixel_offset, int B, uint16_t *depth, int8_t *body)
{
	CHECK_READY(ctx);
	{ const int r = rm_check_args(ctx, poses, cams, depth, w, h, far, pixel_offset, B); if (r) return r; }
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
	{ const int r = ht_render_mesh_depth_dev(ctx, d_poses, d_cams, w, h, far, pixel_offset, B, d_depth, d_body, s); if (r) return r; }
	HIPCHK(ctx, hipMemcpyAsync(depth, d_depth, npx * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
	if (body) HIPCHK(ctx, hipMemcpyAsync(body, d_body, npx, hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipStreamSynchronize(s));
	return HT_OK;
}
