// ht_joints.hip -- the hand's own coordinates: joint read-out, forward kinematics and a seeded pose sampler (an addition).
//
// Reference computations:
//   ConstrainAngularRangeW         third_party/physics.h:351-393 (the swing / twist decomposition of a joint, the y <-> z swap of :358-362, what each axis is limited to)
//   quat_from_to                   third_party/geometric.h:319-328
//   FixPositions                   include/physmodel.h:404-408 (PositionUser1 = PoseUser0 * p0 - q1 * p1), GetLinearConstraints :328-334 (the gap it closes)
//   RigidBody::PositionUser        third_party/physics.h:142
// For joint j (parent rbi0 at q0, child rbi1 at q1, jointframe F): Jb = q0 F, Jf = q1, both times cb = normalize(0,-1,0,1) when the joint is swapped;
// r = conj(Jb) Jf, s = quat_from_to((0,0,1), qzdir(r)), t = conj(s) r; the coordinates are c = (s.x, s.y, t.z) -- no sign canonicalisation, as in the reference.
// The other way: s = (cx, cy, 0, sqrt(max(0, 1 - cx cx - cy cy))), t = (0, 0, cz, sqrt(max(0, 1 - cz cz))), q1 = normalize(q0 F [cb] s t [conj(cb)]).
//
// Mapping.  These kernels are launch- and latency-bound (a frame is about 16 joints x 100 flops); nothing here is tuned.
//   k_joint_coords   one thread per (frame, joint); the joint table, the limits' swap flags and the centres of mass once per block into LDS.  The two poses of a joint are
//                    read straight from global memory: the 64 lanes of a wave cover about four frames, whose 28-byte records are contiguous, so every line fetched is
//                    used whole by the wave and nothing would be gained by staging them.
//   k_joint_pose /   one thread per frame walks the joints in model order.  A thread's poses live in its row of an LDS table [64][nb * 7 | 1] (an odd stride: the 32 lanes
//   k_sample_poses   of an LDS access group fall on 32 banks): the walk indexes the table by the parent's number, which registers cannot do without a private array in
//                    scratch, and the block then copies the table out in whole lines -- lane by lane the records would lie nb * 28 bytes apart.  The coordinates take
//                    the same way through a second table, in (k_joint_pose) or out (k_sample_poses, when asked for).
// Every expression is fp32 with one rounding per operation in the written order (the library is built without contraction; division and sqrtf are correctly
// rounded), so the results equal tests/joints_ref.py bit for bit.
#include <string.h>
#include <math.h>
#include "ht_host.hpp"
#include "ht_mix.hpp"

#define JT_THREADS 64
#define JC_THREADS 256

struct jt_tables { const float *jc, *jl, *com; };      // in LDS: [nj][HT_JC], [nj][HT_JL], [nb][3]
__device__ __forceinline__ int jt_table_floats(int nb, int nj) { return nj * (HT_JC + HT_JL) + nb * 3; }
__device__ __forceinline__ jt_tables jt_load_tables(float *lds, const ht_model_dev &M, const float *__restrict__ jl, int nthreads)
{
	const int nb = M.nb, nj = M.nj;
	float *a = lds, *b = a + nj * HT_JC, *c = b + nj * HT_JL;
	for (int i = threadIdx.x; i < nj * HT_JC; i += nthreads) a[i] = M.jointc[i];
	for (int i = threadIdx.x; i < nj * HT_JL; i += nthreads) b[i] = jl[i];
	for (int i = threadIdx.x; i < nb * 3; i += nthreads) c[i] = M.bodyc[(i / 3) * HT_BC + HT_BC_COM + (i % 3)];
	jt_tables t; t.jc = a; t.jl = b; t.com = c;
	return t;
}
__device__ __forceinline__ v4 jt_cb() { return normalize(V4(0, -1, 0, 1)); }

// c = (s.x, s.y, t.z) of a joint, physics.h:358-365
__device__ __forceinline__ v3 jt_coords(v4 q0, v4 q1, v4 F, bool swapped)
{
	v4 Jb = qmul(q0, F), Jf = q1;
	if (swapped) { const v4 cb = jt_cb(); Jb = qmul(Jb, cb); Jf = qmul(Jf, cb); }
	const v4 r = qmul(qconj(Jb), Jf);
	const v4 s = quat_from_to(V3(0, 0, 1.0f), qzdir(r));
	const v4 t = qmul(qconj(s), r);
	return V3(s.x, s.y, t.z);
}
// the child's orientation from the parent's and the joint's coordinates (out-of-range coordinates clamp to a unit quaternion's)
__device__ __forceinline__ v4 jt_child(v4 q0, v4 F, bool swapped, v3 c)
{
	const v4 s = V4(c.x, c.y, 0.0f, sqrtf(fmax_std(0.0f, (1.0f - c.x * c.x) - c.y * c.y)));
	const v4 t = V4(0.0f, 0.0f, c.z, sqrtf(fmax_std(0.0f, 1.0f - c.z * c.z)));
	v4 q = qmul(q0, F);
	if (swapped) q = qmul(q, jt_cb());
	q = qmul(qmul(q, s), t);
	if (swapped) q = qmul(q, qconj(jt_cb()));
	return normalize(q);
}

__global__ __launch_bounds__(JC_THREADS) void k_joint_coords(const ht_model_dev M, const float *__restrict__ jl, const float *__restrict__ poses, long long n, int com_poses,
                                                             float *__restrict__ coords, float *__restrict__ gaps)
{
	extern __shared__ float jt_lds[];
	const jt_tables T = jt_load_tables(jt_lds, M, jl, JC_THREADS);
	__syncthreads();
	const long long idx = (long long)blockIdx.x * JC_THREADS + threadIdx.x;
	if (idx >= n) return;
	const int nb = M.nb, nj = M.nj;
	const long long f = idx / nj; const int j = (int)(idx - f * nj);
	const float *jc = T.jc + j * HT_JC;
	const int rb0 = (int)jc[HT_JC_RB0], rb1 = (int)jc[HT_JC_RB1];
	const float *a = poses + ((size_t)f * nb + rb0) * HT_POSE, *b = poses + ((size_t)f * nb + rb1) * HT_POSE;
	const v4 q0 = load4(a + 3), q1 = load4(b + 3);
	const v3 c = jt_coords(q0, q1, load4(jc + HT_JC_FRAME), T.jl[j * HT_JL + HT_JL_SWAPPED] != 0.0f);
	coords[idx * 3] = c.x; coords[idx * 3 + 1] = c.y; coords[idx * 3 + 2] = c.z;
	if (gaps)
	{
		v3 u0 = load3(a), u1 = load3(b);
		if (com_poses) { u0 = u0 + qrot(q0, -load3(T.com + rb0 * 3)); u1 = u1 + qrot(q1, -load3(T.com + rb1 * 3)); }      // PositionUser physics.h:142
		gaps[idx] = length((u0 + qrot(q0, load3(jc + HT_JC_P0))) - (u1 + qrot(q1, load3(jc + HT_JC_P1))));
	}
}

// ---- the sampler's uniform numbers: a counter-based hash of (seed, sample, joint, axis), the top 24 bits of the second mix (ht_mix.hpp) -------------------------------
HT_HD float jt_uniform(unsigned long long seed, unsigned long long sample, int joint, int axis)
{
	const unsigned long long h = ht_mix64(ht_mix64(seed ^ (sample * 0x9E3779B97F4A7C15ull)) ^ ((unsigned long long)(joint * 3 + axis + 1) * 0xD6E8FEB86659FD93ull));
	return (float)(unsigned)(h >> 40) * 5.9604644775390625e-8f;      // exact: 24 bits times 2^-24
}

struct jt_sample { unsigned long long seed, first; float spread; int enhanced; double cos40; };      // cos40: cos(40 * 3.14 / 180) in double, handtrack.h:437
// One thread per frame: body 0 from the root, then every joint's child from its parent (FixOrientations / FixPositions top down, physmodel.h:357-408).
template <bool SAMPLE> __device__ __forceinline__ void jt_walk(const ht_model_dev &M, const float *__restrict__ jl, const float *__restrict__ roots, const float *__restrict__ coords_in,
                                                               long long B, int com_poses, const jt_sample &sm, float *__restrict__ poses, float *__restrict__ coords_out)
{
	extern __shared__ float jt_lds[];
	const int nb = M.nb, nj = M.nj, tid = threadIdx.x;
	const jt_tables T = jt_load_tables(jt_lds, M, jl, JT_THREADS);
	const int pstride = (nb * HT_POSE) | 1, cstride = (nj * 3) | 1;
	float *ptab = jt_lds + jt_table_floats(nb, nj), *ctab = ptab + JT_THREADS * pstride;
	const long long f0 = (long long)blockIdx.x * JT_THREADS, f = f0 + tid;
	const int live = (int)((B - f0 < JT_THREADS) ? B - f0 : JT_THREADS);
	if (!SAMPLE)      // the block's coordinates, in whole lines
		for (int i = tid; i < live * nj * 3; i += JT_THREADS) ctab[(i / (nj * 3)) * cstride + i % (nj * 3)] = coords_in[(size_t)f0 * nj * 3 + i];
	__syncthreads();
	if (tid < live)
	{
		float *my = ptab + tid * pstride, *myc = ctab + tid * cstride;
		{
			const float *r = roots + (size_t)f * HT_POSE;
			v3 p = load3(r); const v4 q = load4(r + 3);
			if (com_poses) p = p + qrot(q, -load3(T.com));
			my[0] = p.x; my[1] = p.y; my[2] = p.z; my[3] = q.x; my[4] = q.y; my[5] = q.z; my[6] = q.w;
		}
		for (int j = 0; j < nj; j++)
		{
			const float *jc = T.jc + j * HT_JC, *l = T.jl + j * HT_JL;
			const int rb0 = (int)jc[HT_JC_RB0], rb1 = (int)jc[HT_JC_RB1];
			const float *par = my + rb0 * HT_POSE;
			const v3 p0 = load3(par); const v4 q0 = load4(par + 3);
			const v4 F = load4(jc + HT_JC_FRAME); const bool swapped = l[HT_JL_SWAPPED] != 0.0f;
			v3 c;
			if (SAMPLE)
			{
				float cc[3];
#pragma unroll
				for (int a = 0; a < 3; a++)
				{
					const float lo = l[HT_JL_LO + a], hi = l[HT_JL_HI + a];
					const float u = jt_uniform(sm.seed, sm.first + (unsigned long long)f, j, a);
					cc[a] = lo == hi ? lo : (lo + hi) * 0.5f + ((u - 0.5f) * (hi - lo)) * sm.spread;
				}
				c = V3(cc[0], cc[1], cc[2]);
				// HandModelEnhancements handtrack.h:417-420: joint b - 1 of fingertip b = 7, 10, 13, 16 is locked about x at half the angle of the knuckle above it
				// (bones b - 2 and b - 1, both placed); the literals 3.14159f and 3.14f are the reference's
				if (sm.enhanced && j >= 6 && j <= 15 && j % 3 == 0)
				{
					const float cs = clamp_std(dot(qzdir(load4(my + (j - 1) * HT_POSE + 3)), qzdir(load4(my + j * HT_POSE + 3))), 0.0f, 1.0f);
					const float deg = (float)(acos((double)cs) * (double)180.0f / (double)3.14159f / (double)2.0f);
					c.x = sin_f(((deg * 3.14f) / 180.0f) / 2.0f);
				}
			}
			else c = load3(myc + j * 3);
			v4 q1 = jt_child(q0, F, swapped, c);
			// :434-440: a knuckle (joint 4, 7, 10, 13 of bone 5, 8, 11, 14 on the palm) abducts only while its finger is up; otherwise y is locked at 0: one rebuild
			if (SAMPLE && sm.enhanced && (j == 4 || j == 7 || j == 10 || j == 13) && !((double)dot(qydir(load4(my + HT_POSE + 3)), qydir(q1)) > sm.cos40))
			{
				c.y = 0.0f;
				q1 = jt_child(q0, F, swapped, c);
			}
			if (SAMPLE) { myc[j * 3] = c.x; myc[j * 3 + 1] = c.y; myc[j * 3 + 2] = c.z; }
			const v3 p1 = (p0 + qrot(q0, load3(jc + HT_JC_P0))) - qrot(q1, load3(jc + HT_JC_P1));
			float *ch = my + rb1 * HT_POSE;
			ch[0] = p1.x; ch[1] = p1.y; ch[2] = p1.z; ch[3] = q1.x; ch[4] = q1.y; ch[5] = q1.z; ch[6] = q1.w;
		}
		if (com_poses)
			for (int b = 0; b < nb; b++)
			{
				float *e = my + b * HT_POSE;
				const v3 p = load3(e) + qrot(load4(e + 3), load3(T.com + b * 3));
				e[0] = p.x; e[1] = p.y; e[2] = p.z;
			}
	}
	__syncthreads();
	const int np = nb * HT_POSE;
	for (int i = tid; i < live * np; i += JT_THREADS) poses[(size_t)f0 * np + i] = ptab[(i / np) * pstride + i % np];
	if (SAMPLE && coords_out)
		for (int i = tid; i < live * nj * 3; i += JT_THREADS) coords_out[(size_t)f0 * nj * 3 + i] = ctab[(i / (nj * 3)) * cstride + i % (nj * 3)];
}
__global__ __launch_bounds__(JT_THREADS) void k_joint_pose(const ht_model_dev M, const float *__restrict__ jl, const float *__restrict__ roots, const float *__restrict__ coords, long long B, int com_poses,
                                                           float *__restrict__ poses)
{
	jt_walk<false>(M, jl, roots, coords, B, com_poses, jt_sample{ 0, 0, 0.0f, 0, 0.0 }, poses, nullptr);
}
__global__ __launch_bounds__(JT_THREADS) void k_sample_poses(const ht_model_dev M, const float *__restrict__ jl, const float *__restrict__ roots, long long B, int com_poses, const jt_sample sm,
                                                             float *__restrict__ poses, float *__restrict__ coords)
{
	jt_walk<true>(M, jl, roots, nullptr, B, com_poses, sm, poses, coords);
}

// ---- host: the limits of the coordinates, from the rows of physics.h:367-391 -------------------------------------------------------------------------------
// table [nj][HT_JL]: lo[3] hi[3] (a locked axis: lo == hi == its lock value; an unbounded one: the sampler's +-sin(90 deg / 2)), swapped, the unbounded axes as bits
void ht_joint_limits(const float *jointc, int nj, float *table)
{
	for (int j = 0; j < nj; j++)
	{
		const float *c = jointc + (size_t)j * HT_JC; float *o = table + (size_t)j * HT_JL;
		float lmin[3] = { c[HT_JC_RMIN], c[HT_JC_RMIN + 1], c[HT_JC_RMIN + 2] }, lmax[3] = { c[HT_JC_RMAX], c[HT_JC_RMAX + 1], c[HT_JC_RMAX + 2] };
		float jmin[3], jmax[3];
		for (int i = 0; i < 3; i++) { jmin[i] = (lmin[i] * 3.14f) / 180.0f; jmax[i] = (lmax[i] * 3.14f) / 180.0f; }
		const bool swapped = jmin[0] == 0 && jmax[0] == 0 && jmin[2] < jmax[2];      // physics.h:358
		if (swapped)
		{
			const float nmin[3] = { lmin[2], lmin[1], 0.0f }, nmax[3] = { lmax[2], lmax[1], 0.0f };
			for (int i = 0; i < 3; i++) { jmin[i] = (nmin[i] * 3.14f) / 180.0f; jmax[i] = (nmax[i] * 3.14f) / 180.0f; }
		}
		int unbounded = 0;
		const float wide = sinf((90.0f * 3.14f / 180.0f) / 2.0f);
		if (jmax[0] == jmin[0]) o[HT_JL_LO] = o[HT_JL_HI] = sinf(jmin[0] / 2.0f);                                          // :367-370
		else if (jmax[0] - jmin[0] < 360.0f * 3.14f / 180.0f) { o[HT_JL_LO] = sinf(jmin[0] / 2.0f); o[HT_JL_HI] = sinf(jmax[0] / 2.0f); }      // :371-375
		else { o[HT_JL_LO] = -wide; o[HT_JL_HI] = wide; unbounded |= 1; }                                                    // no rows
		if (jmax[1] == jmin[1]) o[HT_JL_LO + 1] = o[HT_JL_HI + 1] = jmin[1];                                              // :378: the angle itself, not its half sine
		else { o[HT_JL_LO + 1] = sinf(jmin[1] / 2.0f); o[HT_JL_HI + 1] = sinf(jmax[1] / 2.0f); }
		if (jmin[2] == jmax[2]) o[HT_JL_LO + 2] = o[HT_JL_HI + 2] = 0.0f;                                                  // :386: zero whatever the limit says
		else { o[HT_JL_LO + 2] = sinf(jmin[2] / 2.0f); o[HT_JL_HI + 2] = sinf(jmax[2] / 2.0f); }
		o[HT_JL_SWAPPED] = swapped ? 1.0f : 0.0f; o[HT_JL_UNBOUNDED] = (float)unbounded;
	}
}
void ht_joint_limits_public(const float *table, int nj, float *lo, float *hi, int *swapped)
{
	for (int j = 0; j < nj; j++)
	{
		const float *o = table + (size_t)j * HT_JL; const int unb = (int)o[HT_JL_UNBOUNDED];
		for (int a = 0; a < 3; a++)
		{
			if (lo) lo[3 * j + a] = (unb >> a) & 1 ? -INFINITY : o[HT_JL_LO + a];
			if (hi) hi[3 * j + a] = (unb >> a) & 1 ? INFINITY : o[HT_JL_HI + a];
		}
		if (swapped) swapped[j] = o[HT_JL_SWAPPED] != 0.0f;
	}
}
// whether a walk in model order places every body: body 0 is the root, a joint's parent has been placed, its child has not
bool ht_joints_ordered(const float *jointc, int nb, int nj)
{
	unsigned placed = 1u;
	for (int j = 0; j < nj; j++)
	{
		const int rb0 = (int)jointc[(size_t)j * HT_JC + HT_JC_RB0], rb1 = (int)jointc[(size_t)j * HT_JC + HT_JC_RB1];
		if (rb0 < 0 || rb0 >= nb || rb1 < 0 || rb1 >= nb || !((placed >> rb0) & 1u) || ((placed >> rb1) & 1u)) return false;
		placed |= 1u << rb1;
	}
	return placed == (nb >= 32 ? ~0u : (1u << nb) - 1u);
}

// whether HandModelEnhancements' couplings can be applied during a walk: bones 5..16 are four chains knuckle (on bone 1) - middle - tip, joint j attaching bone j + 1
bool ht_joints_hand_layout(const float *jointc, int nb, int nj)
{
	if (nb < 17 || nj < 16) return false;
	for (int j = 4; j <= 15; j++)
	{
		const int rb0 = (int)jointc[(size_t)j * HT_JC + HT_JC_RB0], rb1 = (int)jointc[(size_t)j * HT_JC + HT_JC_RB1];
		if (rb1 != j + 1 || rb0 != ((j - 4) % 3 == 0 ? 1 : j)) return false;
	}
	return true;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------------------
static int jt_check(ht_ctx *ctx, const char *fn, int B, int flags, int known, bool ptrs_ok)
{
	CHECK_MODEL(ctx);
	const std::string f(fn);
	if (!ptrs_ok || B < 0) { ctx->err = f + ": bad argument"; return HT_ERR_ARG; }
	if (flags & ~known) { ctx->err = f + ": unknown flags"; return HT_ERR_ARG; }
	for (int j = 0; j < ctx->model.nj; j++)      // the kernels index the poses with these
	{
		const int rb0 = (int)ctx->h_jointc[(size_t)j * HT_JC + HT_JC_RB0], rb1 = (int)ctx->h_jointc[(size_t)j * HT_JC + HT_JC_RB1];
		if (rb0 < 0 || rb0 >= ctx->model.nb || rb1 < 0 || rb1 >= ctx->model.nb) { ctx->err = f + ": a joint of the model names a body it does not have"; return HT_ERR_STATE; }
	}
	return HT_OK;
}
static int jt_check_walk(ht_ctx *ctx, const char *fn)
{
	if (!ht_joints_ordered(ctx->h_jointc.data(), ctx->model.nb, ctx->model.nj))
	{
		ctx->err = std::string(fn) + ": the model's joints are not in top-down order from body 0 (a joint's parent must be placed before it)"; return HT_ERR_STATE;
	}
	return HT_OK;
}
static size_t jt_walk_lds(const ht_model_dev &M) { return ((size_t)M.nj * (HT_JC + HT_JL) + (size_t)M.nb * 3 + (size_t)JT_THREADS * (((M.nb * HT_POSE) | 1) + ((M.nj * 3) | 1))) * sizeof(float); }
static ht_lds_limit jt_lds_limit;

extern "C" int ht_joint_coords_dev(ht_ctx *ctx, const float *d_poses, int B, int flags, float *d_coords, float *d_gaps, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = jt_check(ctx, "ht_joint_coords", B, flags, HT_JOINTS_COM_POSES, d_poses && d_coords); if (r) return r; }
	if (B == 0 || ctx->model.nj == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const long long n = (long long)B * ctx->model.nj;
	const size_t lds = ((size_t)ctx->model.nj * (HT_JC + HT_JL) + (size_t)ctx->model.nb * 3) * sizeof(float);
	hipLaunchKernelGGL(k_joint_coords, dim3((unsigned)((n + JC_THREADS - 1) / JC_THREADS)), dim3(JC_THREADS), lds, s, ctx->model, ctx->d_jointl, d_poses, n, (flags & HT_JOINTS_COM_POSES) ? 1 : 0, d_coords, d_gaps);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_joint_coords(ht_ctx *ctx, const float *poses, int B, int flags, float *coords, float *gaps)
{
	CHECK_READY(ctx);
	{ const int r = jt_check(ctx, "ht_joint_coords", B, flags, HT_JOINTS_COM_POSES, poses && coords); if (r) return r; }
	if (B == 0 || ctx->model.nj == 0) return HT_OK;
	const size_t n = (size_t)B, nb = ctx->model.nb, nj = ctx->model.nj;
	ht_seg seg[3] = { { (void *)poses, n * nb * HT_POSE * sizeof(float), false }, { coords, n * nj * 3 * sizeof(float), true }, { gaps, n * nj * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return ht_joint_coords_dev(ctx, (const float *)seg[0].dev, B, flags, (float *)seg[1].dev, (float *)seg[2].dev, s); });
}

extern "C" int ht_joint_pose_dev(ht_ctx *ctx, const float *d_roots, const float *d_coords, int B, int flags, float *d_poses, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = jt_check(ctx, "ht_joint_pose", B, flags, HT_JOINTS_COM_POSES, d_roots && d_coords && d_poses); if (r) return r; }
	{ const int r = jt_check_walk(ctx, "ht_joint_pose"); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const size_t lds = jt_walk_lds(ctx->model);
	jt_lds_limit.raise(lds, k_joint_pose, k_sample_poses);
	hipLaunchKernelGGL(k_joint_pose, dim3((unsigned)(((long long)B + JT_THREADS - 1) / JT_THREADS)), dim3(JT_THREADS), lds, s, ctx->model, ctx->d_jointl, d_roots, d_coords, (long long)B,
	                   (flags & HT_JOINTS_COM_POSES) ? 1 : 0, d_poses);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_joint_pose(ht_ctx *ctx, const float *roots, const float *coords, int B, int flags, float *poses)
{
	CHECK_READY(ctx);
	{ const int r = jt_check(ctx, "ht_joint_pose", B, flags, HT_JOINTS_COM_POSES, roots && coords && poses); if (r) return r; }
	{ const int r = jt_check_walk(ctx, "ht_joint_pose"); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t n = (size_t)B, nb = ctx->model.nb, nj = ctx->model.nj;
	for (size_t i = 0; i < n * nj; i++)      // the device form clamps these; the host form names them
	{
		const float *c = coords + 3 * i;
		if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && fabsf(c[0]) <= 1.0f && fabsf(c[1]) <= 1.0f && fabsf(c[2]) <= 1.0f && c[0] * c[0] + c[1] * c[1] <= 1.0f))
		{
			ctx->err = "ht_joint_pose: coordinates must be finite with |c| <= 1 and cx*cx + cy*cy <= 1 (frame " + std::to_string(i / nj) + ", joint " + std::to_string(i % nj) + ")"; return HT_ERR_ARG;
		}
	}
	ht_seg seg[3] = { { (void *)roots, n * HT_POSE * sizeof(float), false }, { (void *)coords, n * nj * 3 * sizeof(float), false }, { poses, n * nb * HT_POSE * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return ht_joint_pose_dev(ctx, (const float *)seg[0].dev, (const float *)seg[1].dev, B, flags, (float *)seg[2].dev, s); });
}

static int jt_check_sample(ht_ctx *ctx, int B, float spread, int flags, bool ptrs_ok)
{
	{ const int r = jt_check(ctx, "ht_sample_poses", B, flags, HT_JOINTS_COM_POSES | HT_SAMPLE_ENHANCED, ptrs_ok); if (r) return r; }
	if (!(spread >= 0.0f && spread <= 1.0f)) { ctx->err = "ht_sample_poses: spread must lie in [0, 1]"; return HT_ERR_ARG; }
	if ((flags & HT_SAMPLE_ENHANCED) && !ht_joints_hand_layout(ctx->h_jointc.data(), ctx->model.nb, ctx->model.nj))
	{
		ctx->err = "ht_sample_poses: HT_SAMPLE_ENHANCED is for hand layouts (at least 17 bodies, joint j between bones j and j + 1 along a finger, knuckles on bone 1)"; return HT_ERR_ARG;
	}
	return jt_check_walk(ctx, "ht_sample_poses");
}
extern "C" int ht_sample_poses_dev(ht_ctx *ctx, const float *d_roots, int B, uint64_t seed, uint64_t first_index, float spread, int flags, float *d_poses, float *d_coords, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = jt_check_sample(ctx, B, spread, flags, d_roots && d_poses); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const size_t lds = jt_walk_lds(ctx->model);
	jt_lds_limit.raise(lds, k_joint_pose, k_sample_poses);
	const jt_sample sm = { seed, first_index, spread, (flags & HT_SAMPLE_ENHANCED) ? 1 : 0, ctx->phys.cos40d };
	hipLaunchKernelGGL(k_sample_poses, dim3((unsigned)(((long long)B + JT_THREADS - 1) / JT_THREADS)), dim3(JT_THREADS), lds, s, ctx->model, ctx->d_jointl, d_roots, (long long)B,
	                   (flags & HT_JOINTS_COM_POSES) ? 1 : 0, sm, d_poses, d_coords);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_sample_poses(ht_ctx *ctx, const float *roots, int B, uint64_t seed, uint64_t first_index, float spread, int flags, float *poses, float *coords)
{
	CHECK_READY(ctx);
	{ const int r = jt_check_sample(ctx, B, spread, flags, roots && poses); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t n = (size_t)B, nb = ctx->model.nb, nj = ctx->model.nj;
	ht_seg seg[3] = { { (void *)roots, n * HT_POSE * sizeof(float), false }, { poses, n * nb * HT_POSE * sizeof(float), true }, { coords, n * nj * 3 * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return ht_sample_poses_dev(ctx, (const float *)seg[0].dev, B, seed, first_index, spread, flags, (float *)seg[1].dev, (float *)seg[2].dev, s); });
}
