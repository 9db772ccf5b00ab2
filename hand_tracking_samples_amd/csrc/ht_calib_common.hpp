// ht_calib_common.hpp -- what the Gauss-Newton loops around closest() share (ht_calib.hip: a view's extrinsics; ht_size.hip: the hand's size, section
// 41), each stated once: closest() keeping its plane, the staging of the face planes and the body table, the block's reduction of N float64 sums in its fixed order, the
// Cholesky factor and its two substitutions, the rigid update of a float64 transform, the record's stores; and the host pieces the second loop takes from the first (the
// argument checks, the cloud's buffers and its launch).
//
// Reference computations:
//   closest(rigidbodies, v), mostabove           include/physmodel.h:137-162, :127-131
#pragma once
#include <limits.h>
#include <string.h>
#include <math.h>
#include "ht_host.hpp"
#include "ht_prepare.hpp"

#define CA_THREADS 256
#define CA_BT 32       // floats per body-table entry, k_split_model's layout: pos 0..2 | radius 3 | rinner 4 | invp 5..7 | RI columns 8..16 | RF columns 17..25 | first face, faces (as integers) 26, 27
#define CA_MAX_ITER 64
#define CA_MAX_B 65535

extern __shared__ __attribute__((aligned(16))) float4 ca_planes[];      // all face planes of the model

// closest(rigidbodies, v), physmodel.h:137-162, for one point by one lane against the bodies of `tab`: the plane it returns (sm_closest of ht_split_model.hip keeps the
// distance alone).  dmin is dot(pmin, (v, 1)) throughout, as the reference re-evaluates it
__device__ __forceinline__ v4 ca_closest(const float *tab, int nb, v3 v)
{
	v4 pmin = V4(0, 0, 0, FLT_MAX);
	float dmin = dot_plane(pmin, v);
	for (int b = 0; b < nb; b++)      // :141-150
	{
		const float *t = tab + b * CA_BT;
		const v3 pos = V3(t[0], t[1], t[2]);
		const v3 n = safenormalize(v - pos);
		const v4 p = V4(n, -dot(pos, n) - t[4]);
		const float d = dot_plane(p, v);
		if (d < dmin) { dmin = d; pmin = p; }
	}
	for (int b = 0; b < nb; b++)      // :151-160
	{
		const float *t = tab + b * CA_BT;
		const v3 pos = V3(t[0], t[1], t[2]);
		if (length(v - pos) - t[3] > dmin) continue;
		const v3 X = V3(t[8], t[9], t[10]), Y = V3(t[11], t[12], t[13]), Z = V3(t[14], t[15], t[16]);
		const v3 vl = V3(t[5], t[6], t[7]) + ((X * v.x + Y * v.y) + Z * v.z);      // pose.inverse() * v
		const float4 *pl = ca_planes + __float_as_int(t[26]);
		const int np = __float_as_int(t[27]);
		float4 f = pl[0];      // mostabove :127-131: std::max_element keeps the first maximum
		float best = dot_plane(V4(f.x, f.y, f.z, f.w), vl);
		for (int i = 1; i < np; i++)
		{
			const float4 g = pl[i];
			const float d = dot_plane(V4(g.x, g.y, g.z, g.w), vl);
			if (best < d) { best = d; f = g; }
		}
		const v3 FX = V3(t[17], t[18], t[19]), FY = V3(t[20], t[21], t[22]), FZ = V3(t[23], t[24], t[25]);
		const v3 n = (FX * f.x + FY * f.y) + FZ * f.z;      // Pose::TransformPlane, geometric.h:124
		const v4 p = V4(n, f.w - dot(pos, n));
		const float d = dot_plane(p, v);
		if (d < dmin) { dmin = d; pmin = p; }
	}
	return pmin;
}

// the model's face planes into ca_planes and slot b's body table into tab [nb][CA_BT] by a block of CA_THREADS; body k of slot b at poses + (b nb + k) pose_stride
// (7: poses; HT_STATE_STRIDE: the slots' state).  The caller's barrier follows
__device__ __forceinline__ void ca_stage(const ht_model_dev &M, const float *__restrict__ poses, int pose_stride, int b, float *tab)
{
	const int t = threadIdx.x, nb = M.nb;
	{
		const int np = M.plane_off[nb];
		for (int i = t; i < np; i += CA_THREADS) ca_planes[i] = M.planes[i];
	}
	if (t < nb)
	{
		const float *p = poses + ((size_t)b * (unsigned)nb + (unsigned)t) * (unsigned)pose_stride;
		const v3 pos = V3(p[0], p[1], p[2]);
		const v4 q = V4(p[3], p[4], p[5], p[6]);
		const float *bc = M.bodyc + t * HT_BC;
		const xf pi = inverse(XF(pos, q));
		const m3 ri = qmat(pi.q), rf = qmat(q);
		float *e = &tab[t * CA_BT];
		e[0] = pos.x; e[1] = pos.y; e[2] = pos.z; e[3] = bc[HT_BC_RADIUS]; e[4] = bc[HT_BC_RINNER];
		e[5] = pi.p.x; e[6] = pi.p.y; e[7] = pi.p.z;
		e[8] = ri.x.x; e[9] = ri.x.y; e[10] = ri.x.z; e[11] = ri.y.x; e[12] = ri.y.y; e[13] = ri.y.z; e[14] = ri.z.x; e[15] = ri.z.y; e[16] = ri.z.z;
		e[17] = rf.x.x; e[18] = rf.x.y; e[19] = rf.x.z; e[20] = rf.y.x; e[21] = rf.y.y; e[22] = rf.y.z; e[23] = rf.z.x; e[24] = rf.z.y; e[25] = rf.z.z;
		e[26] = __int_as_float(M.plane_off[t]); e[27] = __int_as_float(M.plane_off[t + 1] - M.plane_off[t]);
	}
}

// NS float64 sums a thread of a block of CA_THREADS -> out[0..NS) and the point count n at out[NS].  The wave: a fixed butterfly through registers (every lane ends with
// the same bits); the waves: 4 x NS doubles of LDS, added as (w0 + w1) + (w2 + w3)
template <int NS> __device__ __forceinline__ void ca_reduce(const double (&acc)[NS], double (*red)[NS], double *__restrict__ out, int n)
{
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
	for (int k = 0; k < NS; k++)
	{
		double v = acc[k];
#pragma unroll
		for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
		if (lane == 0) red[wave][k] = v;
	}
	__syncthreads();
	if (t < NS) out[t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
	else if (t == NS) out[NS] = (double)n;
}

// a float64 as two words: the caller's stats are 4-byte aligned and no more
__device__ __forceinline__ void ca_store(unsigned *at, double v) { at[0] = (unsigned)__double2loint(v); at[1] = (unsigned)__double2hiint(v); }
__device__ __forceinline__ bool ca_finite(double v) { return fabs(v) <= DBL_MAX; }      // false for NaN too

// Cholesky A = L L^T of the lower triangle held in L, column by column, in place; a pivot that is not > 0 is replaced by 1 and reported
template <int N> __device__ __forceinline__ bool ca_cholesky(double (&L)[N][N])
{
	bool ok = true;
#pragma unroll
	for (int j = 0; j < N; j++)
	{
		double v = L[j][j];
#pragma unroll
		for (int k = 0; k < j; k++) v -= L[j][k] * L[j][k];
		if (!(v > 0.0)) { ok = false; v = 1.0; }
		const double pj = sqrt(v);
		L[j][j] = pj;
#pragma unroll
		for (int i = j + 1; i < N; i++)
		{
			double u = L[i][j];
#pragma unroll
			for (int k = 0; k < j; k++) u -= L[i][k] * L[j][k];
			L[i][j] = u / pj;
		}
	}
	return ok;
}
// L L^T d = rhs: forward y_i = (rhs_i - L_i0 y_0 - ..) / L_ii, back d_i = (y_i - L_{i+1,i} d_{i+1} - ..) / L_ii, k ascending in both
template <int N> __device__ __forceinline__ void ca_substitute(const double (&L)[N][N], const double (&rhs)[N], double (&d)[N])
{
	double y[N];
#pragma unroll
	for (int i = 0; i < N; i++)
	{
		double v = rhs[i];
#pragma unroll
		for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
		y[i] = v / L[i][i];
	}
#pragma unroll
	for (int i = N - 1; i >= 0; i--)
	{
		double v = y[i];
#pragma unroll
		for (int k = i + 1; k < N; k++) v -= L[k][i] * d[k];
		d[i] = v / L[i][i];
	}
}
// the candidate of a step d = (dt, dw) about (cx, cy, cz) from Ts [7]: dq = (dw / 2, 1) normalised, q <- qmul(dq, q) / its length, pos <- (c + qrot(dq, pos - c)) + dt.
// -> n [7]; true iff every entry is finite
__device__ __forceinline__ bool ca_candidate(const double *Ts, const double *d, double cx, double cy, double cz, double (&n)[7])
{
	const double hx = d[3] * 0.5, hy = d[4] * 0.5, hz = d[5] * 0.5;
	const double hl = sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0);
	const double ax = hx / hl, ay = hy / hl, az = hz / hl, aw = 1.0 / hl;      // dq
	const double bx = Ts[3], by = Ts[4], bz = Ts[5], bw = Ts[6];
	double qx = ax * bw + aw * bx + ay * bz - az * by, qy = ay * bw + aw * by + az * bx - ax * bz, qz = az * bw + aw * bz + ax * by - ay * bx, qw = aw * bw - ax * bx - ay * by - az * bz;
	const double ql = sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw);
	qx = qx / ql; qy = qy / ql; qz = qz / ql; qw = qw / ql;
	const double px = Ts[0] - cx, py = Ts[1] - cy, pz = Ts[2] - cz;
	const double Xx = aw * aw + ax * ax - ay * ay - az * az, Xy = (ax * ay + az * aw) * 2.0, Xz = (az * ax - ay * aw) * 2.0;
	const double Yx = (ax * ay - az * aw) * 2.0, Yy = aw * aw - ax * ax + ay * ay - az * az, Yz = (ay * az + ax * aw) * 2.0;
	const double Zx = (az * ax + ay * aw) * 2.0, Zy = (ay * az - ax * aw) * 2.0, Zz = aw * aw - ax * ax - ay * ay + az * az;
	n[0] = (cx + ((Xx * px + Yx * py) + Zx * pz)) + d[0]; n[1] = (cy + ((Xy * px + Yy * py) + Zy * pz)) + d[1]; n[2] = (cz + ((Xz * px + Yz * py) + Zz * pz)) + d[2];
	n[3] = qx; n[4] = qy; n[5] = qz; n[6] = qw;
	return ca_finite(n[0]) && ca_finite(n[1]) && ca_finite(n[2]) && ca_finite(qx) && ca_finite(qy) && ca_finite(qz) && ca_finite(qw);
}

// ---- host (ht_calib.hip) ------------------------------------------------------------------------------------------------------------------------------------------
struct ca_call { ht_calib o; int bound, N; };      // bound: the most points a slot's cloud can have; N: transforms
// every refusal that needs no device, before anything grows or runs (a context that never came up answers them too)
int ht_calib_check(ht_ctx *ctx, const char *fn, int which, const void *poses, const void *depth, const void *cams, int w, int h, int B, const ht_calib *opt, const void *T_out, const void *stats, ca_call &c);
// what needs the device but launches nothing: the context's state, the model's planes against `lds_fixed` bytes of static LDS, and the cloud's buffers grown to this call
int ht_calib_reserve(ht_ctx *ctx, const char *fn, const ca_call &c, int B, size_t lds_fixed);
// k_calib_cloud on s: the view's clouds into the context's buffer, the cameras' poses widened into its float64 transforms (one a slot, or slot 0's alone)
void ht_calib_cloud(ht_ctx *ctx, const ca_call &c, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, int per_slot, hipStream_t s);
