// ht_optim.hip -- the mini-batch gradient as a buffer, and the optimiser steps over it.
//
// ht_train_batch.hip forms  SUM_b g_b(w)  tile by tile and applies it where it stands.  Here the same sums are written out: G, one float per weight in .cnnb order
// (cnnb_layout), and a step over all weights of a net reads G, the weights and the optimiser's state.  The forward pass, the soft-max and the backward-data kernels of a
// gradient call are the launches of ht_train_batch.hip, unchanged (tb_step); the kernels of this file take the place of the two weight steps and of k_tb_conv_apply.
//
// The step, per element i (k_opt_step).  fp32 throughout, one IEEE operation per written operation, in this order (the build has -ffp-contract=off, and `/` and sqrtf
// are correctly rounded).  gs = grad_scale, c = the clip factor:
//     g = (G[i] * gs) * c
//   Decay applies to W1 W2 W3 W4 only, never to B1..B4 (decided per element from the eight ranges of cnnb_layout).
//   Coupled decay (decoupled_decay = 0, weight_decay != 0), on the W ranges:   g = g + weight_decay * w
//   SGD        w' = w - lr * g
//   MOMENTUM   m' = momentum * m + g,   w' = w - lr * m'
//   NESTEROV   the same m',             w' = w - lr * (g + momentum * m')
//   ADAM       t' = t + 1
//              m' = beta1 * m + omb1 * g
//              v' = beta2 * v + (omb2 * g) * g
//              u = (m' / bc1) / (sqrtf(v' / bc2) + eps)
//              with decoupled_decay, on the W ranges:   u = u + weight_decay * w
//              w' = w - lr * u
//              omb1 = 1.0f - beta1 and omb2 = 1.0f - beta2 are formed in float, bc1 = (float)(1.0 - pow((double)beta1, t')), likewise bc2: all four on the host,
//              passed as kernel arguments.  t counts the Adam steps of the net; the other kinds leave it.
//   Clip       norm = sqrt(SUM_i ((double)G[i] * (double)gs)^2), squares and sums in float64: a thread adds the elements of its 128-bit groups q = t, t + T, t + 2 T, ...
//              in order (T = all threads of k_opt_norm), a block adds its threads pairwise (stride 128, 64, ... 1), k_opt_norm_final adds the blocks' partial sums in block order.
//              c = norm > clip_norm ? (float)((double)clip_norm / norm) : 1.0f.  Clipping off: c = 1.0f and no norm kernel is launched.
//              The factor reaches k_opt_step through device memory, so the call stays asynchronous.
#include "ht_device.hpp"
#include "ht_launch.hpp"
#include "ht_train_shared.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Weight gradient of a fully connected layer into G: G[i,j] = (accumulate ? G[i,j] : 0) + sum_b X[b,i] E[b,j], G [M][N] row-major.  The products are k_tb_fc_wgrad's
// (ht_train_batch.hip): the sample is the summed index, lanes 0..31 hold sample 2 s, lanes 32..63 sample 2 s + 1 (zero beyond n), a wave owns one 32x32 tile, a block
// four tiles side by side.  The weights are never read; the tile of G is read only when accumulating, before the products.  The blocks of the first tile row also
// write the bias gradient, GB[j] = (accumulate ? GB[j] : 0) + sum_b E[b,j], samples ascending.
__global__ __launch_bounds__(256) void k_opt_fc_wgrad(float *__restrict__ G, float *__restrict__ GB, const float *__restrict__ X, const float *__restrict__ E, int n, int M, int N, int accumulate)
{
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
	const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 128 + 32 * w;
	float *gp = G + (size_t)(i0 + 4 * h) * N + j0 + r;
	float gv[16];
#pragma unroll
	for (int g = 0; g < 16; g++) gv[g] = 0.0f;
	if (accumulate)
	{
#pragma unroll
		for (int g = 0; g < 16; g++) gv[g] = gp[(size_t)((g & 3) + 8 * (g >> 2)) * N];
	}
	f32x16 acc;
#pragma unroll
	for (int g = 0; g < 16; g++) acc[g] = 0.0f;
	const float *xp = X + i0 + r, *ep = E + j0 + r;
#pragma unroll 4
	for (int s = 0; s < n; s += 2)
	{
		const int b = s + h;
		const bool on = b < n;
		float xv = xp[(size_t)(on ? b : 0) * M], ev = ep[(size_t)(on ? b : 0) * N];
		if (!on) { xv = 0.0f; ev = 0.0f; }
		acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, ev, acc, 0, 0, 0);
	}
	if (accumulate)
	{
#pragma unroll
		for (int g = 0; g < 16; g++) gp[(size_t)((g & 3) + 8 * (g >> 2)) * N] = gv[g] + acc[g];
	}
	else
	{
#pragma unroll
		for (int g = 0; g < 16; g++) gp[(size_t)((g & 3) + 8 * (g >> 2)) * N] = acc[g];
	}
	if (blockIdx.y == 0 && lane < 32)
	{
		float sum = 0.0f;
		for (int b = 0; b < n; b++) sum += ep[(size_t)b * N];
		GB[j0 + r] = accumulate ? GB[j0 + r] + sum : sum;
	}
}
void ht_launch_opt_fc_wgrad(float *G, float *GB, const float *X, const float *E, int n, int M, int N, int accumulate, hipStream_t s)
{
	hipLaunchKernelGGL(k_opt_fc_wgrad, dim3(N / 128, M / 32), dim3(256), 0, s, G, GB, X, E, n, M, N, accumulate);
}
// The convolutions' gradients: the groups' partial sums pw [groups][stride] (k_tb_conv_grad's layout: W2 [16384], B2 [64], then 16 x (25 taps of W1 + B1); made with
// alpha = -1, so that they are the plain sums) added in group order into G's W2, B2, W1 and B1 ranges
__global__ __launch_bounds__(256) void k_opt_conv_reduce(const float *__restrict__ pw, int groups, int stride, float *__restrict__ G1, float *__restrict__ GB1, float *__restrict__ G2, float *__restrict__ GB2, int accumulate)
{
	const int e = blockIdx.x * 256 + threadIdx.x;
	if (e >= 16384 + 64 + 16 * 26) return;
	float sum = 0.0f;
	for (int g = 0; g < groups; g++) sum += pw[(size_t)g * stride + e];
	float *p;
	if (e < 16384) p = G2 + e;
	else if (e < 16448) p = GB2 + (e - 16384);
	else
	{
		const int q = e - 16448, oz = q / 26, tap = q % 26;
		p = tap < 25 ? G1 + oz * 25 + tap : GB1 + oz;
	}
	*p = accumulate ? *p + sum : sum;
}
void ht_launch_opt_conv_reduce(const float *pw, int groups, int stride, float *G1, float *GB1, float *G2, float *GB2, int accumulate, hipStream_t s)
{
	hipLaunchKernelGGL(k_opt_conv_reduce, dim3((16384 + 64 + 16 * 26 + 255) / 256), dim3(256), 0, s, pw, groups, stride, G1, GB1, G2, GB2, accumulate);
}

// ---- the global norm ------------------------------------------------------------------------------------------------------------------------
#define OPT_NORM_BLOCKS 512
// float64 partial sums of ((double)G[i] * (double)gs)^2.  Thread t of all T = OPT_NORM_BLOCKS x 256 takes the 128-bit groups q = t, t + T, ... of G, each group's four
// elements in order, on one running sum; the n % 4 elements after the last group go to thread 0 of block 0, after its groups.  The block's 256 sums are added pairwise.
__global__ __launch_bounds__(256) void k_opt_norm(const float *__restrict__ G, unsigned n, float gs, double *__restrict__ part)
{
	__shared__ double red[256];
	const unsigned t = threadIdx.x, T = gridDim.x * 256u, nv = n >> 2;
	const double s = (double)gs;
	double sum = 0.0;
#pragma unroll 4
	for (unsigned q = blockIdx.x * 256u + t; q < nv; q += T)
	{
		const float4 g = reinterpret_cast<const float4 *>(G)[q];
		const double x = (double)g.x * s, y = (double)g.y * s, z = (double)g.z * s, w = (double)g.w * s;
		sum += x * x; sum += y * y; sum += z * z; sum += w * w;
	}
	if (blockIdx.x == 0 && t == 0) for (unsigned i = 4 * nv; i < n; i++) { const double x = (double)G[i] * s; sum += x * x; }
	red[t] = sum;
	__syncthreads();
	for (unsigned k = 128; k > 0; k >>= 1)
	{
		if (t < k) red[t] += red[t + k];
		__syncthreads();
	}
	if (t == 0) part[blockIdx.x] = red[0];
}
// one block: the OPT_NORM_BLOCKS partial sums, staged in LDS by all threads, added in block order by one; the norm and the clip factor.  stat[0] = norm, the float at
// stat + 1 = the factor
__global__ __launch_bounds__(256) void k_opt_norm_final(const double *__restrict__ part, float clip_norm, double *__restrict__ stat)
{
	__shared__ double p[OPT_NORM_BLOCKS];
	for (int b = threadIdx.x; b < OPT_NORM_BLOCKS; b += 256) p[b] = part[b];
	__syncthreads();
	if (threadIdx.x != 0) return;
	double sum = 0.0;
	for (int b = 0; b < OPT_NORM_BLOCKS; b++) sum += p[b];
	const double norm = sqrt(sum);
	stat[0] = norm;
	*reinterpret_cast<float *>(stat + 1) = norm > (double)clip_norm ? (float)((double)clip_norm / norm) : 1.0f;
}
size_t ht_opt_stat_doubles() { return 2 + OPT_NORM_BLOCKS; }
// stat: ht_opt_stat_doubles() doubles: the norm, the factor (a float), then the blocks' partial sums
void ht_launch_opt_norm(const float *G, size_t n, float gs, float clip_norm, double *stat, hipStream_t s)
{
	hipLaunchKernelGGL(k_opt_norm, dim3(OPT_NORM_BLOCKS), dim3(256), 0, s, G, (unsigned)n, gs, stat + 2);
	hipLaunchKernelGGL(k_opt_norm_final, dim3(1), dim3(256), 0, s, stat + 2, clip_norm, stat);
}

// ---- the step -------------------------------------------------------------------------------------------------------------------------------
// whether element i is a weight (W1 W2 W3 W4) rather than a bias: r = where W1 B1 W2 B2 W3 B3 W4 B4 begin
__device__ static inline bool opt_is_weight(unsigned i, const ht_opt_args &a)
{
	return i < a.r[1] || (i >= a.r[2] && i < a.r[3]) || (i >= a.r[4] && i < a.r[5]) || (i >= a.r[6] && i < a.r[7]);
}
// one element, as the head of this file writes it; m and v are read and written only by the kinds that keep them
template <int KIND> __device__ static inline void opt_element(unsigned i, float &w, float G, float &m, float &v, float c, const ht_opt_args &a)
{
	float g = (G * a.gs) * c;
	const bool decay = (a.coupled || a.decoupled) && opt_is_weight(i, a);
	if (a.coupled && decay) g = g + a.wd * w;
	if (KIND == HT_OPT_SGD) w = w - a.lr * g;
	else if (KIND == HT_OPT_MOMENTUM) { m = a.momentum * m + g; w = w - a.lr * m; }
	else if (KIND == HT_OPT_NESTEROV) { m = a.momentum * m + g; w = w - a.lr * (g + a.momentum * m); }
	else
	{
		m = a.beta1 * m + a.omb1 * g;
		v = a.beta2 * v + (a.omb2 * g) * g;
		float u = (m / a.bc1) / (sqrtf(v / a.bc2) + a.eps);
		if (a.decoupled && decay) u = u + a.wd * w;
		w = w - a.lr * u;
	}
}
// all n elements of a net: thread t < n / 4 takes elements 4 t .. 4 t + 3 with 128-bit accesses, the n % 4 threads after them one element each of the tail
template <int KIND> __global__ __launch_bounds__(256) void k_opt_step(float *__restrict__ W, const float *__restrict__ G, float *__restrict__ M, float *__restrict__ V, unsigned n, const float *__restrict__ clip, ht_opt_args a)
{
	constexpr bool HM = KIND != HT_OPT_SGD, HV = KIND == HT_OPT_ADAM;
	const unsigned t = blockIdx.x * 256u + threadIdx.x, nv = n >> 2;
	const float c = clip ? *clip : 1.0f;
	if (t < nv)
	{
		float4 w = reinterpret_cast<float4 *>(W)[t];
		const float4 g = reinterpret_cast<const float4 *>(G)[t];
		float4 m = make_float4(0, 0, 0, 0), v = make_float4(0, 0, 0, 0);
		if (HM) m = reinterpret_cast<float4 *>(M)[t];
		if (HV) v = reinterpret_cast<float4 *>(V)[t];
		opt_element<KIND>(4 * t, w.x, g.x, m.x, v.x, c, a);
		opt_element<KIND>(4 * t + 1, w.y, g.y, m.y, v.y, c, a);
		opt_element<KIND>(4 * t + 2, w.z, g.z, m.z, v.z, c, a);
		opt_element<KIND>(4 * t + 3, w.w, g.w, m.w, v.w, c, a);
		reinterpret_cast<float4 *>(W)[t] = w;
		if (HM) reinterpret_cast<float4 *>(M)[t] = m;
		if (HV) reinterpret_cast<float4 *>(V)[t] = v;
	}
	else if (t - nv < (n & 3u))
	{
		const unsigned i = 4 * nv + (t - nv);
		float w = W[i], m = HM ? M[i] : 0.0f, v = HV ? V[i] : 0.0f;
		opt_element<KIND>(i, w, G[i], m, v, c, a);
		W[i] = w;
		if (HM) M[i] = m;
		if (HV) V[i] = v;
	}
}
// W, G, M, V: n floats each, 16-byte aligned (M for the kinds with momentum, V for Adam); clip: the factor on the device, or null for 1.0f
void ht_launch_opt_step(int kind, float *W, const float *G, float *M, float *V, size_t n, const float *clip, const ht_opt_args &a, hipStream_t s)
{
	const unsigned threads = (unsigned)(n / 4 + n % 4);
	const dim3 g((threads + 255) / 256), t(256);
	if (kind == HT_OPT_SGD) hipLaunchKernelGGL(k_opt_step<HT_OPT_SGD>, g, t, 0, s, W, G, M, V, (unsigned)n, clip, a);
	else if (kind == HT_OPT_MOMENTUM) hipLaunchKernelGGL(k_opt_step<HT_OPT_MOMENTUM>, g, t, 0, s, W, G, M, V, (unsigned)n, clip, a);
	else if (kind == HT_OPT_NESTEROV) hipLaunchKernelGGL(k_opt_step<HT_OPT_NESTEROV>, g, t, 0, s, W, G, M, V, (unsigned)n, clip, a);
	else hipLaunchKernelGGL(k_opt_step<HT_OPT_ADAM>, g, t, 0, s, W, G, M, V, (unsigned)n, clip, a);
}
// conv2's weights into the MFMA-packed copy k_conv2 reads (cnn_w2p_index), as k_tb_conv_apply leaves it after a fused step
__global__ __launch_bounds__(256) void k_opt_pack_w2(const float *__restrict__ W2, float *__restrict__ W2p)
{
	const int e = blockIdx.x * 256 + threadIdx.x;
	const int oz = e >> 8, t = e & 255, kx = t & 3, ky = (t >> 2) & 3, iz = t >> 4;
	W2p[cnn_w2p_index(oz, iz, ky, kx)] = W2[e];
}
void ht_launch_opt_pack_w2(const float *W2, float *W2p, hipStream_t s) { hipLaunchKernelGGL(k_opt_pack_w2, dim3(16384 / 256), dim3(256), 0, s, W2, W2p); }
