// ht_train_shared.hpp -- what the per-sample training step (ht_train.hip) and the mini-batch step (ht_train_batch.hip) compute alike: the two
// convolutions forward, the pool / tanh backward into an error map, conv2's backward gather and conv1's gradient over the compact list, each
// written once, with the net's dimensions as template parameters (cnn_dims, ht_device.hpp: the 64x64-input net by default, the 128x128-input one for the
// sized mini-batch step), so that a correction reaches every step.  Every function is the floating-point operations of the kernels it came from, in their
// order (the build has no contraction and no fast math, so that fixes the bits).  Also the index of the packed conv2 copy, which the weight loader
// (ht_api.hip) reads too.
#pragma once
#include "ht_device.hpp"

// conv2 weight (oc, ic, ky, kx) in the MFMA-packed copy W2p[k][oc], k = (ky*4+kx)*16 + ic, that k_conv2 reads (reference index: kx + 4*(ky + 4*(ic + 16*oc)), cnn.h:45-47)
__host__ __device__ static inline size_t cnn_w2p_index(int oc, int ic, int ky, int kx) { return (size_t)((ky * 4 + kx) * 16 + ic) * 64 + oc; }

__device__ __forceinline__ float t_tanh(float t) { float e = (float)exp((double)(2 * t)); return (e - 1) / (e + 1); }      // TanH::f cnn.h:31
// first maximum of a 2x2 window in the reference's scan order (x then y, strict >: cnn.h:150-160)
__device__ __forceinline__ int first_max4(float a, float b, float c, float d, float &m)
{
	int k = 0; m = a;
	if (b > m) { m = b; k = 1; }
	if (c > m) { m = c; k = 2; }
	if (d > m) { m = d; k = 3; }
	return k;
}
__device__ __forceinline__ float wave_sum(float v) { for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ float seg16_sum(float v) { for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ float seg8_sum(float v) { for (int o = 4; o >= 1; o >>= 1) v += __shfl_xor(v, o); return v; }

// conv1 (5x5, 1 -> 16 channels, S x S -> (S-4) x (S-4)) + tanh: output (oz, y, x) of one S x S input, taps in the reference's order (cnn.h:226-228)
template <int S = 64> __device__ __forceinline__ float t_conv1_out(const float *in, const float *W, const float *B, int oz, int y, int x)
{
	float acc = B[oz];
#pragma unroll
	for (int ky = 0; ky < 5; ky++)
#pragma unroll
		for (int kx = 0; kx < 5; kx++) acc += in[(y + ky) * S + x + kx] * W[kx + 5 * (ky + 5 * oz)];
	return t_tanh(acc);
}
// conv2 (4x4, 16 -> 64 channels, P2 x P2 -> C2 x C2, C2 = P2 - 3) + tanh of one sample (a3 [16][P2][P2]) and output channel oz by a block of NT threads:
// input and taps staged in the caller's LDS (s_in [16 P2 P2], s_w [256]); output e = y C2 + x is left in s_o[e] by thread e % NT, which returns the last
// one it formed (with C2 C2 <= NT, as at P2 = 15: thread t < 144 returns output t).  No barrier after the outputs.
template <int P2 = 15, int NT = 192> __device__ __forceinline__ float t_conv2_out(const float *a3, const float *W, const float *B, int oz, float *s_in, float *s_w, float *s_o)
{
	constexpr int C2 = P2 - 3;
	const int t = threadIdx.x;
	for (int i = t; i < 16 * P2 * P2; i += NT) s_in[i] = a3[i];
	for (int i = t; i < 256; i += NT) s_w[i] = W[oz * 256 + i];
	__syncthreads();
	float o = 0.0f;
	for (int e = t; e < C2 * C2; e += NT)
	{
		const int x = e % C2, y = e / C2;
		float acc = B[oz];
		for (int ky = 0; ky < 4; ky++) for (int kx = 0; kx < 4; kx++)
#pragma unroll
			for (int iz = 0; iz < 16; iz++) acc += s_in[iz * P2 * P2 + (y + ky) * P2 + x + kx] * s_w[kx + 4 * (ky + 4 * iz)];
		o = t_tanh(acc);
		s_o[e] = o;
	}
	return o;
}
// third max-pool backward into a channel's error map e4c of C2-wide rows: entry k (x fastest) of the 2x2 window p (p / (C2/2) = window row, counted from
// e4c's first row), its first maximum, takes the error d and the other three are cleared (cnn.h:150-164).  The caller folds conv2's tanh' (1 - m^2 at
// the maximum m) into d.
template <int C2 = 12> __device__ __forceinline__ void t_window_scatter(float *e4c, int p, int k, float d)
{
	const int base = (2 * (p / (C2 / 2))) * C2 + 2 * (p % (C2 / 2));
	e4c[base] = k == 0 ? d : 0.0f; e4c[base + 1] = k == 1 ? d : 0.0f; e4c[base + C2] = k == 2 ? d : 0.0f; e4c[base + C2 + 1] = k == 3 ? d : 0.0f;
}
// LConv::backward of conv2 as a gather (cnn.h:236-250) for input position (x, y) of one input channel: s_e [NOZ][ROWS][C2] rows row0 .. row0 + ROWS - 1 of
// the output channels' error maps (the whole maps, or the band that position reads), s_w [NOZ][16] their taps on that input channel; output channel,
// output y, output x ascending
template <int NOZ, int C2 = 12, int ROWS = 12> __device__ __forceinline__ float t_conv2_back_gather(const float *s_w, const float *s_e, int x, int y, int row0 = 0)
{
	const int oy0 = max(0, y - 3), oy1 = min(C2 - 1, y), ox0 = max(0, x - 3), ox1 = min(C2 - 1, x);
	float acc = 0.0f;
	for (int oz = 0; oz < NOZ; oz++) for (int oy = oy0; oy <= oy1; oy++) for (int ox = ox0; ox <= ox1; ox++)
		acc += s_w[oz * 16 + (x - ox) + 4 * (y - oy)] * s_e[oz * (ROWS * C2) + (oy - row0) * C2 + ox];
	return acc;
}
// LConv::update (cnn.h:252-279) of one conv1 channel for one sample.  The two max-pools pass conv1's error to one position per 4x4 window only, so
// it is a list of NP (225 at S = 64, 961 at 128) (input position s_i, value after tanh' s_e) pairs over the input s_x [S][S]; eight lanes (sub) per tap share
// the list: taps 0..24, tap 25 = bias, 26..31 idle.  Adds a lane's share to acc; seg8_sum of acc finishes the tap (once per sample, or after several samples).
template <int S = 64, int NP = 225> __device__ __forceinline__ float t_conv1_grad_add(float acc, const float *s_x, const int *s_i, const float *s_e, int tap, int sub)
{
	const int off = tap < 25 ? (tap / 5) * S + tap % 5 : 0;
	if (tap < 25) for (int p = sub; p < NP; p += 8) acc += s_x[s_i[p] + off] * s_e[p];
	else if (tap == 25) for (int p = sub; p < NP; p += 8) acc += s_e[p];
	return acc;
}
