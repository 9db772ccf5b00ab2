// ht_train_shared.hpp -- what the per-sample training step (ht_train.hip) and the mini-batch step (ht_train_batch.hip) compute alike: the two
// convolutions forward, the pool / tanh backward into a 12x12 error map, conv2's backward gather and conv1's gradient over the compact list, each
// written once so that a correction reaches both steps.  Every function is the floating-point operations of the kernels it came from, in their
// order (the build has no contraction and no fast math, so that fixes the bits).  Also the .cnnb layout and the index of the packed conv2 copy,
// which the weight loader (ht_api.hip) reads too.
#pragma once
#include "ht_device.hpp"

// The .cnnb order of the weights (CNN::saveb cnn.h:591-593) from the base pointer; fc_in = inputs of the first fully connected layer (2304 of the
// 64x64-input net, 12544 of the 128x128 one)
template <class T> struct cnnb_layout { T *W1, *B1, *W2, *B2, *W3, *B3, *W4, *B4; };
template <class T> static inline cnnb_layout<T> cnnb_layout_of(T *w, size_t fc_in = 2304)
{
	cnnb_layout<T> L;
	L.W1 = w; L.B1 = L.W1 + 400; L.W2 = L.B1 + 16; L.B2 = L.W2 + 16384; L.W3 = L.B2 + 64; L.B3 = L.W3 + fc_in * 2048; L.W4 = L.B3 + 2048; L.B4 = L.W4 + (size_t)2048 * 2304;
	return L;
}
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

// conv1 (5x5, 1 -> 16 channels, 64x64 -> 60x60) + tanh: output (oz, y, x) of one 64x64 input, taps in the reference's order (cnn.h:226-228)
__device__ __forceinline__ float t_conv1_out(const float *in, const float *W, const float *B, int oz, int y, int x)
{
	float acc = B[oz];
#pragma unroll
	for (int ky = 0; ky < 5; ky++)
#pragma unroll
		for (int kx = 0; kx < 5; kx++) acc += in[(y + ky) * 64 + x + kx] * W[kx + 5 * (ky + 5 * oz)];
	return t_tanh(acc);
}
// conv2 (4x4, 16 -> 64 channels, 15x15 -> 12x12) + tanh of one sample (a3 [16][15][15]) and output channel oz by a block of 192 threads: input and
// taps staged in the caller's LDS (s_in [3600], s_w [256]), thread t < 144 leaves its output in s_o[t] and returns it.  No barrier after the outputs.
__device__ __forceinline__ float t_conv2_out(const float *a3, const float *W, const float *B, int oz, float *s_in, float *s_w, float *s_o)
{
	const int t = threadIdx.x;
	for (int i = t; i < 3600; i += 192) s_in[i] = a3[i];
	for (int i = t; i < 256; i += 192) s_w[i] = W[oz * 256 + i];
	__syncthreads();
	float o = 0.0f;
	if (t < 144)
	{
		const int x = t % 12, y = t / 12;
		float acc = B[oz];
		for (int ky = 0; ky < 4; ky++) for (int kx = 0; kx < 4; kx++)
#pragma unroll
			for (int iz = 0; iz < 16; iz++) acc += s_in[iz * 225 + (y + ky) * 15 + x + kx] * s_w[kx + 4 * (ky + 4 * iz)];
		o = t_tanh(acc);
		s_o[t] = o;
	}
	return o;
}
// third max-pool backward into a channel's 12x12 error map e4c: entry k (x fastest) of pooled element p's 2x2 window, its first maximum, takes the
// error d and the other three are cleared (cnn.h:150-164).  The caller folds conv2's tanh' (1 - m^2 at the maximum m) into d.
__device__ __forceinline__ void t_window_scatter(float *e4c, int p, int k, float d)
{
	const int base = (2 * (p / 6)) * 12 + 2 * (p % 6);
	e4c[base] = k == 0 ? d : 0.0f; e4c[base + 1] = k == 1 ? d : 0.0f; e4c[base + 12] = k == 2 ? d : 0.0f; e4c[base + 13] = k == 3 ? d : 0.0f;
}
// LConv::backward of conv2 as a gather (cnn.h:236-250) for input position (x, y) of one input channel: s_e [NOZ][144] the output channels' error
// maps, s_w [NOZ][16] their taps on that input channel; output channel, output y, output x ascending
template <int NOZ> __device__ __forceinline__ float t_conv2_back_gather(const float *s_w, const float *s_e, int x, int y)
{
	const int oy0 = max(0, y - 3), oy1 = min(11, y), ox0 = max(0, x - 3), ox1 = min(11, x);
	float acc = 0.0f;
	for (int oz = 0; oz < NOZ; oz++) for (int oy = oy0; oy <= oy1; oy++) for (int ox = ox0; ox <= ox1; ox++)
		acc += s_w[oz * 16 + (x - ox) + 4 * (y - oy)] * s_e[oz * 144 + oy * 12 + ox];
	return acc;
}
// LConv::update (cnn.h:252-279) of one conv1 channel for one sample.  The two max-pools pass conv1's error to one position per 4x4 window only, so
// it is a list of 225 (input position s_i, value after tanh' s_e) pairs over the input s_x [64][64]; eight lanes (sub) per tap share the list:
// taps 0..24, tap 25 = bias, 26..31 idle.  Adds a lane's share to acc; seg8_sum of acc finishes the tap (once per sample, or after several samples).
__device__ __forceinline__ float t_conv1_grad_add(float acc, const float *s_x, const int *s_i, const float *s_e, int tap, int sub)
{
	const int off = tap < 25 ? (tap / 5) * 64 + tap % 5 : 0;
	if (tap < 25) for (int p = sub; p < 225; p += 8) acc += s_x[s_i[p] + off] * s_e[p];
	else if (tap == 25) for (int p = sub; p < 225; p += 8) acc += s_e[p];
	return acc;
}
