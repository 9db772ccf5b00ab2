// ht_train.hip -- one SGD step of the pose-initialiser CNN per sample.
//
// Reference computations (third_party/cnn.h): CNN::Train :558-580 (forward keeping every layer's output, E = y - t, backward() of
// layers 10..1 with the weights as they are, then update() of every layer), LConv :205-279, LMaxPool :141-164, LFull :405-445,
// LActivation<TanH> :457-469 (df = 1 - y*y), LSoftMaxChunked :497-526.  Topology: include/handtrack.h:108-118.
//
// Batch-1 SGD is sequential over samples, so the parallelism is inside one sample, and the two fully connected layers (2 x 18.9 MB of
// weights) make a step HBM-bound: the forward product streams each matrix once (rows split 32 ways, partial sums reduced in a fixed
// order), and the backward product and the weight update of a layer share one pass over its matrix (row i yields d[i] = W[i,:].E with
// the old weights and is then rewritten as W[i,:] - x[i]*E*alpha): 113 MB of traffic per sample.  Everything else is fused around
// those four passes so that a step is 9 launches:
//   conv1+tanh+pool+pool | conv2+tanh+pool | FC1 partial | (reduce+tanh of FC1) FC2 partial | reduce+softmax+loss+softmax' |
//   FC2 back+update (+bias, tanh', loss value) | FC1 back+update (+bias) | (pool', tanh') conv2 back |
//   (pool', pool', tanh') conv1 update, (pool', tanh') conv2 update + the MFMA-packed copy of conv2 the inference kernel reads
// The error that reaches conv1's update is non-zero at one position per 4x4 pooling window only (the two max-pools route it to the first
// maximum), so it is handled as a compact (position, value) list instead of three dense maps.
// Sums are reduced in parallel (fixed order, deterministic), so results agree with the reference to float rounding, not bit for bit.
#include "ht_device.hpp"
#include "ht_launch.hpp"
#include "ht_train_shared.hpp"

__device__ __forceinline__ float max4(float a, float b, float c, float d) { return fmax_std(fmax_std(fmax_std(a, b), c), d); }

// conv1 + tanh (t_conv1_out) + the two max-pools (-> 30x30 -> 15x15).  Block (py, oz): four output rows of one channel, one thread per output;
// the first 15 threads then pool the 4x60 strip.
__global__ __launch_bounds__(256) void k_t_conv1_tanh_pool(const float *__restrict__ in, const float *__restrict__ W, const float *__restrict__ B, float *__restrict__ a1, float *__restrict__ a3)
{
	__shared__ float s_o[4][60];
	const int py = blockIdx.x, oz = blockIdx.y, t = threadIdx.x;
	if (t < 240)
	{
		const int r = t / 60, x = t % 60, y = 4 * py + r;
		const float o = t_conv1_out(in, W, B, oz, y, x);
		a1[oz * 3600 + y * 60 + x] = o; s_o[r][x] = o;
	}
	__syncthreads();
	if (t < 15)
	{
		float q[4];
#pragma unroll
		for (int k = 0; k < 4; k++) { const int r = 2 * (k >> 1), c = 4 * t + 2 * (k & 1); q[k] = max4(s_o[r][c], s_o[r][c + 1], s_o[r + 1][c], s_o[r + 1][c + 1]); }
		a3[oz * 225 + py * 15 + t] = max4(q[0], q[1], q[2], q[3]);
	}
}
// conv2 + tanh (t_conv2_out) + max-pool (-> 6x6): one block per output channel
__global__ __launch_bounds__(192) void k_t_conv2_tanh_pool(const float *__restrict__ a3, const float *__restrict__ W, const float *__restrict__ B, float *__restrict__ a5, float *__restrict__ a6)
{
	__shared__ float s_in[3600], s_w[256], s_o[144];
	const int oz = blockIdx.x, t = threadIdx.x;
	const float o = t_conv2_out(a3, W, B, oz, s_in, s_w, s_o);
	if (t < 144) a5[oz * 144 + t] = o;
	__syncthreads();
	if (t < 36) { const float *p = s_o + (2 * (t / 6)) * 12 + 2 * (t % 6); a6[oz * 36 + t] = max4(p[0], p[1], p[12], p[13]); }
}
// y[j] = B[j] + sum_i x[i] W[i][j].  Block (jb, ks): rows [ks*M/32, (ks+1)*M/32) of 256 consecutive columns; wave w takes every fourth
// row of the slab, a lane four columns (128-bit loads); the four waves' sums are added in wave order.  part[ks][j].
// XPART: x is the tanh of the previous layer's output, still in partial sums xpart[32][M] + xb: the block reduces the slab's rows itself
// (and column-block 0 keeps them in xout for the backward pass).
#define T_KSPLIT 32
template <bool XPART> __global__ __launch_bounds__(256) void k_t_fc_partial(const float *__restrict__ x, const float *__restrict__ xpart, const float *__restrict__ xb, float *__restrict__ xout,
                                                                           const float *__restrict__ W, float *__restrict__ part, int M, int N)
{
	__shared__ float4 s_acc[4][64];
	__shared__ float s_x[72];
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = blockIdx.x * 256 + 4 * lane, ks = blockIdx.y, rows = M / T_KSPLIT;
	const int i0 = ks * rows;
	if (threadIdx.x < rows)
	{
		const int i = i0 + threadIdx.x;
		float v;
		if (XPART)
		{
			float acc = xb[i];
#pragma unroll 8
			for (int k = 0; k < T_KSPLIT; k++) acc += xpart[(size_t)k * M + i];
			v = t_tanh(acc);
			if (blockIdx.x == 0) xout[i] = v;
		}
		else v = x[i];
		s_x[threadIdx.x] = v;
	}
	__syncthreads();
	float4 acc = make_float4(0, 0, 0, 0);
#pragma unroll 6
	for (int r = w; r < rows; r += 4)
	{
		const float xi = s_x[r];
		const float4 ww = *reinterpret_cast<const float4 *>(W + (size_t)(i0 + r) * N + j);
		acc.x += xi * ww.x; acc.y += xi * ww.y; acc.z += xi * ww.z; acc.w += xi * ww.w;
	}
	s_acc[w][lane] = acc;
	__syncthreads();
	if (w == 0)
	{
		for (int k = 1; k < 4; k++) { const float4 o = s_acc[k][lane]; acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w; }
		*reinterpret_cast<float4 *>(part + (size_t)ks * N + j) = acc;
	}
}
// Output layer: reduce FC2's partial sums, chunked softmax forward (cnn.h:497-511), E = y - t, softmax backward (cnn.h:512-526).
// Blocks 0..7 own the eight 256-wide chunks (a thread per element), block 8 the sixteen 16-wide ones; sqp[block] = its sum of E^2.
__global__ __launch_bounds__(256) void k_t_softmax_loss(const float *__restrict__ part, const float *__restrict__ B, const float *__restrict__ target, float *__restrict__ e9, float *__restrict__ sqp)
{
	__shared__ float red[3][4];
	const int t = threadIdx.x, w = t >> 6, lane = t & 63, i = blockIdx.x * 256 + t;
	const bool wide = blockIdx.x < 8;
	float acc = B[i];
#pragma unroll 8
	for (int k = 0; k < T_KSPLIT; k++) acc += part[(size_t)k * HT_CNN_OUT + i];
	const float v = (float)exp((double)acc);
	float cs = wide ? wave_sum(v) : seg16_sum(v);
	if (lane == 0) red[0][w] = cs;
	__syncthreads();
	if (wide) cs = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
	const float y = v / cs, d = y - target[i];
	float cd = wide ? wave_sum(d * y) : seg16_sum(d * y);
	const float sq = wave_sum(d * d);
	if (lane == 0) { red[1][w] = cd; red[2][w] = sq; }
	__syncthreads();
	if (wide) cd = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
	e9[i] = y * (d - cd);
	if (t == 0) sqp[blockIdx.x] = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
}
// One wave per row i of a fully connected layer: d = W[i,:].E with the old weights, then W[i,:] -= X[i]*E*alpha (cnn.h:430-445).
// OUTPUT (the layer under the softmax): X is the output of a tanh layer whose backward is folded in, D[i] = (1 - X[i]^2) d, and the
// first thread finishes the loss value CNN::Train returns.  The first blocks also step the bias.
template <bool OUTPUT> __global__ __launch_bounds__(256) void k_t_fc_back_update(float *__restrict__ W, float *__restrict__ B, const float *__restrict__ X, const float *__restrict__ E, float *__restrict__ D, int M, int N, float alpha,
                                                                                const float *__restrict__ sqp, float *__restrict__ mse_out)
{
	const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	{ const int j = blockIdx.x * 256 + threadIdx.x; if (j < N) B[j] -= E[j] * alpha; }
	if (OUTPUT && blockIdx.x == 0 && threadIdx.x == 0) { float m = 0.0f; for (int k = 0; k < 9; k++) m += sqp[k]; *mse_out = m / (float)HT_CNN_OUT; }
	if (i >= M) return;
	float *w = W + (size_t)i * N;
	const float xi = X[i];
	float acc = 0.0f;
#pragma unroll 3
	for (int j = 4 * lane; j < N; j += 256)
	{
		const float4 ww = *reinterpret_cast<const float4 *>(w + j), ee = *reinterpret_cast<const float4 *>(E + j);
		acc += ww.x * ee.x; acc += ww.y * ee.y; acc += ww.z * ee.z; acc += ww.w * ee.w;
		*reinterpret_cast<float4 *>(w + j) = make_float4(ww.x - xi * ee.x * alpha, ww.y - xi * ee.y * alpha, ww.z - xi * ee.z * alpha, ww.w - xi * ee.w * alpha);
	}
	acc = wave_sum(acc);
	if (lane == 0) D[i] = OUTPUT ? (1.0f - xi * xi) * acc : acc;
}
// third max-pool backward + conv2's tanh backward for pooled element p of channel oz: the first maximum of the 2x2 window, found in a5, takes
// the error times scale (t_window_scatter)
__device__ __forceinline__ void pool3_back_tanh(const float *__restrict__ a5, const float *__restrict__ e6, int oz, int p, float scale, float *__restrict__ e4c)
{
	const float *a = a5 + oz * 144 + (2 * (p / 6)) * 12 + 2 * (p % 6);
	float m;
	const int k = first_max4(a[0], a[1], a[12], a[13], m);
	t_window_scatter(e4c, p, k, scale * ((1.0f - m * m) * e6[oz * 36 + p]));
}
// LConv::backward of conv2 (t_conv2_back_gather).  Block (iz, g): input channel iz, output channels [4g, 4g+4), whose error maps
// are rebuilt in LDS from the pooled error; a thread owns one input position.
#define T_CB_GROUPS 16
__global__ __launch_bounds__(256) void k_t_conv2_back(const float *__restrict__ a5, const float *__restrict__ e6, const float *__restrict__ W, float *__restrict__ part3)
{
	__shared__ float s_e[4 * 144], s_w[4 * 16];
	const int iz = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
	if (t < 144) pool3_back_tanh(a5, e6, 4 * g + t / 36, t % 36, 1.0f, s_e + (t / 36) * 144);
	if (t < 64) { const int oz = t >> 4, k = t & 15; s_w[t] = W[k + 16 * (iz + 16 * (4 * g + oz))]; }
	__syncthreads();
	if (t >= 225) return;
	part3[g * 3600 + iz * 225 + t] = t_conv2_back_gather<4>(s_w, s_e, t % 15, t / 15);
}
// LConv::update (cnn.h:252-279) of both convolutions in one launch.
// blocks 0..63: conv2, output channel = block, a thread per tap walks the 144 output positions in the reference's order, then the
//               MFMA-packed copy (cnn_w2p_index) k_conv2 reads is refreshed;
// blocks 64..79: conv1, output channel = block - 64: the block first finds the 225 (position, value after tanh') pairs that carry conv1's
//               error, then eight lanes per tap share them (t_conv1_grad_add).
__global__ __launch_bounds__(256) void k_t_conv_update(const float *__restrict__ x0, const float *__restrict__ a1, const float *__restrict__ a3, const float *__restrict__ a5, const float *__restrict__ e6, const float *__restrict__ part3,
                                                       float *__restrict__ W1, float *__restrict__ B1, float *__restrict__ W2, float *__restrict__ B2, float *__restrict__ W2p, float alpha)
{
	__shared__ float s_x[4096], s_e[256];
	__shared__ int s_i[256];
	const int t = threadIdx.x;
	if (blockIdx.x < 64)
	{
		const int oz = blockIdx.x;
		for (int i = t; i < 3600; i += 256) s_x[i] = a3[i];
		if (t < 36) pool3_back_tanh(a5, e6, oz, t, -alpha, s_e);
		__syncthreads();
		const int kx = t & 3, ky = (t >> 2) & 3, iz = t >> 4;
		float w = W2[oz * 256 + t];
		const float *xp = s_x + iz * 225 + ky * 15 + kx;
		for (int y = 0; y < 12; y++)
#pragma unroll
			for (int x = 0; x < 12; x++) w += xp[y * 15 + x] * s_e[y * 12 + x];
		W2[oz * 256 + t] = w;
		W2p[cnn_w2p_index(oz, iz, ky, kx)] = w;
		if (t == 0) { float bb = B2[oz]; for (int p = 0; p < 144; p++) bb += s_e[p]; B2[oz] = bb; }
	}
	else
	{
		const int oz = blockIdx.x - 64;
		for (int i = t; i < 4096; i += 256) s_x[i] = x0[i];
		if (t < 225)
		{
			const int x = t % 15, y = t / 15, i = oz * 225 + t;
			const float *p = a1 + oz * 3600 + (4 * y) * 60 + 4 * x;
			float q[4], m;
#pragma unroll
			for (int k = 0; k < 4; k++) { const float *r = p + (k >> 1) * 120 + (k & 1) * 2; q[k] = max4(r[0], r[1], r[60], r[61]); }
			const int k2 = first_max4(q[0], q[1], q[2], q[3], m);
			const float *r = p + (k2 >> 1) * 120 + (k2 & 1) * 2;
			const int k1 = first_max4(r[0], r[1], r[60], r[61], m);
			float e3 = 0.0f;
#pragma unroll
			for (int g = 0; g < T_CB_GROUPS; g++) e3 += part3[g * 3600 + i];
			s_i[t] = (4 * y + 2 * (k2 >> 1) + (k1 >> 1)) * 64 + 4 * x + 2 * (k2 & 1) + (k1 & 1);
			s_e[t] = -alpha * ((1.0f - m * m) * e3);
		}
		__syncthreads();
		const int tap = t >> 3, sub = t & 7;
		const float acc = seg8_sum(t_conv1_grad_add(0.0f, s_x, s_i, s_e, tap, sub));
		if (sub == 0 && tap < 25) W1[oz * 25 + tap] += acc;
		if (sub == 0 && tap == 25) B1[oz] += acc;
	}
}

// act: layer outputs kept for the backward pass; err: errors and conv2-backward partial sums; part: FC1's and FC2's partial sums
void ht_launch_train_step(float *w, float *W2p, const float *x, const float *target, float alpha, float *act, float *err, float *part, float *mse_out, hipStream_t s)
{
	float *a1 = act, *a3 = a1 + 57600, *a5 = a3 + cnn_dims<64>::A3, *a6 = a5 + 9216, *a8 = a6 + 2304;
	float *e9 = err, *e7 = e9 + 2304, *e6 = e7 + 2048, *part3 = e6 + 2304, *sqp = part3 + T_CB_GROUPS * cnn_dims<64>::A3;
	float *part1 = part, *part2 = part + (size_t)T_KSPLIT * 2048;
	const cnnb_layout<float> L = cnnb_layout_of(w);
	// forward
	hipLaunchKernelGGL(k_t_conv1_tanh_pool, dim3(15, 16), dim3(256), 0, s, x, L.W1, L.B1, a1, a3);
	hipLaunchKernelGGL(k_t_conv2_tanh_pool, dim3(64), dim3(192), 0, s, a3, L.W2, L.B2, a5, a6);
	hipLaunchKernelGGL(k_t_fc_partial<false>, dim3(2048 / 256, T_KSPLIT), dim3(256), 0, s, a6, nullptr, nullptr, nullptr, L.W3, part1, 2304, 2048);
	hipLaunchKernelGGL(k_t_fc_partial<true>, dim3(2304 / 256, T_KSPLIT), dim3(256), 0, s, nullptr, part1, L.B3, a8, L.W4, part2, 2048, 2304);
	hipLaunchKernelGGL(k_t_softmax_loss, dim3(9), dim3(256), 0, s, part2, L.B4, target, e9, sqp);
	// backward with the old weights, each layer's update in the same pass
	hipLaunchKernelGGL(k_t_fc_back_update<true>, dim3(2048 / 4), dim3(256), 0, s, L.W4, L.B4, a8, e9, e7, 2048, 2304, alpha, sqp, mse_out);
	hipLaunchKernelGGL(k_t_fc_back_update<false>, dim3(2304 / 4), dim3(256), 0, s, L.W3, L.B3, a6, e7, e6, 2304, 2048, alpha, nullptr, nullptr);
	hipLaunchKernelGGL(k_t_conv2_back, dim3(16, T_CB_GROUPS), dim3(256), 0, s, a5, e6, L.W2, part3);
	hipLaunchKernelGGL(k_t_conv_update, dim3(80), dim3(256), 0, s, x, a1, a3, a5, e6, part3, L.W1, L.B1, L.W2, L.B2, W2p, alpha);
}
size_t ht_train_act_floats() { return 57600 + cnn_dims<64>::A3 + 9216 + 2304 + 2048; }
size_t ht_train_err_floats() { return 2304 + 2048 + 2304 + T_CB_GROUPS * cnn_dims<64>::A3 + 16; }
size_t ht_train_part_floats() { return (size_t)T_KSPLIT * (2048 + 2304); }
