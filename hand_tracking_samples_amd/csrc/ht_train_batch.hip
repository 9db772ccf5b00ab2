// ht_train_batch.hip -- one SGD step of the pose-initialiser CNN on a mini-batch: w' = w - alpha * sum_b g_b(w), every sample's gradient taken at
// the same weights.  g_b is what CNN::Train (third_party/cnn.h:558-580) subtracts for sample b, divided by alpha; the per-sample
// arithmetic is that of ht_train.hip: what the two steps compute alike is written once, in ht_train_shared.hpp.
//
// With n samples in a step the two fully connected layers are dense products, three per layer, on v_mfma_f32_32x32x2_f32:
//   forward        Y[b,j] = B[j] + sum_i X[b,i] W[i,j]            k_fc (ht_cnn.hip) on the row-major weights
//   backward-data  D[b,i] = sum_j E[b,j] W[i,j]  (old weights)     k_tb_fc_back: both operands contiguous along j, (1 - y^2) folded into the store
//   weight step    W[i,j] -= alpha * sum_b X[b,i] E[b,j]            k_tb_fc_wgrad: the batch is the summed index, the tile is applied in one read-modify-write
// so a matrix is read twice and rewritten once per step, not per sample.  A step is 13 launches:
//   sample indices | conv1+tanh+pool+pool | conv2+tanh+pool | FC1 | FC2 | softmax, loss, softmax' | FC2 back | FC2 step | FC1 back | FC1 step |
//   conv2 back | conv1/conv2 gradient partial sums over groups of four samples | their sum in group order, applied to W1 B1 W2 B2 and the packed W2p
// The convolutions keep, per pooling window, the pooled value and which entry won (the first maximum, cnn.h:150-160) instead of the unpooled maps:
// that is all the backward pass reads of them (tanh' = 1 - m^2 at the maximum m, the error goes to that entry alone).
// Every sum has a fixed order and there are no floating-point atomics: the same call on the same weights gives the same bits.
#include "ht_device.hpp"
#include "ht_launch.hpp"
#include "ht_train_shared.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define TB_GS 4                                  // samples per partial sum of the convolutions' gradients
#define TB_MAXG (HT_TRAIN_MAX_BATCH / TB_GS)
#define TB_PW (16384 + 64 + 16 * 26)             // floats of one partial sum: W2, B2, then 16 x (25 taps of W1 + B1)
struct tb_index { int v[HT_TRAIN_MAX_BATCH]; };

// the step's sample indices, handed over as a kernel argument (no host memory has to outlive the call)
__global__ __launch_bounds__(256) void k_tb_set_index(tb_index ix, int n, int *__restrict__ idx)
{
	if ((int)threadIdx.x < n) idx[threadIdx.x] = ix.v[threadIdx.x];
}
// conv1 + tanh (t_conv1_out) + the two max-pools (-> P2 x P2), k_t_conv1_tanh_pool per sample (blockIdx.z) for the net of input side S (cnn_dims).  Of the
// C1 x C1 map only the pooled value a3 and r1 = the input position (y * S + x) of the conv output that won both pools are kept.
template <int S> __global__ __launch_bounds__(256) void k_tb_conv1_tanh_pool(const float *__restrict__ pool, const int *__restrict__ idx, const float *__restrict__ W, const float *__restrict__ B, float *__restrict__ a3, int *__restrict__ r1)
{
	typedef cnn_dims<S> D;
	__shared__ float s_o[4][D::C1];
	const int py = blockIdx.x, oz = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
	const float *in = pool + (size_t)idx[b] * (S * S);
	for (int e = t; e < 4 * D::C1; e += 256)
	{
		const int r = e / D::C1, x = e % D::C1, y = 4 * py + r;
		s_o[r][x] = t_conv1_out<S>(in, W, B, oz, y, x);
	}
	__syncthreads();
	if (t < D::P2)
	{
		float q[4], m;
#pragma unroll
		for (int k = 0; k < 4; k++) { const int r = 2 * (k >> 1), c = 4 * t + 2 * (k & 1); float mk; first_max4(s_o[r][c], s_o[r][c + 1], s_o[r + 1][c], s_o[r + 1][c + 1], mk); q[k] = mk; }
		const int k2 = first_max4(q[0], q[1], q[2], q[3], m);
		const int r = 2 * (k2 >> 1), c = 4 * t + 2 * (k2 & 1);
		const int k1 = first_max4(s_o[r][c], s_o[r][c + 1], s_o[r + 1][c], s_o[r + 1][c + 1], m);
		const size_t o = (size_t)b * D::A3 + oz * D::NP2 + py * D::P2 + t;
		a3[o] = m; r1[o] = (4 * py + r + (k1 >> 1)) * S + c + (k1 & 1);
	}
}
// conv2 + tanh (t_conv2_out) + max-pool (-> P3 x P3), k_t_conv2_tanh_pool per sample (blockIdx.y) by NT threads; a6 = the pooled value,
// r3 = which of the window's four entries (x fastest) is its first maximum.  The whole a3 of the sample is staged (14 KB; 61.5 KB at S = 128)
template <int S, int NT> __global__ __launch_bounds__(NT) void k_tb_conv2_tanh_pool(const float *__restrict__ a3, const float *__restrict__ W, const float *__restrict__ B, float *__restrict__ a6, int *__restrict__ r3)
{
	typedef cnn_dims<S> D;
	__shared__ float s_in[D::A3], s_w[256], s_o[D::NC2];
	const int oz = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
	t_conv2_out<D::P2, NT>(a3 + (size_t)b * D::A3, W, B, oz, s_in, s_w, s_o);
	__syncthreads();
	for (int e = t; e < D::NP3; e += NT)
	{
		const float *p = s_o + (2 * (e / D::P3)) * D::C2 + 2 * (e % D::P3);
		float m;
		const int k = first_max4(p[0], p[1], p[D::C2], p[D::C2 + 1], m);
		a6[(size_t)b * D::A6 + oz * D::NP3 + e] = m; r3[(size_t)b * D::A6 + oz * D::NP3 + e] = k;
	}
}
// Output layer of sample b = blockIdx.x from its logits: chunked softmax (cnn.h:497-511), E = y - t, softmax backward (cnn.h:512-526) and the loss
// sum E^2 / 2304.  Thread t owns element t of each 256-wide chunk and element t of the 256 that form the sixteen 16-wide chunks.
__global__ __launch_bounds__(256) void k_tb_softmax_loss(const float *__restrict__ logits, const float *__restrict__ targets, const int *__restrict__ idx, float *__restrict__ e9, float *__restrict__ mse)
{
	__shared__ float red[2][8][4], rsq[4];
	const int b = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
	const float *lg = logits + (size_t)b * HT_CNN_OUT, *tg = targets + (size_t)idx[b] * HT_CNN_OUT;
	float v[9], cs[9];
#pragma unroll
	for (int c = 0; c < 9; c++)
	{
		v[c] = (float)exp((double)lg[c * 256 + t]);
		cs[c] = c < 8 ? wave_sum(v[c]) : seg16_sum(v[c]);
		if (c < 8 && lane == 0) red[0][c][w] = cs[c];
	}
	__syncthreads();
	float y[9], d[9], cd[9], sq = 0.0f;
#pragma unroll
	for (int c = 0; c < 9; c++)
	{
		if (c < 8) cs[c] = ((red[0][c][0] + red[0][c][1]) + red[0][c][2]) + red[0][c][3];
		y[c] = v[c] / cs[c]; d[c] = y[c] - tg[c * 256 + t];
		cd[c] = c < 8 ? wave_sum(d[c] * y[c]) : seg16_sum(d[c] * y[c]);
		if (c < 8 && lane == 0) red[1][c][w] = cd[c];
		sq += d[c] * d[c];
	}
	sq = wave_sum(sq);
	if (lane == 0) rsq[w] = sq;
	__syncthreads();
#pragma unroll
	for (int c = 0; c < 9; c++)
	{
		if (c < 8) cd[c] = ((red[1][c][0] + red[1][c][1]) + red[1][c][2]) + red[1][c][3];
		e9[(size_t)b * HT_CNN_OUT + c * 256 + t] = y[c] * (d[c] - cd[c]);
	}
	if (t == 0) mse[b] = (((rsq[0] + rsq[1]) + rsq[2]) + rsq[3]) / (float)HT_CNN_OUT;
}
// Backward-data of a fully connected layer for the whole step: D[b,i] = sum_j E[b,j] W[i,j] with W [R][K] row-major (R rows i, K columns j), times
// (1 - Y[b,i]^2) when FOLD (the tanh under the layer).  Block = 32 rows of W x all samples, 8 waves; wave w sums the columns [w K/8, (w+1) K/8) into
// NB 32x32 accumulator tiles (sample tile x row tile), so W is read once.  Both operands are contiguous along the summed index: a lane (r = lane & 31,
// h = lane >> 5) reads the four columns j0 + 8 s + 4 h + c of its row with one 128-bit load and component c feeds matrix instruction c, whose two
// k-slots are therefore columns (j0 + 8 s + c, j0 + 8 s + 4 + c) for A (= E) and B (= W^T) alike.  The eight waves' tiles are added in wave order through
// LDS.  C/D map of 32x32: column (here i) = lane & 31, row (here b) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
template <int NB, bool FOLD> __global__ __launch_bounds__(512) void k_tb_fc_back(const float *__restrict__ E, const float *__restrict__ W, const float *__restrict__ Y, float *__restrict__ D, int n, int R, int K)
{
	__shared__ float red[8][1024];
	const int t = threadIdx.x, w = t >> 6, lane = t & 63, r = lane & 31, h = lane >> 5;
	const int i0 = blockIdx.x * 32, kc = K / 8, j0 = w * kc + 4 * h;
	const float *wp = W + (size_t)(i0 + r) * K + j0;
	const float *ep[NB]; bool on[NB];
	f32x16 acc[NB];
#pragma unroll
	for (int q = 0; q < NB; q++)
	{
		on[q] = 32 * q + r < n;
		ep[q] = E + (size_t)(on[q] ? 32 * q + r : 0) * K + j0;
#pragma unroll
		for (int g = 0; g < 16; g++) acc[q][g] = 0.0f;
	}
#pragma unroll 2
	for (int s = 0; s < kc; s += 8)
	{
		const float4 wv = *reinterpret_cast<const float4 *>(wp + s);
#pragma unroll
		for (int q = 0; q < NB; q++)
		{
			float4 ev = *reinterpret_cast<const float4 *>(ep[q] + s);
			if (!on[q]) ev = make_float4(0, 0, 0, 0);
			acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ev.x, wv.x, acc[q], 0, 0, 0);
			acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ev.y, wv.y, acc[q], 0, 0, 0);
			acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ev.z, wv.z, acc[q], 0, 0, 0);
			acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ev.w, wv.w, acc[q], 0, 0, 0);
		}
	}
#pragma unroll
	for (int q = 0; q < NB; q++)
	{
		if (q) __syncthreads();
#pragma unroll
		for (int g = 0; g < 16; g++) red[w][g * 64 + lane] = acc[q][g];
		__syncthreads();
#pragma unroll
		for (int u = 0; u < 2; u++)
		{
			const int e = t + 512 * u, g = e >> 6, ln = e & 63;
			float v = red[0][e];
#pragma unroll
			for (int k = 1; k < 8; k++) v += red[k][e];
			const int b = 32 * q + (g & 3) + 8 * (g >> 2) + 4 * (ln >> 5);
			const size_t o = (size_t)b * R + i0 + (ln & 31);
			if (b < n) { if (FOLD) { const float y = Y[o]; v = (1.0f - y * y) * v; } D[o] = v; }
		}
	}
}
// Weight gradient and step of a fully connected layer: W[i,j] -= alpha * sum_b X[b,i] E[b,j], W [M][N] row-major.  The summed index is the sample:
// lanes 0..31 hold sample 2 s, lanes 32..63 sample 2 s + 1 (zero beyond n), as 32 consecutive floats of X (A operand, i) and of E (B operand, j).
// A wave owns one 32x32 tile of W, read before the products and rewritten once after them; a block is four tiles side by side, M N / 1024 tiles per
// matrix.  The blocks of the first tile row also step the bias, B[j] -= alpha * sum_b E[b,j], samples ascending.
__global__ __launch_bounds__(256) void k_tb_fc_wgrad(float *__restrict__ W, float *__restrict__ B, const float *__restrict__ X, const float *__restrict__ E, int n, int M, int N, float alpha)
{
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
	const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 128 + 32 * w;
	float *wp = W + (size_t)(i0 + 4 * h) * N + j0 + r;
	float wv[16];
#pragma unroll
	for (int g = 0; g < 16; g++) wv[g] = wp[(size_t)((g & 3) + 8 * (g >> 2)) * N];
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
#pragma unroll
	for (int g = 0; g < 16; g++) wp[(size_t)((g & 3) + 8 * (g >> 2)) * N] = wv[g] - alpha * acc[g];
	if (blockIdx.y == 0 && lane < 32)
	{
		float sum = 0.0f;
		for (int b = 0; b < n; b++) sum += ep[(size_t)b * N];
		B[j0 + r] -= alpha * sum;
	}
}
// LConv::backward of conv2 (t_conv2_back_gather) for the IZB input channels from IZB blockIdx.x of sample b = blockIdx.y, input rows [BH z, BH z + BH) (z = blockIdx.z):
// the rows of the 64 error maps that those positions read are rebuilt in LDS from the pooled error (conv2's tanh' at the kept maximum, then t_window_scatter to the
// kept entry), whole pooling windows: WR window rows from row pr0.  A thread owns an input position of one channel at a time.  S = 64: one channel and one band, the
// whole maps (36 KB); S = 128: bands of BH = 4 rows, eight map rows each (56 KB of the 196 KB that the whole maps would take), shared by IZB = 4 input channels, so
// that a sample's bands are rebuilt 32 times, not 128.
template <int S, int BH, int NT, int IZB> __global__ __launch_bounds__(NT) void k_tb_conv2_back(const float *__restrict__ a6, const int *__restrict__ r3, const float *__restrict__ e6, const float *__restrict__ W, float *__restrict__ e3)
{
	typedef cnn_dims<S> D;
	static_assert(BH >= D::P2 || BH % 2 == 0, "a band starts on an even input row");
	static_assert(16 % IZB == 0, "the input channels are dealt out evenly");
	constexpr int WR = BH >= D::P2 ? D::P3 : (BH + 4) / 2, ROWS = 2 * WR;
	__shared__ float s_e[64 * ROWS * D::C2], s_w[IZB * 64 * 16];
	const int iz0 = blockIdx.x * IZB, b = blockIdx.y, y0 = blockIdx.z * BH, t = threadIdx.x;
	const int pr0 = max(0, y0 - 3) / 2;
	for (int i = t; i < 64 * WR * D::P3; i += NT)
	{
		const int oz = i / (WR * D::P3), p = i % (WR * D::P3), py = pr0 + p / D::P3;
		if (py >= D::P3) continue;
		const size_t o = (size_t)b * D::A6 + oz * D::NP3 + py * D::P3 + p % D::P3;
		const float m = a6[o];
		t_window_scatter<D::C2>(s_e + oz * (ROWS * D::C2), p, r3[o], (1.0f - m * m) * e6[o]);
	}
	for (int i = t; i < IZB * 1024; i += NT) { const int j = i & 1023; s_w[i] = W[(j & 15) + 16 * (iz0 + (i >> 10) + 16 * (j >> 4))]; }
	__syncthreads();
	for (int e = t; e < IZB * BH * D::P2; e += NT)
	{
		const int q = e / (BH * D::P2), r = e % (BH * D::P2), x = r % D::P2, y = y0 + r / D::P2;
		if (y < D::P2) e3[(size_t)b * D::A3 + (iz0 + q) * D::NP2 + y * D::P2 + x] = t_conv2_back_gather<64, D::C2, ROWS>(s_w + q * 1024, s_e, x, y, 2 * pr0);
	}
}
// LConv::update (cnn.h:252-279) of both convolutions, summed over the TB_GS samples of group blockIdx.y into pw[group][TB_PW] (times -alpha).  Only one
// entry per pooling window carries an error, so both sums run over (position, value) lists, as k_t_conv_update's conv1 branch does.
// blocks 0..15: conv2, output channels 4 x .. 4 x + 3: a thread per tap (iz, ky, kx), NP3 windows per channel (36; 196 at S = 128) over the staged a3.
// blocks 16..31: conv1, output channel x - 16: t_conv1_grad_add per sample over the staged input, the eight lanes of a tap added once after the group's samples.
template <int S> __global__ __launch_bounds__(256) void k_tb_conv_grad(const float *__restrict__ pool, const int *__restrict__ idx, const float *__restrict__ a3, const int *__restrict__ r1, const float *__restrict__ a6, const int *__restrict__ r3,
                                                                       const float *__restrict__ e6, const float *__restrict__ e3, int n, float alpha, float *__restrict__ pw)
{
	typedef cnn_dims<S> D;
	constexpr int NL = ((4 * D::NP3 > D::NP2 ? 4 * D::NP3 : D::NP2) + 255) & ~255;      // the longer list: 4 channels' windows of conv2, a channel's of conv1
	__shared__ float s_x[S * S], s_e[NL];
	__shared__ int s_i[NL];
	static_assert(D::A3 <= S * S, "a3 is staged where the input is");
	const int t = threadIdx.x, b0 = blockIdx.y * TB_GS, b1 = min(n, b0 + TB_GS);
	float *out = pw + (size_t)blockIdx.y * TB_PW;
	if (blockIdx.x < 16)
	{
		const int g = blockIdx.x, kx = t & 3, ky = (t >> 2) & 3, iz = t >> 4;
		float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, bias = 0.0f;
		for (int b = b0; b < b1; b++)
		{
			__syncthreads();
			for (int i = t; i < D::A3; i += 256) s_x[i] = a3[(size_t)b * D::A3 + i];
			for (int e = t; e < 4 * D::NP3; e += 256)
			{
				const size_t o = (size_t)b * D::A6 + g * (4 * D::NP3) + e;
				const int p = e % D::NP3, k = r3[o];
				const float m = a6[o];
				s_i[e] = (2 * (p / D::P3) + (k >> 1)) * D::P2 + 2 * (p % D::P3) + (k & 1);
				s_e[e] = -alpha * ((1.0f - m * m) * e6[o]);
			}
			__syncthreads();
			const float *xp = s_x + iz * D::NP2 + ky * D::P2 + kx;
#pragma unroll
			for (int oz = 0; oz < 4; oz++)
#pragma unroll 4
				for (int p = 0; p < D::NP3; p++) acc[oz] += xp[s_i[oz * D::NP3 + p]] * s_e[oz * D::NP3 + p];
			if (t < 4) for (int p = 0; p < D::NP3; p++) bias += s_e[t * D::NP3 + p];
		}
#pragma unroll
		for (int oz = 0; oz < 4; oz++) out[(4 * g + oz) * 256 + t] = acc[oz];
		if (t < 4) out[16384 + 4 * g + t] = bias;
	}
	else
	{
		const int oz = blockIdx.x - 16, tap = t >> 3, sub = t & 7;
		float acc = 0.0f;
		for (int b = b0; b < b1; b++)
		{
			__syncthreads();
			const float *x0 = pool + (size_t)idx[b] * (S * S);
			for (int i = t; i < S * S; i += 256) s_x[i] = x0[i];
			for (int e = t; e < D::NP2; e += 256)
			{
				const size_t o = (size_t)b * D::A3 + oz * D::NP2 + e;
				const float m = a3[o];
				s_i[e] = r1[o];
				s_e[e] = -alpha * ((1.0f - m * m) * e3[o]);
			}
			__syncthreads();
			acc = t_conv1_grad_add<S, D::NP2>(acc, s_x, s_i, s_e, tap, sub);
		}
		acc = seg8_sum(acc);
		if (sub == 0 && tap < 26) out[16448 + oz * 26 + tap] = acc;
	}
}
// the groups' partial sums added in group order and applied: W2 (with the MFMA-packed copy k_conv2 reads, cnn_w2p_index), B2, W1, B1
__global__ __launch_bounds__(256) void k_tb_conv_apply(const float *__restrict__ pw, int groups, float *__restrict__ W1, float *__restrict__ B1, float *__restrict__ W2, float *__restrict__ B2, float *__restrict__ W2p)
{
	const int e = blockIdx.x * 256 + threadIdx.x;
	if (e >= TB_PW) return;
	float sum = 0.0f;
	for (int g = 0; g < groups; g++) sum += pw[(size_t)g * TB_PW + e];
	if (e < 16384)
	{
		const int oz = e >> 8, t = e & 255, kx = t & 3, ky = (t >> 2) & 3, iz = t >> 4;
		const float w = W2[e] + sum;
		W2[e] = w; W2p[cnn_w2p_index(oz, iz, ky, kx)] = w;
	}
	else if (e < 16448) B2[e - 16384] += sum;
	else
	{
		const int q = e - 16448, oz = q / 26, tap = q % 26;
		if (tap < 25) W1[oz * 25 + tap] += sum; else B1[oz] += sum;
	}
}

// The arena of a step of up to cap samples (cap a multiple of 32) of the net of dimensions d: per-sample tensors [cap][...], then the partial sums, the
// indices and a sink for the losses
struct tb_arena { float *a3, *a6, *a8, *lg, *e9, *e7, *e6, *e3, *pw, *sink; int *r1, *r3, *idx; };
static tb_arena tb_layout(float *p, size_t cap, const ht_net_dims &d)
{
	const size_t n3 = d.act1, n6 = d.act2;
	tb_arena A;
	A.a3 = p; p += cap * n3; A.r1 = (int *)p; p += cap * n3; A.a6 = p; p += cap * n6; A.r3 = (int *)p; p += cap * n6; A.a8 = p; p += cap * 2048;
	A.lg = p; p += cap * 2304; A.e9 = p; p += cap * 2304; A.e7 = p; p += cap * 2048; A.e6 = p; p += cap * n6; A.e3 = p; p += cap * n3;
	A.pw = p; p += (size_t)TB_MAXG * TB_PW; A.sink = p; p += HT_TRAIN_MAX_BATCH; A.idx = (int *)p;
	return A;
}
size_t ht_train_batch_floats(int cap, const ht_net_dims &d) { return (size_t)cap * (3 * d.act1 + 3 * d.act2 + 2 * 2304 + 2 * 2048) + (size_t)TB_MAXG * TB_PW + 2 * HT_TRAIN_MAX_BATCH; }
// the per-sample tensors ht_debug_train_batch_buffers returns, in its order: a3 a6 a8 e9 e7 e6 e3, and the floats of each per sample
void ht_train_batch_views(float *arena, int cap, const float *view[7], size_t per[7], const ht_net_dims &d)
{
	const tb_arena A = tb_layout(arena, (size_t)cap, d);
	view[0] = A.a3; view[1] = A.a6; view[2] = A.a8; view[3] = A.e9; view[4] = A.e7; view[5] = A.e6; view[6] = A.e3;
	per[0] = d.act1; per[1] = d.act2; per[2] = 2048; per[3] = 2304; per[4] = 2048; per[5] = d.act2; per[6] = d.act1;
}
template <bool FOLD> static void tb_fc_back(const float *E, const float *W, const float *Y, float *D, int n, int R, int K, hipStream_t s)
{
	const dim3 g(R / 32), t(512);
	if (n <= 32) hipLaunchKernelGGL((k_tb_fc_back<1, FOLD>), g, t, 0, s, E, W, Y, D, n, R, K);
	else if (n <= 64) hipLaunchKernelGGL((k_tb_fc_back<2, FOLD>), g, t, 0, s, E, W, Y, D, n, R, K);
	else if (n <= 128) hipLaunchKernelGGL((k_tb_fc_back<4, FOLD>), g, t, 0, s, E, W, Y, D, n, R, K);
	else hipLaunchKernelGGL((k_tb_fc_back<8, FOLD>), g, t, 0, s, E, W, Y, D, n, R, K);
}
// One step of the net of input side S on samples index[0..n) of the pools; C2T = threads of a conv2 block, BH / BT / IZB = band height, threads and input channels per block of conv2's backward
// G: null for the step; else the weights are left alone and the three weight launches write G = (accumulate ? G : 0) + sum_b g_b(w) in .cnnb order instead (ht_optim.hip;
// k_tb_conv_grad at alpha = -1 forms the plain sums, -(-1) * x being x).  Everything before them is the same launch either way.
template <int S, int C2T, int BH, int BT, int IZB> static void tb_step(float *w, float *W2p, const float *inputs, const float *targets, const int *index, int n, float alpha, float *arena, int cap, float *mse_out, hipStream_t s,
                                                                       float *G = nullptr, int accumulate = 0)
{
	typedef cnn_dims<S> D;
	const tb_arena A = tb_layout(arena, (size_t)cap, ht_net_dims_of<S>());
	const cnnb_layout<float> L = cnnb_layout_of(w, (size_t)D::A6), LG = G ? cnnb_layout_of(G, (size_t)D::A6) : cnnb_layout<float>{};
	tb_index ix;
	for (int b = 0; b < n; b++) ix.v[b] = index[b];
	for (int b = n; b < HT_TRAIN_MAX_BATCH; b++) ix.v[b] = 0;
	const int groups = (n + TB_GS - 1) / TB_GS;
	hipLaunchKernelGGL(k_tb_set_index, dim3(1), dim3(256), 0, s, ix, n, A.idx);
	// forward
	hipLaunchKernelGGL(k_tb_conv1_tanh_pool<S>, dim3(D::P2, 16, n), dim3(256), 0, s, inputs, A.idx, L.W1, L.B1, A.a3, A.r1);
	hipLaunchKernelGGL((k_tb_conv2_tanh_pool<S, C2T>), dim3(64, n), dim3(C2T), 0, s, A.a3, L.W2, L.B2, A.a6, A.r3);
	ht_launch_fc_rowmajor(A.a6, L.W3, L.B3, A.a8, n, 2048, D::A6, true, s);
	ht_launch_fc_rowmajor(A.a8, L.W4, L.B4, A.lg, n, 2304, 2048, false, s);
	hipLaunchKernelGGL(k_tb_softmax_loss, dim3(n), dim3(256), 0, s, A.lg, targets, A.idx, A.e9, mse_out ? mse_out : A.sink);
	// backward with the old weights, then each layer's step
	tb_fc_back<true>(A.e9, L.W4, A.a8, A.e7, n, 2048, 2304, s);
	if (G) ht_launch_opt_fc_wgrad(LG.W4, LG.B4, A.a8, A.e9, n, 2048, 2304, accumulate, s);
	else hipLaunchKernelGGL(k_tb_fc_wgrad, dim3(2304 / 128, 2048 / 32), dim3(256), 0, s, L.W4, L.B4, A.a8, A.e9, n, 2048, 2304, alpha);
	tb_fc_back<false>(A.e7, L.W3, nullptr, A.e6, n, D::A6, 2048, s);
	if (G) ht_launch_opt_fc_wgrad(LG.W3, LG.B3, A.a6, A.e7, n, D::A6, 2048, accumulate, s);
	else hipLaunchKernelGGL(k_tb_fc_wgrad, dim3(2048 / 128, D::A6 / 32), dim3(256), 0, s, L.W3, L.B3, A.a6, A.e7, n, D::A6, 2048, alpha);
	hipLaunchKernelGGL((k_tb_conv2_back<S, BH, BT, IZB>), dim3(16 / IZB, n, (D::P2 + BH - 1) / BH), dim3(BT), 0, s, A.a6, A.r3, A.e6, L.W2, A.e3);
	hipLaunchKernelGGL(k_tb_conv_grad<S>, dim3(32, groups), dim3(256), 0, s, inputs, A.idx, A.a3, A.r1, A.a6, A.r3, A.e6, A.e3, n, G ? -1.0f : alpha, A.pw);
	if (G) ht_launch_opt_conv_reduce(A.pw, groups, TB_PW, LG.W1, LG.B1, LG.W2, LG.B2, accumulate, s);
	else hipLaunchKernelGGL(k_tb_conv_apply, dim3((TB_PW + 255) / 256), dim3(256), 0, s, A.pw, groups, L.W1, L.B1, L.W2, L.B2, W2p);
}
// One step on samples index[0..n) of the pools ([..][side side] inputs); mse_out[n] or null.  The packed copy of the last layer is NOT refreshed here (once per
// call: ht_api.hip).  d: the dimensions of one of the context's nets (ht_net_of).
void ht_launch_train_batch_step(float *w, float *W2p, const float *inputs, const float *targets, const int *index, int n, float alpha, float *arena, int cap, float *mse_out, hipStream_t s, const ht_net_dims &d)
{
	if (d.side == 128) tb_step<128, 256, 4, 256, 4>(w, W2p, inputs, targets, index, n, alpha, arena, cap, mse_out, s);
	else tb_step<64, 192, 15, 256, 1>(w, W2p, inputs, targets, index, n, alpha, arena, cap, mse_out, s);
}
// The gradient of the same samples at the weights w, which are only read: G [d.count] in .cnnb order = (accumulate ? G : 0) + sum_b g_b(w)
void ht_launch_train_batch_grad(const float *w, float *G, int accumulate, const float *inputs, const float *targets, const int *index, int n, float *arena, int cap, float *mse_out, hipStream_t s, const ht_net_dims &d)
{
	float *wr = const_cast<float *>(w);      // tb_step with a G writes neither the weights nor W2p
	if (d.side == 128) tb_step<128, 256, 4, 256, 4>(wr, nullptr, inputs, targets, index, n, 0.0f, arena, cap, mse_out, s, G, accumulate);
	else tb_step<64, 192, 15, 256, 1>(wr, nullptr, inputs, targets, index, n, 0.0f, arena, cap, mse_out, s, G, accumulate);
}
