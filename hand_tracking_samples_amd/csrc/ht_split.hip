// ht_split.hip -- two hands in one frame: the blobs of a depth frame, the two largest, which of them is the right hand, and one masked frame per hand (an addition;
// DESIGN section 27).  All of it integers on u16 pixels (W4 = w / 4, H4 = h / 4, the size rule ht_segment_vr_supported's):
//   quarter image   Q[Y][X] = the minimum of the 4x4 block of input pixels (DownSampleMin twice, handtrack.h:285)
//   foreground      range_lo <= Q < range_hi
//   connectivity    4-neighbours, both foreground, |Qa - Qb| <= max_step
//   label           the smallest raster index Y * W4 + X of a cell's component; background cells 0xFFFF
//   selection       components of at least min_pixels cells are eligible (n_components counts them); the two with the most cells, a tie to the smaller label
//   left / right    a is LOWER than b iff sum_x_a * count_b < sum_x_b * count_a (64-bit; a tie to the smaller label).  HT_SPLIT_RIGHT_IS_LOW_X clear: the higher one is the
//                   right hand; set: the lower one.  A single eligible component is low iff 2 * sum_x < count * (W4 - 1) and becomes the hand the flag puts on that side
//   frames          out[k][y][x] = in[y][x] where label[y/4][x/4] is hand k's, `far` elsewhere (k = 0 right, 1 left; an absent hand's frame is all far); with
//                   HT_SPLIT_MIRROR_LEFT frame 1 is written mirrored, out[1][y][x] = masked[y][w-1-x], and its camera is the mirrored camera (section 26)
//   info [2][8]     count (0 = absent), label (0xFFFF when absent), sum_x, sum_y, min_x, min_y, max_x, max_y in cells (zeros when absent)
//
// Mapping.
//   k_split_label   one block of 1024 threads per frame; Q and the labels as u16 in LDS (2 x 38400 bytes at 640x480: two blocks a CU).  Thread t owns cells t, t + 1024, ...
//                   Labels are parent links of a union-find forest, always lab[i] <= i and a cell of i's own component:
//                     1. rows    lab[i] = i - 1 if i is connected to its left neighbour, else i; eight rounds of lab[i] = lab[lab[i]] make it the start of i's horizontal
//                                run (a run is at most 160 cells <= 2^8).
//                     2. columns every cell connected to the cell above it unites the two runs' trees: the larger root is hung under the smaller with a 16-bit minimum on
//                                its parent link (a compare-and-swap on the LDS word that holds two links).  No plain store runs in this phase.
//                     3. flatten lab[i] = lab[lab[i]] with a barrier between rounds until nothing changes: the root of a tree is its smallest index, the canonical label.
//                   Every loop ends by construction -- links only ever decrease and are bounded below by 0: a find walks strictly down (at most n hops); in a union the larger
//                   of the two roots strictly decreases from one iteration to the next (at most n iterations); a compare-and-swap is retried only after another lane lowered
//                   a link of the same word, of which there are finitely many; flattening halves every depth per round, at most ceil(log2 19200) + 1 = 16 rounds (the loop
//                   is capped at 32).  Counts: Q's storage is dead by then and takes 16-bit counters per label, two to a word, by LDS atomic adds (a count is at most
//                   19200, so no carry crosses).  Selection: two block-wide arg-max reductions on the key (count << 16) | (0xFFFF - label).  The two chosen components'
//                   sums and boxes by integer LDS atomics: order-free, exact.
//   k_split_write<N> a byte mover in the manner of k_mirror_frames: one thread moves N dwords = 2N pixels of a row with one load (16 / 8 / 4 bytes as width and alignment
//                   allow, k_split_write<0>: single pixels), masks them against both hands' labels (one label read per 4-pixel group) and stores both frames, the left
//                   one reversed in registers at the mirrored place of the row.
//   k_split_cams    [B][12] -> [B][2][12]: the frame's camera, and for k = 1 its mirror image (ht_mirror_cam_word, ht_mirror.hpp).
#include <string.h>
#include "ht_host.hpp"
#include "ht_frame_vec.hpp"
#include "ht_mirror.hpp"

#define SP_THREADS 1024
#define SP_MAXCELLS 19200
#define SP_WTHREADS 256
#define SP_NONE 0xFFFFu
#define SP_FLAGS (HT_SPLIT_RIGHT_IS_LOW_X | HT_SPLIT_MIRROR_LEFT)

// ---- labels ------------------------------------------------------------------------------------------------------------------------------------------------------
// the 16-bit minimum on link idx (two links to a word); returns the link it found there
__device__ __forceinline__ unsigned sp_min16(unsigned *words, unsigned idx, unsigned val)
{
	unsigned *wp = words + (idx >> 1); const unsigned sh = (idx & 1u) * 16u;
	unsigned old = *(volatile unsigned *)wp;
	for (;;)      // retried only when another lane lowered a link of this word in between
	{
		const unsigned cur = (old >> sh) & 0xFFFFu;
		if (cur <= val) return cur;
		const unsigned seen = atomicCAS(wp, old, (old & ~(0xFFFFu << sh)) | (val << sh));
		if (seen == old) return cur;
		old = seen;
	}
}
__device__ __forceinline__ unsigned sp_find(const volatile uint16_t *lab, unsigned a)
{
	for (;;) { const unsigned p = lab[a]; if (p == a) return a; a = p; }      // p < a: strictly down
}
__device__ __forceinline__ void sp_union(uint16_t *lab, unsigned a, unsigned b)
{
	const unsigned a0 = a, b0 = b;
	for (;;)      // max(a, b) strictly decreases
	{
		a = sp_find(lab, a); b = sp_find(lab, b);
		if (a == b) break;
		if (a < b) { const unsigned t = a; a = b; b = t; }
		const unsigned old = sp_min16((unsigned *)lab, a, b);
		if (old == a) { a = b; break; }
		a = old;
	}
	sp_min16((unsigned *)lab, a0, a); sp_min16((unsigned *)lab, b0, a);      // shorten both chains to an ancestor: later finds start nearer the root
}
// block-wide maximum / sum of one unsigned per thread (all threads call; red holds SP_THREADS / 64 + 1 words)
__device__ __forceinline__ unsigned sp_block_max(unsigned v, unsigned *red)
{
	for (int o = 32; o; o >>= 1) { const unsigned u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
	__syncthreads();
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	if (threadIdx.x < 64)
	{
		unsigned m = threadIdx.x < SP_THREADS / 64 ? red[threadIdx.x] : 0u;
		for (int o = 32; o; o >>= 1) { const unsigned u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
		if (threadIdx.x == 0) red[SP_THREADS / 64] = m;
	}
	__syncthreads();
	return red[SP_THREADS / 64];
}
__device__ __forceinline__ unsigned sp_block_sum(unsigned v, unsigned *red)
{
	for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
	__syncthreads();
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	if (threadIdx.x < 64)
	{
		unsigned m = threadIdx.x < SP_THREADS / 64 ? red[threadIdx.x] : 0u;
		for (int o = 32; o; o >>= 1) m += __shfl_xor(m, o, 64);
		if (threadIdx.x == 0) red[SP_THREADS / 64] = m;
	}
	__syncthreads();
	return red[SP_THREADS / 64];
}

// stats [2][8]: count, label, sum_x, sum_y, min_x, min_y, max_x, max_y of the larger (0) and the smaller (1) chosen component
__global__ __launch_bounds__(SP_THREADS) void k_split_label(const uint16_t *__restrict__ depth, int w, int h, unsigned lo, unsigned hi, unsigned max_step, int min_pixels, int right_is_low,
                                                            int wide, int32_t *__restrict__ info, int32_t *__restrict__ ncomp, uint16_t *__restrict__ labels)
{
	__shared__ __align__(16) uint16_t q[SP_MAXCELLS];
	__shared__ __align__(16) uint16_t lab[SP_MAXCELLS];
	__shared__ unsigned red[SP_THREADS / 64 + 1];
	__shared__ int stats[2][8];
	const unsigned t = threadIdx.x, W4 = (unsigned)w >> 2, H4 = (unsigned)h >> 2, n = W4 * H4;
	const uint16_t *src = depth + (size_t)blockIdx.x * (unsigned)w * (unsigned)h;
	// the quarter image
	for (unsigned i = t; i < n; i += SP_THREADS)
	{
		const unsigned Y = i / W4, X = i - Y * W4;
		const uint16_t *p = src + (size_t)(4u * Y) * (unsigned)w + 4u * X;
		unsigned m = 0xFFFFu;
		if (wide)      // rows are multiples of 8 bytes, the base is 8-byte aligned
		{
#pragma unroll
			for (int r = 0; r < 4; r++)
			{
				const uint2 v = *(const uint2 *)(p + (size_t)r * (unsigned)w);
				m = min(min(m, min(v.x & 0xFFFFu, v.x >> 16)), min(v.y & 0xFFFFu, v.y >> 16));
			}
		}
		else
		{
#pragma unroll
			for (int r = 0; r < 4; r++)
#pragma unroll
				for (int c = 0; c < 4; c++) m = min(m, (unsigned)p[(size_t)r * (unsigned)w + c]);
		}
		q[i] = (uint16_t)m;
	}
	__syncthreads();
	// 1. rows: a link to the left neighbour where connected
	for (unsigned i = t; i < n; i += SP_THREADS)
	{
		const unsigned v = q[i];
		unsigned l = SP_NONE;
		if (v >= lo && v < hi)
		{
			l = i;
			if (i % W4)
			{
				const unsigned u = q[i - 1];
				if (u >= lo && u < hi && (v > u ? v - u : u - v) <= max_step) l = i - 1;
			}
		}
		lab[i] = (uint16_t)l;
	}
	__syncthreads();
	for (int round = 0; round < 8; round++)      // 2^8 >= 160 cells of a row
	{
		// in place: a link read while its owner rewrites it is the old or the new one, both cells of the run further left, so a round at least halves every depth
		for (unsigned i = t; i < n; i += SP_THREADS)
		{
			const unsigned l = ((volatile uint16_t *)lab)[i];
			if (l != SP_NONE && l != i) ((volatile uint16_t *)lab)[i] = ((volatile uint16_t *)lab)[l];
		}
		__syncthreads();
	}
	// 2. columns: unite with the run above
	for (unsigned i = t + W4; i < n; i += SP_THREADS)      // (t + W4: row 0 has nothing above it)
	{
		const unsigned v = q[i], u = q[i - W4];
		if (v >= lo && v < hi && u >= lo && u < hi && (v > u ? v - u : u - v) <= max_step) sp_union(lab, i, i - W4);
	}
	__syncthreads();
	// 3. flatten
	for (int round = 0; round < 32; round++)      // at most 16 change anything
	{
		int changed = 0;
		for (unsigned i = t; i < n; i += SP_THREADS)
		{
			const unsigned l = ((volatile uint16_t *)lab)[i];
			if (l == SP_NONE) continue;
			const unsigned g = ((volatile uint16_t *)lab)[l];
			if (g != l) { ((volatile uint16_t *)lab)[i] = (uint16_t)g; changed = 1; }
		}
		if (!__syncthreads_or(changed)) break;
	}
	// counts: 16-bit counters, two to a word, in Q's place
	unsigned *cnt = (unsigned *)q;
	for (unsigned i = t; i < (n + 1) / 2; i += SP_THREADS) cnt[i] = 0u;
	if (t < 16) (&stats[0][0])[t] = 0;
	__syncthreads();
	for (unsigned i = t; i < n; i += SP_THREADS) { const unsigned l = lab[i]; if (l != SP_NONE) atomicAdd(&cnt[l >> 1], 1u << ((l & 1u) * 16u)); }
	__syncthreads();
	// selection
	unsigned best = 0, second = 0, eligible = 0;
	for (unsigned i = t; i < n; i += SP_THREADS)
	{
		if (lab[i] != i) continue;
		const unsigned c = (cnt[i >> 1] >> ((i & 1u) * 16u)) & 0xFFFFu;
		if ((long long)c < (long long)min_pixels) continue;
		eligible++;
		const unsigned key = (c << 16) | (0xFFFFu - i);
		if (key > best) { second = best; best = key; } else if (key > second) second = key;
	}
	const unsigned k1 = sp_block_max(best, red);
	const unsigned k2 = sp_block_max(best == k1 ? second : best, red);      // keys are distinct: only k1's owner gives its runner-up
	const unsigned total = sp_block_sum(eligible, red);
	const unsigned la = k1 ? 0xFFFFu - (k1 & 0xFFFFu) : 0x10000u, lb = k2 ? 0xFFFFu - (k2 & 0xFFFFu) : 0x10000u;
	if (t == 0)
	{
		stats[0][0] = (int)(k1 >> 16); stats[0][1] = k1 ? (int)la : (int)SP_NONE; stats[1][0] = (int)(k2 >> 16); stats[1][1] = k2 ? (int)lb : (int)SP_NONE;
		for (int c = 0; c < 2; c++) if (c ? k2 : k1) { stats[c][4] = stats[c][5] = 0x7fffffff; }
	}
	__syncthreads();
	if (k1)
	{
		int sx[2] = { 0, 0 }, sy[2] = { 0, 0 }, x0[2] = { 0x7fffffff, 0x7fffffff }, y0[2] = { 0x7fffffff, 0x7fffffff }, x1[2] = { -1, -1 }, y1[2] = { -1, -1 };
		for (unsigned i = t; i < n; i += SP_THREADS)
		{
			const unsigned l = lab[i];
			if (l != la && l != lb) continue;
			const int Y = (int)(i / W4), X = (int)(i - (unsigned)Y * W4);
#pragma unroll
			for (int c = 0; c < 2; c++) if (l == (c ? lb : la)) { sx[c] += X; sy[c] += Y; x0[c] = min(x0[c], X); y0[c] = min(y0[c], Y); x1[c] = max(x1[c], X); y1[c] = max(y1[c], Y); }
		}
#pragma unroll
		for (int c = 0; c < 2; c++) if (x1[c] >= 0)
		{
			atomicAdd(&stats[c][2], sx[c]); atomicAdd(&stats[c][3], sy[c]);
			atomicMin(&stats[c][4], x0[c]); atomicMin(&stats[c][5], y0[c]); atomicMax(&stats[c][6], x1[c]); atomicMax(&stats[c][7], y1[c]);
		}
	}
	__syncthreads();
	// left / right: slot 0 of info is the right hand, slot 1 the left
	if (t < 16)
	{
		int low = -1, high = -1;      // which of stats[0], stats[1] is on the low-x side and which on the high-x side; -1: none
		if (k1 && k2)
		{
			const long long a = (long long)stats[0][2] * stats[1][0], b = (long long)stats[1][2] * stats[0][0];
			const bool a_lower = a < b || (a == b && stats[0][1] < stats[1][1]);
			low = a_lower ? 0 : 1; high = 1 - low;
		}
		else if (k1) { if (2ll * stats[0][2] < (long long)stats[0][0] * (long long)(W4 - 1u)) low = 0; else high = 0; }
		const int right = right_is_low ? low : high, left = right_is_low ? high : low;
		const int hand = t >> 3, e = t & 7, from = hand ? left : right;
		info[(size_t)blockIdx.x * 16 + t] = from < 0 ? (e == 1 ? (int)SP_NONE : 0) : stats[from][e];
		if (t == 0 && ncomp) ncomp[blockIdx.x] = (int)total;
	}
	if (labels) for (unsigned i = t; i < n; i += SP_THREADS) labels[(size_t)blockIdx.x * n + i] = lab[i];
}

// ---- frames --------------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned sp_hand_label(const int32_t *info, unsigned f, unsigned k) { return info[(size_t)f * 16 + k * 8] ? (unsigned)info[(size_t)f * 16 + k * 8 + 1] : 0x10000u; }

// in [B][h][w], labels [B][H4][W4], info [B][2][8] -> out [B][2][h][w].  per_row vectors a row (w % (2N) == 0), W4 cells a row
template <int N> __global__ __launch_bounds__(SP_WTHREADS) void k_split_write(const uint16_t *__restrict__ in, const uint16_t *__restrict__ labels, const int32_t *__restrict__ info, uint16_t *__restrict__ out,
                                                                              unsigned per_row, unsigned per_frame, unsigned W4, unsigned cells, unsigned B, unsigned far2, int mirror)
{
	const unsigned r = blockIdx.x * SP_WTHREADS + threadIdx.x;
	if (r >= per_frame) return;
	const unsigned y = r / per_row, xv = r - y * per_row, rm = r - xv + (per_row - 1u - xv);
	const unsigned cell = (y >> 2) * W4 + ((xv * 2u * N) >> 2);
	const ht_dwords<N> *src = (const ht_dwords<N> *)in; ht_dwords<N> *dst = (ht_dwords<N> *)out;
	for (unsigned f = blockIdx.y; f < B; f += gridDim.y)
	{
		const unsigned right = sp_hand_label(info, f, 0), left = sp_hand_label(info, f, 1);
		const unsigned l0 = labels[(size_t)f * cells + cell], l1 = N == 4 ? (unsigned)labels[(size_t)f * cells + cell + 1] : l0;      // 8 pixels: two cells
		const ht_dwords<N> a = src[(size_t)f * per_frame + r];
		ht_dwords<N> o, m;
#pragma unroll
		for (int i = 0; i < N; i++) { const unsigned l = i >= 2 ? l1 : l0; o.v[i] = l == right ? a.v[i] : far2; m.v[i] = l == left ? a.v[i] : far2; }
		dst[(size_t)(2u * f) * per_frame + r] = o;
		if (mirror) { ht_dwords<N> x; ht_reverse(m, x); dst[(size_t)(2u * f + 1u) * per_frame + rm] = x; }
		else dst[(size_t)(2u * f + 1u) * per_frame + r] = m;
	}
}
// a pixel per thread: buffers aligned to two bytes only
template <> __global__ __launch_bounds__(SP_WTHREADS) void k_split_write<0>(const uint16_t *__restrict__ in, const uint16_t *__restrict__ labels, const int32_t *__restrict__ info, uint16_t *__restrict__ out,
                                                                            unsigned per_row, unsigned per_frame, unsigned W4, unsigned cells, unsigned B, unsigned far2, int mirror)
{
	const unsigned r = blockIdx.x * SP_WTHREADS + threadIdx.x;
	if (r >= per_frame) return;
	const unsigned y = r / per_row, xv = r - y * per_row, rm = r - xv + (per_row - 1u - xv);
	const unsigned cell = (y >> 2) * W4 + (xv >> 2);
	for (unsigned f = blockIdx.y; f < B; f += gridDim.y)
	{
		const unsigned right = sp_hand_label(info, f, 0), left = sp_hand_label(info, f, 1);
		const unsigned l = labels[(size_t)f * cells + cell];
		const uint16_t a = in[(size_t)f * per_frame + r];
		out[(size_t)(2u * f) * per_frame + r] = l == right ? a : (uint16_t)far2;
		out[(size_t)(2u * f + 1u) * per_frame + (mirror ? rm : r)] = l == left ? a : (uint16_t)far2;
	}
}
// cams [B][12] -> out [B][2][12]
__global__ __launch_bounds__(SP_WTHREADS) void k_split_cams(const unsigned *__restrict__ in, unsigned *__restrict__ out, float wm1, unsigned n, int mirror)
{
	const unsigned i = blockIdx.x * SP_WTHREADS + threadIdx.x;
	if (i >= n) return;
	const unsigned f = i / (2 * HT_CAM), j = i - f * (2 * HT_CAM), k = j % HT_CAM;
	const unsigned v = in[f * HT_CAM + k];
	out[i] = (j >= HT_CAM && mirror) ? ht_mirror_cam_word(v, k, wm1) : v;
}

// ---- launch layer ------------------------------------------------------------------------------------------------------------------------------------------------
void ht_launch_split_label(const uint16_t *depth, int w, int h, int B, unsigned lo, unsigned hi, unsigned max_step, int min_pixels, int flags, int32_t *info, int32_t *ncomp, uint16_t *labels, hipStream_t s)
{
	const int wide = ((uintptr_t)depth & 7) == 0;      // (w % 4 == 0: every 4-pixel group of an 8-byte aligned buffer is 8-byte aligned)
	hipLaunchKernelGGL(k_split_label, dim3(B), dim3(SP_THREADS), 0, s, depth, w, h, lo, hi, max_step, min_pixels, (flags & HT_SPLIT_RIGHT_IS_LOW_X) ? 1 : 0, wide, info, ncomp, labels);
}
void ht_launch_split_write(const uint16_t *in, const uint16_t *labels, const int32_t *info, int w, int h, int B, unsigned far, int flags, uint16_t *out, hipStream_t s)
{
	const int mirror = (flags & HT_SPLIT_MIRROR_LEFT) ? 1 : 0;
	ht_frame_vec_dispatch(ht_frame_vec_pixels((uintptr_t)in | (uintptr_t)out, w), [&](auto px)      // a hand's frame starts a multiple of w * h pixels into `out`
	{
		const ht_frame_grid g(w, h, B, px, SP_WTHREADS);
		hipLaunchKernelGGL(k_split_write<px / 2>, g.grid, dim3(SP_WTHREADS), 0, s, in, labels, info, out, g.per_row, g.per_frame, (unsigned)w / 4u, ((unsigned)w / 4u) * ((unsigned)h / 4u), (unsigned)B,
		                   far | (far << 16), mirror);
	});
}
void ht_launch_split_cams(const float *in, int w, int B, int flags, float *out, hipStream_t s)
{
	const unsigned n = (unsigned)B * 2u * HT_CAM;
	hipLaunchKernelGGL(k_split_cams, dim3((n + SP_WTHREADS - 1) / SP_WTHREADS), dim3(SP_WTHREADS), 0, s, (const unsigned *)in, (unsigned *)out, (float)(w - 1), n, (flags & HT_SPLIT_MIRROR_LEFT) ? 1 : 0);
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------------------------------------
// Every check runs before anything grows or launches.  B is not bounded by max_batch: no tracker slot, no model, no weights.
int ht_split_check(ht_ctx *ctx, const char *fn, int w, int h, int range_lo, int range_hi, int min_pixels, int far, int flags)
{
	const std::string f(fn);
	if (!ht_segment_supported_sized(w, h, 64)) { ctx->err = f + ": frame size must be a multiple of 4, at least 8x8 and at most 640x480 pixels (19200 quarter-size pixels)"; return HT_ERR_ARG; }
	if (range_lo >= range_hi) { ctx->err = f + ": range_lo must be below range_hi"; return HT_ERR_ARG; }
	if (far < range_hi) { ctx->err = f + ": far must not be below range_hi (a masked pixel would be foreground)"; return HT_ERR_ARG; }
	if (min_pixels < 1) { ctx->err = f + ": min_pixels must be at least 1"; return HT_ERR_ARG; }
	if (flags & ~SP_FLAGS) { ctx->err = f + ": unknown flag bits"; return HT_ERR_ARG; }
	return HT_OK;
}
static int split_check_call(ht_ctx *ctx, const void *in, const void *out, const void *info, int w, int h, int B, int range_lo, int range_hi, int min_pixels, int far, int flags, const void *cams, const void *cams_out)
{
	if (!in || !out || !info || B < 0 || (B > 0x7fffffff / 24)) { ctx->err = "ht_split_hands: bad argument"; return HT_ERR_ARG; }
	if ((cams_out != nullptr) != (cams != nullptr)) { ctx->err = "ht_split_hands: cams and cams_out are given together or not at all"; return HT_ERR_ARG; }
	{ const int r = ht_split_check(ctx, "ht_split_hands", w, h, range_lo, range_hi, min_pixels, far, flags); if (r) return r; }
	const size_t bytes = (size_t)B * w * h * sizeof(uint16_t);
	if (ht_ranges_overlap(in, bytes, out, 2 * bytes)) { ctx->err = "ht_split_hands: depth and depth_out must not overlap"; return HT_ERR_ARG; }
	return HT_OK;
}
extern "C" int ht_split_hands_dev(ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, int flags,
                                  uint16_t *d_depth_out, float *d_cams_out, int32_t *d_info, int32_t *d_n_components, uint16_t *d_label_img, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = split_check_call(ctx, d_depth, d_depth_out, d_info, w, h, B, range_lo, range_hi, min_pixels, far, flags, d_cams, d_cams_out); if (r) return r; }
	if (B == 0) return HT_OK;
	if (!d_label_img)      // the frames are cut along the label image: the context keeps one when the caller wants none
	{
		const int r = dev_grow(ctx, &ctx->d_split_labels, &ctx->split_labels_cap, (size_t)B * (w / 4) * (h / 4));
		if (r) return r;
		d_label_img = ctx->d_split_labels;
	}
	hipStream_t s = ht_user_stream(ctx, stream);
	{ ht_prof_scope ps(ctx, "k_split_label", s); ht_launch_split_label(d_depth, w, h, B, range_lo, range_hi, max_step, min_pixels, flags, d_info, d_n_components, d_label_img, s); }
	{ ht_prof_scope ps(ctx, "k_split_write", s); ht_launch_split_write(d_depth, d_label_img, d_info, w, h, B, far, flags, d_depth_out, s); }
	if (d_cams) { ht_prof_scope ps(ctx, "k_split_cams", s); ht_launch_split_cams(d_cams, w, B, flags, d_cams_out, s); }
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
// The host form: inputs and outputs through the context's staging (ht_staged_call), the same kernels.  Its segments are 256-byte aligned: the widest path the width allows.
extern "C" int ht_split_hands(ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, int B, uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, int flags,
                              uint16_t *depth_out, float *cams_out, int32_t *info, int32_t *n_components, uint16_t *labels)
{
	CHECK_READY(ctx);
	{ const int r = split_check_call(ctx, depth, depth_out, info, w, h, B, range_lo, range_hi, min_pixels, far, flags, cams, cams_out); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t bytes = (size_t)B * w * h * sizeof(uint16_t), cb = (size_t)B * HT_CAM * sizeof(float);
	ht_seg seg[7] = { { (void *)depth, bytes, false }, { (void *)cams, cb, false }, { depth_out, 2 * bytes, true }, { cams_out, 2 * cb, true }, { info, (size_t)B * 16 * sizeof(int32_t), true },
	                  { n_components, (size_t)B * sizeof(int32_t), true }, { labels, (size_t)B * (w / 4) * (h / 4) * sizeof(uint16_t), true } };
	return ht_staged_call(ctx, seg, 7, [&](hipStream_t s)
	                      { return ht_split_hands_dev(ctx, (const uint16_t *)seg[0].dev, (const float *)seg[1].dev, w, h, B, range_lo, range_hi, max_step, min_pixels, far, flags, (uint16_t *)seg[2].dev,
	                                                  (float *)seg[3].dev, (int32_t *)seg[4].dev, (int32_t *)seg[5].dev, (uint16_t *)seg[6].dev, s); });
}
