// ht_frame_vec.hpp -- what the kernels that move u16 frames one pixel vector per thread share (k_mirror_frames, k_split_write, k_depth_compare, k_sensor_simulate):
// the vector types, the pixel reversal, the rule that picks the vector's width, the launch shape and the step from that width to a template argument.  Host and device.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "ht_math.hpp"

// One load or store: N dwords = 2N pixels for the kernels that keep pixels packed, N pixels for the one that works on each
template <int N> struct alignas(4 * N) ht_dwords { unsigned v[N]; };
template <int N> struct alignas(2 * N) ht_pixels { uint16_t v[N]; };

// o = the pixels of a in reverse order: the dwords in reverse order, each rotated by 16 bits.  (Filling the caller's vector, not returning one: k_split_write<2>
// keeps its single store with a selected address only this way.)
template <int N> HT_HD void ht_reverse(const ht_dwords<N> &a, ht_dwords<N> &o)
{
#pragma unroll
	for (int i = 0; i < N; i++) { const unsigned d = a.v[N - 1 - i]; o.v[i] = (d >> 16) | (d << 16); }
}

// The width rule, the only one.  Pixels per vector for frames w pixels wide: 8 (16 bytes) for w % 8 == 0 and 16-byte alignment, 4 for w % 4 == 0 and 8 bytes, 2, and 1 for an odd
// width or buffers aligned to two bytes only.  `addrs`: the OR of the addresses of every u16 buffer the vectors are loaded from or stored to (frame f starts a multiple
// of w * h pixels in, so the first frame's alignment and the width decide every vector's); a u8 buffer written as many elements goes in shifted left by one.
static inline int ht_frame_vec_pixels(uintptr_t addrs, int w)
{
	for (int px = 8; px > 1; px >>= 1) if (w % px == 0 && (addrs & (uintptr_t)(2 * px - 1)) == 0) return px;
	return 1;
}
// The launch shape (vectors of a frame) x (frames, strided): thread r of blockIdx.x owns vector r of every frame blockIdx.y, blockIdx.y + gridDim.y, ..., so its place
// in the frame is worked out once; about eight blocks a CU
struct ht_frame_grid
{
	unsigned per_row, per_frame; dim3 grid;
	ht_frame_grid(int w, int h, int B, int px, unsigned threads) : per_row((unsigned)w / (unsigned)px), per_frame(per_row * (unsigned)h)
	{
		const unsigned gx = (per_frame + threads - 1) / threads, gy = (2048 + gx - 1) / gx, most = B < 65535 ? (unsigned)B : 65535u;
		grid = dim3(gx, gy < most ? gy : most);
	}
};
// f(std::integral_constant<int, px>) for the rule's 8, 4, 2 or 1
template <class F> static inline void ht_frame_vec_dispatch(int px, F f)
{
	switch (px)
	{
	case 8: f(std::integral_constant<int, 8>()); break;
	case 4: f(std::integral_constant<int, 4>()); break;
	case 2: f(std::integral_constant<int, 2>()); break;
	default: f(std::integral_constant<int, 1>()); break;
	}
}
