// ht_rank.hpp -- ranking a segment of frames by counting, the keys in LDS: what k_contact_order (ht_gjk.hip) and k_rank_desc (ht_solver.hip) share (product code).
#pragma once
#include <hip/hip_runtime.h>

#define HT_RANK_SEG 4096      // frames a segment holds (the count is quadratic): a larger batch is ranked segment by segment, each over its own blocks

// The block stages key(w[i]) of the segment's B frames into lds, padded to whole int4 with key(-1) (a work is never negative, so key must put -1 below every frame's key)
template <class F> __device__ __forceinline__ void rank_stage(int *lds, const int *__restrict__ w, int B, int nthreads, F key)
{
	for (int i = threadIdx.x, B4 = (B + 3) & ~3; i < B4; i += nthreads) lds[i] = key(i < B ? w[i] : -1);
}
// The place of frame i (< B) among the staged keys, largest first, equal keys by index.  RANK_KEYS4(lds)(j): the four keys from j on, read where the kernel's array is in
// sight -- the compiler widens the read as far as it knows that array to be aligned, and through a pointer parameter it would take an int4's alignment for granted
// (k_contact_order's dynamic array is 4-byte aligned: the hardware splits such a read, 293 -> 702 us at 8192 frames)
#define RANK_KEYS4(lds) [&](int j) { return *reinterpret_cast<const int4 *>((lds) + j); }
template <class L> __device__ __forceinline__ int rank_desc(L keys4, int wi, int i, int B)
{
	const int B4 = (B + 3) & ~3; int rank = 0;
	for (int j = 0; j < B4; j += 4)
	{
		const int4 k = keys4(j);
		rank += ((k.x > wi || (k.x == wi && j < i)) ? 1 : 0) + ((k.y > wi || (k.y == wi && j + 1 < i)) ? 1 : 0) + ((k.z > wi || (k.z == wi && j + 2 < i)) ? 1 : 0) + ((k.w > wi || (k.w == wi && j + 3 < i)) ? 1 : 0);
	}
	return rank;
}
