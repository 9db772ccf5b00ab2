// ht_prepare.hpp -- what the kernels that turn depth words into points make of one, each stated once: k_prepare, k_prepare_frame, k_cnn_input (ht_cnn.hip) and
// k_fuse_views (ht_views.hip).  Device code; include after ht_device.hpp.
#pragma once
#include "ht_device.hpp"

__device__ __forceinline__ float depth_metres(unsigned px, float dscale) { return (float)(int)px * dscale; }
__device__ __forceinline__ float cnn_input_value(float d, float drangey) { return clamp_std(1.0f - (d - 0.1f) / (drangey - 0.1f), 0.0f, 1.0f); }      // handtrack.h:700
__device__ __forceinline__ bool depth_in_range(float d, float lo, float hi) { return d >= lo && d < hi; }                                              // FallsWithinRange misc_image.h:24
__device__ __forceinline__ bool depth_in_range(float d, float drangey) { return depth_in_range(d, 0.1f, drangey); }                                       // the tracker's range {0.1, drangey} (handtrack.h:703)
__device__ __forceinline__ float4 deproject_point(float x, float y, float d, float fx, float fy, float cx, float cy) { return make_float4(((x - cx) / fx) * d, ((y - cy) / fy) * d, 1.0f * d, 0.0f); }      // deprojectz misc_image.h:48
// exclusive prefix of cnt over the block's 256 threads (every thread calls it): the thread's base; total: the block's sum
__device__ __forceinline__ int block_prefix256(int cnt, int lane, int wave, int &total)
{
	int incl = cnt;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) { int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
	__shared__ int wsum[4];
	if (lane == 63) wsum[wave] = incl;
	__syncthreads();
	int base = incl - cnt;
	for (int i = 0; i < wave; i++) base += wsum[i];
	total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
	return base;
}
