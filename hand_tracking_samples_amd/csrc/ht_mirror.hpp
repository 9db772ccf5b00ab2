// ht_mirror.hpp -- the mirror x -> -x on one word of a camera [12], shared by the kernels that write mirrored cameras (k_mirror_cams, ht_mirror.hip; k_split_cams, ht_split.hip).
#pragma once
#include "ht_device.hpp"

// word k of a camera of frames whose last column is wm1 = (float)(w - 1): principal x at 2, the pose at 5..11 (position 5 6 7, quaternion xyzw 8 9 10 11)
__device__ __forceinline__ unsigned ht_mirror_cam_word(unsigned v, unsigned k, float wm1)
{
	if (k == 2) return __float_as_uint(wm1 - __uint_as_float(v));
	if (k == 5 || k == 9 || k == 10) return v ^ 0x80000000u;
	return v;
}
