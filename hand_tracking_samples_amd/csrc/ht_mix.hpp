// ht_mix.hpp -- the 64-bit mixing function behind every counter-based random number of the library: ht_sample_poses' uniform numbers (ht_joints.hip) and
// ht_sensor_simulate's per-pixel fields (ht_sensor.hip).  A bijection of 64-bit words (two xor-shift / multiply rounds and a last xor-shift), the same on host and device.
#pragma once
#include "ht_math.hpp"

HT_HD unsigned long long ht_mix64(unsigned long long x)
{
	x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
	return x;
}
