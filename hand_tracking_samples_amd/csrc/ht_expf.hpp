// ht_expf.hpp -- glibc's expf, restated operation for operation, for the label kernel's 2-D heat-maps (ht_labels.hip).
//
// The reference renders its landmark heat-maps with the C library's expf (misc_image.h:246-272 via GatherHandExpectedCNN, handtrack.h:160-173).
// glibc's expf (sysdeps/ieee754/flt-32/e_expf.c since glibc 2.28, from Arm's optimized-routines) is not correctly rounded: it evaluates
// 2^(k/32) * p(r) in double and rounds once.  (float)exp((double)x), the correctly rounded value, differs from it on 88 557 of the floats in
// [-28, 0] and, after the label's truncation (uchar)(v * 255), on one of them (x = -0x1.265af2p-5: 246 against 245).  So the device repeats
// glibc's evaluation: the same table, constants and double operations in the same order.  tests/test_labels_expf.py compiles this header on the
// host and checks it against the C library's expf on every float in [-28, 0].
//
// Domain: |x| < 88 (glibc's main path; the arguments of the heat-maps lie in (-27.3, 0]).  Freestanding: compiles as plain C++ as well.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HT_EXPF_HD __host__ __device__ __forceinline__
#else
#define HT_EXPF_HD static inline
#endif

// tab[i] = bits(2^(i/32)) - (i << 47): 2^(k/32) for an integer k is the double with bits tab[k % 32] + (k << 47)
#define HT_EXPF_TABLE                                                                                           \
	{ 0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,           \
	  0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,           \
	  0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,           \
	  0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,           \
	  0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,           \
	  0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,           \
	  0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,           \
	  0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull }

HT_EXPF_HD double ht_expf_asdouble(uint64_t u) { double d; memcpy(&d, &u, sizeof d); return d; }
HT_EXPF_HD uint64_t ht_expf_asuint64(double d) { uint64_t u; memcpy(&u, &d, sizeof u); return u; }

// tab: the 32 entries of HT_EXPF_TABLE (the device keeps them in LDS, the host test in a static array)
HT_EXPF_HD float ht_expf_glibc(float x, const uint64_t *tab)
{
	const double InvLn2N = 0x1.71547652b82fep+0 * 32, Shift = 0x1.8p+52;
	const double C0 = 0x1.c6af84b912394p-5 / 32 / 32 / 32, C1 = 0x1.ebfce50fac4f3p-3 / 32 / 32, C2 = 0x1.62e42ff0c52d6p-1 / 32;
	const double xd = (double)x;
	double z = InvLn2N * xd;                      // x * 32 / ln 2 = k + r, r in [-1/2, 1/2]
	double kd = z + Shift;                         // round to nearest through the shift
	const uint64_t ki = ht_expf_asuint64(kd);
	kd -= Shift;
	const double r = z - kd;
	uint64_t t = tab[ki % 32];
	t += ki << (52 - 5);
	const double s = ht_expf_asdouble(t);          // 2^(k/32)
	z = C0 * r + C1;
	const double r2 = r * r;
	double y = C2 * r + 1;
	y = z * r2 + y;
	y = y * s;
	return (float)y;
}
