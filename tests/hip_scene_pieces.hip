// The scene pieces of csrc/ht_raster.hpp, which the host's definition and the kernel both call, printed for tests/test_raster_scene_ref.py: the limit on
// instances times triangles, the mirrored principal point's bits, the flags, the column flip and the composite rule.  Host code only.
#include <cstdio>
#include <cstring>
#include "ht_mi355x.h"
#include "ht_raster.hpp"

int main()
{
	const int fits[][2] = { { 1, 65535 }, { 1, 65536 }, { 2, 32767 }, { 2, 32768 }, { 3, 21845 }, { 3, 21846 }, { 4, 16383 }, { 4, 16384 }, { 4, 8896 }, { 0, 10 }, { 5, 10 }, { -1, 10 }, { 4, 0 } };
	for (auto &f : fits) printf("fits %d %d %d\n", f[0], f[1], rz_scene_fits(f[0], f[1]) ? 1 : 0);
	const struct { float cx; int w; float off; } px[] = { { 12.0f, 24, 0.0f }, { 15.25f, 24, 0.5f }, { 18.5f, 37, 0.5f }, { 160.3f, 320, 0.0f }, { 160.3f, 320, 0.5f }, { 2047.7f, 4096, 1.0f }, { -3.1f, 7, 0.25f } };
	for (auto &p : px) { const float v = rz_mirror_px(p.cx, p.w, p.off); unsigned u; memcpy(&u, &v, 4); printf("px %08x\n", u); }
	const int flags[] = { 0, 1, 7, 254, 255 };
	for (int f : flags) printf("flag %d %d %d\n", f, rz_scene_absent((unsigned char)f) ? 1 : 0, rz_scene_left((unsigned char)f) ? 1 : 0);
	printf("col %d\ncol %d\ncol %d\ncol %d\n", rz_scene_column(5, 37, false), rz_scene_column(5, 37, true), rz_scene_column(36, 37, true), rz_scene_column(0, 37, true));
	const int wins[][3] = { { 10, 0, 5 }, { 10, 1, 0 }, { 10, 1, 10 }, { 10, 1, 9 }, { 10, 1, 11 }, { 0, 1, 0 }, { 65535, 1, 65535 }, { 65535, 1, 65534 } };
	for (auto &k : wins) printf("wins %d\n", rz_scene_wins(k[0], k[1] != 0, (unsigned short)k[2]) ? 1 : 0);
	float p[7] = { 1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f, 7.0f }, o[7];
	rz_mirror_pose(p, o);
	return (o[0] == -1.0f && o[1] == 2.0f && o[2] == 3.0f && o[3] == 4.0f && o[4] == -5.0f && o[5] == -6.0f && o[6] == 7.0f) ? 0 : 1;
}
