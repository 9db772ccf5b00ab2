// The device renderer through the reference-named C++ surface: HandTracker::render_depth (an addition of include/ht_handtrack.hpp) renders the
// frames the application's software rasteriser would (synthetic-tracker.cpp:69-76,182) for the ground-truth poses of a recording.
//
//   driver <model> <in.bin> <out.bin>
//
// in.bin:  int32 n, w, h, nb; then n records { u16 depth[w*h]; f32 cam[12]; f32 start[nb][7]; f32 gt[nb][7] } (tests/cxx_headless_driver.cpp's input)
// out.bin: n records { u16 depth[w*h] }: all frames in one batch with frame 0's camera; frame 0 once more through the single-frame overload must agree.
#define HT_MI355X_GLOBAL_NAMES
#include <cstdio>
#include <cstring>
#include "../include/ht_handtrack.hpp"

int main(int argc, char **argv)
{
	if (argc < 4) { printf("usage: %s <model> <in> <out>\n", argv[0]); return 2; }
	try
	{
		FILE *f = fopen(argv[2], "rb"); if (!f) throw std::runtime_error("cannot open input");
		int hdr[4]; if (fread(hdr, 4, 4, f) != 4) throw std::runtime_error("short input");
		const int n = hdr[0], w = hdr[1], h = hdr[2], nb = hdr[3];
		std::vector<std::vector<Pose>> gt(n); float cam[12] = { 0 };
		for (int k = 0; k < n; k++)
		{
			std::vector<unsigned short> d((size_t)w * h); std::vector<float> start((size_t)nb * 7), g((size_t)nb * 7); float c[12];
			if (fread(d.data(), 2, d.size(), f) != d.size() || fread(c, 4, 12, f) != 12 || fread(start.data(), 4, start.size(), f) != start.size() || fread(g.data(), 4, g.size(), f) != g.size()) throw std::runtime_error("short record");
			if (k == 0) memcpy(cam, c, sizeof cam);
			for (int b = 0; b < nb; b++) { Pose p; p.position = { g[7 * b], g[7 * b + 1], g[7 * b + 2] }; p.orientation = { g[7 * b + 3], g[7 * b + 4], g[7 * b + 5], g[7 * b + 6] }; gt[k].push_back(p); }
		}
		fclose(f);
		HandTracker htk(argv[1], "");                                                             // no net needed to draw
		Pose cp; cp.position = { cam[5], cam[6], cam[7] }; cp.orientation = { cam[8], cam[9], cam[10], cam[11] };
		const DCamera dcam({ w, h }, { cam[0], cam[1] }, { cam[2], cam[3] }, cam[4], cp);
		const std::vector<Image<unsigned short>> frames = htk.render_depth(gt, dcam);           // 4 m far point, as the application
		const Image<unsigned short> one = htk.render_depth(gt[0], dcam);
		if ((int)frames.size() != n || one.raster != frames[0].raster) throw std::runtime_error("single-frame overload disagrees with the batch");
		FILE *o = fopen(argv[3], "wb"); if (!o) throw std::runtime_error("cannot open output");
		for (auto &im : frames) fwrite(im.raster.data(), 2, im.raster.size(), o);
		fclose(o);
		printf("render_depth: %d frames of %dx%d\n", n, frames[0].dim().x, frames[0].dim().y);
		return 0;
	}
	catch (const std::exception &e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
