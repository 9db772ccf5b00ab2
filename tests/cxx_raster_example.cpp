// The mesh rasteriser through the reference-named C++ surface: HandTracker::render_mesh_raster (an addition of include/ht_handtrack.hpp) against the C call
// ht_raster_mesh_depth on the same poses.
//
//   example <model> <in.bin> <out.bin>
//
// in.bin:  int32 n, w, h, nb; f32 far, pixel_offset; f32 cam[12]; then n records { f32 pose[nb][7] } (centre-of-mass poses)
// out.bin: n records { u16 depth[w*h] } of the batch form, then the same n records from the C call on a context of its own; frame 0 through the
//          single-frame overload must agree with the batch.
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
		int hdr[4]; float opt[2], cam[12];
		if (fread(hdr, 4, 4, f) != 4 || fread(opt, 4, 2, f) != 2 || fread(cam, 4, 12, f) != 12) throw std::runtime_error("short input");
		const int n = hdr[0], w = hdr[1], h = hdr[2], nb = hdr[3];
		std::vector<float> flat((size_t)n * nb * 7);
		if (fread(flat.data(), 4, flat.size(), f) != flat.size()) throw std::runtime_error("short poses");
		fclose(f);
		std::vector<std::vector<Pose>> poses(n);
		for (int k = 0; k < n; k++) for (int b = 0; b < nb; b++)
		{
			const float *g = &flat[((size_t)k * nb + b) * 7];
			Pose p; p.position = { g[0], g[1], g[2] }; p.orientation = { g[3], g[4], g[5], g[6] }; poses[k].push_back(p);
		}
		HandTracker htk(argv[1], "");                                                             // no net needed to draw
		Pose cp; cp.position = { cam[5], cam[6], cam[7] }; cp.orientation = { cam[8], cam[9], cam[10], cam[11] };
		const DCamera dcam({ w, h }, { cam[0], cam[1] }, { cam[2], cam[3] }, cam[4], cp);
		const std::vector<Image<unsigned short>> frames = htk.render_mesh_raster(poses, dcam, opt[0], opt[1]);
		const Image<unsigned short> one = htk.render_mesh_raster(poses[0], dcam, opt[0], opt[1]);
		if ((int)frames.size() != n || one.raster != frames[0].raster) throw std::runtime_error("single-frame overload disagrees with the batch");
		// the C call
		ht_ctx *ctx = nullptr;
		if (ht_create(argv[1], 1, 0, &ctx) != HT_OK) throw std::runtime_error("ht_create failed");
		std::vector<float> cams; for (int k = 0; k < n; k++) cams.insert(cams.end(), cam, cam + 12);
		std::vector<unsigned short> d((size_t)n * w * h);
		const int rc = ht_raster_mesh_depth(ctx, flat.data(), cams.data(), w, h, opt[0], opt[1], n, d.data(), nullptr);
		ht_destroy(ctx);
		if (rc != HT_OK) throw std::runtime_error("ht_raster_mesh_depth failed");
		FILE *o = fopen(argv[3], "wb"); if (!o) throw std::runtime_error("cannot open output");
		for (auto &im : frames) fwrite(im.raster.data(), 2, im.raster.size(), o);
		fwrite(d.data(), 2, d.size(), o);
		fclose(o);
		printf("render_mesh_raster: %d frames of %dx%d\n", n, frames[0].dim().x, frames[0].dim().y);
		return 0;
	}
	catch (const std::exception &e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
