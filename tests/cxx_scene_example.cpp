// A scene of several hands through the reference-named C++ surface: HandTracker::render_scene (an addition of include/ht_handtrack.hpp) against the C call
// ht_raster_scene_depth on the same poses.
//
//   example <model> <in.bin> <out.bin>
//
// in.bin:  int32 H, w, h, nb, with_bg; f32 far, pixel_offset; f32 cam[12]; u8 left[H] padded to 4 bytes; H records { f32 pose[nb][7] } (centre-of-mass poses);
//          u16 bg[w*h] when with_bg
// out.bin: u16 depth[w*h], i8 hand[w*h], i8 body[w*h], i32 visible[H] of render_scene, then the same from the C call on a context of its own
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
		int hdr[5]; float opt[2], cam[12];
		if (fread(hdr, 4, 5, f) != 5 || fread(opt, 4, 2, f) != 2 || fread(cam, 4, 12, f) != 12) throw std::runtime_error("short input");
		const int H = hdr[0], w = hdr[1], h = hdr[2], nb = hdr[3];
		if (H < 1 || H > HT_SCENE_MAX_HANDS) throw std::runtime_error("between 1 and 4 hands");
		unsigned char left[4];
		if (fread(left, 1, 4, f) != 4) throw std::runtime_error("short flags");
		std::vector<float> flat((size_t)H * nb * 7);
		if (fread(flat.data(), 4, flat.size(), f) != flat.size()) throw std::runtime_error("short poses");
		std::vector<unsigned short> bg;
		if (hdr[4]) { bg.resize((size_t)w * h); if (fread(bg.data(), 2, bg.size(), f) != bg.size()) throw std::runtime_error("short background"); }
		fclose(f);
		std::vector<std::pair<std::vector<Pose>, bool>> hands(H);
		for (int k = 0; k < H; k++)
		{
			for (int b = 0; b < nb; b++)
			{
				const float *g = &flat[((size_t)k * nb + b) * 7];
				Pose p; p.position = { g[0], g[1], g[2] }; p.orientation = { g[3], g[4], g[5], g[6] }; hands[k].first.push_back(p);
			}
			hands[k].second = left[k] != 0;
		}
		HandTracker htk(argv[1], "");                                                             // no net needed to draw
		Pose cp; cp.position = { cam[5], cam[6], cam[7] }; cp.orientation = { cam[8], cam[9], cam[10], cam[11] };
		const DCamera dcam({ w, h }, { cam[0], cam[1] }, { cam[2], cam[3] }, cam[4], cp);
		const HandTracker::Scene s = bg.empty() ? htk.render_scene(hands, dcam, opt[0], opt[1]) : htk.render_scene(hands, dcam, opt[0], opt[1], Image<unsigned short>(dcam, bg));
		// the C call
		ht_ctx *ctx = nullptr;
		if (ht_create(argv[1], 1, 0, &ctx) != HT_OK) throw std::runtime_error("ht_create failed");
		const size_t n = (size_t)w * h;
		std::vector<unsigned short> d(n); std::vector<int8_t> hand(n), body(n); std::vector<int32_t> vis(H);
		uint8_t flags[4]; for (int k = 0; k < 4; k++) flags[k] = left[k] ? 1 : HT_SCENE_RIGHT;
		const int rc = ht_raster_scene_depth(ctx, flat.data(), flags, H, cam, w, h, opt[0], opt[1], 1, bg.empty() ? nullptr : bg.data(), d.data(), hand.data(), body.data(), vis.data());
		ht_destroy(ctx);
		if (rc != HT_OK) throw std::runtime_error("ht_raster_scene_depth failed");
		FILE *o = fopen(argv[3], "wb"); if (!o) throw std::runtime_error("cannot open output");
		fwrite(s.depth.raster.data(), 2, n, o); fwrite(s.hand.data(), 1, n, o); fwrite(s.body.data(), 1, n, o); fwrite(s.visible.data(), 4, H, o);
		fwrite(d.data(), 2, n, o); fwrite(hand.data(), 1, n, o); fwrite(body.data(), 1, n, o); fwrite(vis.data(), 4, H, o);
		fclose(o);
		printf("render_scene: %d hands in %dx%d\n", H, s.depth.dim().x, s.depth.dim().y);
		return 0;
	}
	catch (const std::exception &e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
