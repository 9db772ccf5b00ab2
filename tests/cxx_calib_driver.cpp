// HandTracker::CalibrateView from C++ held against the C call: the frames of one view, the tracked model's poses per frame and a guess in; the view's extrinsics out.
//   cxx_calib_driver model.htfx w h frames.u16 cams.f32 poses.f32 [iterations fraction]
//     frames: [B][h][w] raw uint16, cams: [B][12] raw fp32 (focal principal depth_scale, then the guess: position quaternion; frame 0's guess is the call's),
//     poses: [B][nb][7] raw fp32, centre-of-mass poses in tracking space.
// Runs the C++ form on a HandTracker (one slot) and ht_calibrate_view on a context of its own with the same options, compares T and every double of stats bit for bit,
// and prints T and the first and last record's cost as hexadecimal floats (exact); tests/test_gpu_calib.py compares them with the Python binding's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include "../include/ht_handtrack.hpp"
using namespace ht_mi355x;
static std::vector<char> read_bytes(const char *path)
{
	std::ifstream is(path, std::ios_base::binary);
	if (!is.is_open()) throw std::runtime_error(std::string("cannot open ") + path);
	return std::vector<char>((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
}
static std::vector<float> read_floats(const char *path)
{
	const std::vector<char> b = read_bytes(path);
	std::vector<float> f(b.size() / sizeof(float));
	memcpy(f.data(), b.data(), f.size() * sizeof(float));
	return f;
}
int main(int argc, char **argv)
{
	if (argc < 7) { printf("usage: %s model.htfx w h frames.u16 cams.f32 poses.f32 [iterations fraction]\n", argv[0]); return 2; }
	try
	{
		const int w = atoi(argv[2]), h = atoi(argv[3]);
		HandTracker htk(argv[1], "");
		const std::vector<char> raw = read_bytes(argv[4]);
		const std::vector<float> cams = read_floats(argv[5]), p7 = read_floats(argv[6]);
		const size_t B = cams.size() / HT_CAM, px = (size_t)w * h;
		if (w < 1 || h < 1 || B < 1 || raw.size() != B * px * sizeof(unsigned short) || p7.size() % (B * HT_POSE)) { printf("the files do not match: %zu cameras, %zu frame bytes for %dx%d, %zu pose floats\n", B, raw.size(), w, h, p7.size()); return 1; }
		const size_t nb = p7.size() / (B * HT_POSE);
		std::vector<Image<unsigned short>> frames; std::vector<std::vector<Pose>> poses(B, std::vector<Pose>(nb));
		for (size_t b = 0; b < B; b++)
		{
			const float *c = &cams[b * HT_CAM];
			std::vector<unsigned short> d(px);
			memcpy(d.data(), raw.data() + b * px * sizeof(unsigned short), px * sizeof(unsigned short));
			frames.emplace_back(DCamera({ w, h }, { c[0], c[1] }, { c[2], c[3] }, c[4], Pose()), std::move(d));
			for (size_t k = 0; k < nb; k++) { const float *p = &p7[(b * nb + k) * HT_POSE]; poses[b][k].position = { p[0], p[1], p[2] }; poses[b][k].orientation = { p[3], p[4], p[5], p[6] }; }
		}
		Pose guess; guess.position = { cams[5], cams[6], cams[7] }; guess.orientation = { cams[8], cams[9], cams[10], cams[11] };
		HandTracker::CalibOptions options(htk);
		if (argc >= 9) { options.iterations = atoi(argv[7]); options.fraction = atoi(argv[8]); }
		const HandTracker::ViewCalibration r = htk.CalibrateView(frames, poses, guess, &options);
		// the C call on a context of its own: every slot's guess is frame 0's, as the C++ form passes it
		ht_ctx *ctx = nullptr;
		if (ht_create(argv[1], 1, 0, &ctx) != HT_OK) { printf("error: %s\n", ctx ? ht_last_error(ctx) : "ht_create failed"); if (ctx) ht_destroy(ctx); return 1; }
		std::vector<float> c2 = cams;
		for (size_t b = 0; b < B; b++) memcpy(&c2[b * HT_CAM + 5], &cams[5], 7 * sizeof(float));
		float T[7]; std::vector<double> stats(r.stats.size());
		const int rc = ht_calibrate_view(ctx, 0, p7.data(), (const uint16_t *)raw.data(), c2.data(), w, h, (int)B, &options, T, stats.data());
		if (rc != HT_OK) { printf("error: %s\n", ht_last_error(ctx)); ht_destroy(ctx); return 1; }
		ht_destroy(ctx);
		const float Tc[7] = { r.T.position.x, r.T.position.y, r.T.position.z, r.T.orientation.x, r.T.orientation.y, r.T.orientation.z, r.T.orientation.w };
		const bool equal = !memcmp(T, Tc, sizeof(T)) && !memcmp(stats.data(), r.stats.data(), stats.size() * sizeof(double));
		printf("frames=%zu records=%zu degenerate=%d equal=%d\n", B, r.stats.size() / HT_CALIB_STATS, r.degenerate ? 1 : 0, equal ? 1 : 0);
		printf("T %a %a %a %a %a %a %a\n", Tc[0], Tc[1], Tc[2], Tc[3], Tc[4], Tc[5], Tc[6]);
		printf("cost %a %a\n", r.stats[2], r.stats[r.stats.size() - HT_CALIB_STATS + 2]);
		return equal ? 0 : 1;
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
}
