// HandTracker::EstimateHandSize from C++ held against the C call: the frames of one view and the tracked model's poses per frame in; the hand's size out.
//   cxx_size_example model.htfx w h frames.u16 cams.f32 poses.f32 [iterations fraction free_pose]
//     frames: [B][h][w] raw uint16, cams: [B][12] raw fp32 (focal principal depth_scale, then the view's pose: position quaternion),
//     poses: [B][nb][7] raw fp32, centre-of-mass poses in tracking space.
// Runs the C++ form on a HandTracker (one slot) and ht_estimate_scale on a context of its own with the same options, compares the scale, every T and every double of
// stats bit for bit, and prints the scale, frame 0's T and the first and last row's cost as hexadecimal floats (exact); tests/test_cxx_size.py compares them with the
// Python binding's.
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
	if (argc < 7) { printf("usage: %s model.htfx w h frames.u16 cams.f32 poses.f32 [iterations fraction free_pose]\n", argv[0]); return 2; }
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
			Pose view; view.position = { c[5], c[6], c[7] }; view.orientation = { c[8], c[9], c[10], c[11] };
			frames.emplace_back(DCamera({ w, h }, { c[0], c[1] }, { c[2], c[3] }, c[4], view), std::move(d));
			for (size_t k = 0; k < nb; k++) { const float *p = &p7[(b * nb + k) * HT_POSE]; poses[b][k].position = { p[0], p[1], p[2] }; poses[b][k].orientation = { p[3], p[4], p[5], p[6] }; }
		}
		HandTracker::SizeOptions options(htk);
		if (argc >= 10) { options.iterations = atoi(argv[7]); options.fraction = atoi(argv[8]); options.free_pose = atoi(argv[9]); }
		const HandTracker::HandSize r = htk.EstimateHandSize(frames, poses, &options);
		// the C call on a context of its own
		ht_ctx *ctx = nullptr;
		if (ht_create(argv[1], 1, 0, &ctx) != HT_OK) { printf("error: %s\n", ctx ? ht_last_error(ctx) : "ht_create failed"); if (ctx) ht_destroy(ctx); return 1; }
		float scale = 0.0f; std::vector<float> T(B * 7); std::vector<double> stats(r.stats.size());
		const int rc = ht_estimate_scale(ctx, 0, p7.data(), (const uint16_t *)raw.data(), cams.data(), w, h, (int)B, &options, &scale, T.data(), stats.data());
		if (rc != HT_OK) { printf("error: %s\n", ht_last_error(ctx)); ht_destroy(ctx); return 1; }
		ht_destroy(ctx);
		std::vector<float> Tc;
		for (const Pose &p : r.T) { const float t[7] = { p.position.x, p.position.y, p.position.z, p.orientation.x, p.orientation.y, p.orientation.z, p.orientation.w }; Tc.insert(Tc.end(), t, t + 7); }
		const bool equal = !memcmp(&scale, &r.scale, sizeof(float)) && Tc.size() == T.size() && !memcmp(T.data(), Tc.data(), T.size() * sizeof(float)) && !memcmp(stats.data(), r.stats.data(), stats.size() * sizeof(double));
		const size_t row = (size_t)HT_SIZE_ROW(1, B);
		printf("frames=%zu rows=%zu degenerate=%d equal=%d\n", B, r.stats.size() / row, r.degenerate ? 1 : 0, equal ? 1 : 0);
		printf("scale %a\n", r.scale);
		printf("T %a %a %a %a %a %a %a\n", Tc[0], Tc[1], Tc[2], Tc[3], Tc[4], Tc[5], Tc[6]);
		printf("cost %a %a\n", r.stats[2], r.stats[r.stats.size() - row + 2]);
		return equal ? 0 : 1;
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
}
