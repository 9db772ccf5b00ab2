// The host side of ht_calibrate_view under the sanitizers: a stand-alone program (its own main) that takes csrc/ht_calib.hip's host code into this translation unit, so
// that -Xarch_host -fsanitize=address,undefined instruments it, and links everything else from the library as it is built.  It drives, on a context whose ht_create
// failed (no device is needed, none is used): every argument check of both forms, the defaults, and the staging plan of the host form -- each segment's byte count is
// walked over a host array of exactly the documented size, so a plan that is one byte too long is a heap overflow the sanitizer reports.
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tests/hip_calib_host_check.hip -L<libdir> -lht_mi355x -fsanitize=address,undefined
#include <cstdio>
#include <vector>
#include "../hand_tracking_samples_amd/csrc/ht_calib.hip"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static unsigned walk(const ht_seg &s)      // reads every byte of a segment's host range
{
	unsigned sum = 0;
	const unsigned char *p = (const unsigned char *)s.host;
	for (size_t i = 0; p && i < s.bytes; i++) sum += p[i];
	return sum;
}

int main()
{
	ht_ctx *ctx = nullptr;
	EXPECT(ht_create("/nonexistent/model.htfx", 4, 0, &ctx) != HT_OK);
	if (!ctx) { printf("ht_create left no context to ask\n"); return 1; }
	ht_calib o;
	EXPECT(ht_calib_default(ctx, &o) == HT_OK && o.mode == HT_CALIB_RIG && o.iterations == 10 && o.min_points == 12);
	EXPECT(ht_calib_default(nullptr, &o) == HT_ERR_ARG && ht_calib_default(ctx, nullptr) == HT_ERR_ARG);
	const int w = 37, h = 29, nb = 17;
	for (int mode = 0; mode < 2; mode++) for (int B = 1; B <= 4; B += 3) for (int it = 0; it <= 64; it += 32)
	{
		o.mode = mode; o.iterations = it; o.fraction = 1 + B;
		const int N = mode == HT_CALIB_PER_SLOT ? B : 1;
		std::vector<float> poses((size_t)B * nb * HT_POSE, 1.0f), cams((size_t)B * HT_CAM, 1.0f), T((size_t)N * 7, 0.0f);
		std::vector<uint16_t> depth((size_t)B * w * h, 1);
		std::vector<double> stats((size_t)(it + 1) * N * HT_CALIB_STATS, 0.0);
		ca_call c;
		EXPECT(ht_calib_check(ctx, "check", 0, poses.data(), depth.data(), cams.data(), w, h, B, &o, T.data(), stats.data(), c) == HT_OK);
		EXPECT(c.N == N && c.bound == (w * h + B) / (1 + B));
		ht_seg seg[5];
		EXPECT(ht_calib_segments(c, nb, poses.data(), depth.data(), cams.data(), w, h, B, T.data(), stats.data(), seg) == 5);
		EXPECT(walk(seg[0]) == (unsigned)walk(ht_seg{ poses.data(), poses.size() * sizeof(float), false, nullptr }));
		EXPECT(seg[0].bytes == poses.size() * sizeof(float) && seg[1].bytes == depth.size() * sizeof(uint16_t) && seg[2].bytes == cams.size() * sizeof(float));
		EXPECT(seg[3].bytes == T.size() * sizeof(float) && seg[4].bytes == stats.size() * sizeof(double) && seg[3].out && seg[4].out && !seg[0].out && !seg[1].out && !seg[2].out);
		EXPECT(walk(seg[1]) + walk(seg[2]) + walk(seg[3]) + walk(seg[4]) > 0);
		// both forms get as far as the context's own state and no further; nothing is written
		EXPECT(ht_calibrate_view(ctx, 0, poses.data(), depth.data(), cams.data(), w, h, B, &o, T.data(), stats.data()) == HT_ERR_STATE);
		EXPECT(ht_calibrate_view_dev(ctx, 0, poses.data(), depth.data(), cams.data(), w, h, B, &o, T.data(), stats.data(), nullptr) == HT_ERR_STATE);
		EXPECT(ht_calibrate_view(ctx, 1, nullptr, depth.data(), cams.data(), w, h, B, &o, T.data(), stats.data()) == HT_ERR_STATE);
		for (float v : T) EXPECT(v == 0.0f);
		for (double v : stats) EXPECT(v == 0.0);
		// refusals by argument
		EXPECT(ht_calibrate_view(ctx, 2, nullptr, depth.data(), cams.data(), w, h, B, &o, T.data(), stats.data()) == HT_ERR_ARG);
		EXPECT(ht_calibrate_view(ctx, 0, nullptr, depth.data(), cams.data(), w, h, 5, &o, T.data(), stats.data()) == HT_ERR_ARG);
		EXPECT(ht_calibrate_view(ctx, 0, nullptr, depth.data(), cams.data(), 0, h, B, &o, T.data(), stats.data()) == HT_ERR_ARG);
		EXPECT(ht_calibrate_view(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, nullptr, stats.data()) == HT_ERR_ARG);
		EXPECT(ht_calibrate_view(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, T.data(), nullptr) == HT_ERR_ARG);
		EXPECT(ht_calibrate_view(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, cams.data() + 5, stats.data()) == HT_ERR_ARG);      // T_out inside cams
		ht_calib bad = o; bad.fraction = 0;
		EXPECT(ht_calibrate_view(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, T.data(), stats.data()) == HT_ERR_ARG);
		bad = o; bad.iterations = 65;
		EXPECT(ht_calibrate_view_dev(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, T.data(), stats.data(), nullptr) == HT_ERR_ARG);
		bad = o; bad.max_dist = 0.0f;
		EXPECT(ht_calibrate_view_dev(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, T.data(), stats.data(), nullptr) == HT_ERR_ARG);
		EXPECT(ht_calibrate_view_dev(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, (float *)((char *)T.data() + 2), stats.data(), nullptr) == HT_ERR_ARG);
	}
	ht_destroy(ctx);
	if (!fails) printf("calib host checks: ok\n");
	return fails ? 1 : 0;
}
