// The host side of ht_estimate_scale under the sanitizers: a stand-alone program (its own main) that takes csrc/ht_size.hip's host code into this translation unit, so
// that -Xarch_host -fsanitize=address,undefined instruments it, and links everything else from the library as it is built.  It drives, on a context whose ht_create
// failed (no device is needed, none is used): every argument check of both forms, the defaults, and the staging plan of the host form -- each segment's byte count is
// walked over a host array of exactly the documented size, so a plan that is one byte too long is a heap overflow the sanitizer reports.
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tests/hip_size_host_check.hip -L<libdir> -lht_mi355x -fsanitize=address,undefined
#include <cstdio>
#include <vector>
#include "../hand_tracking_samples_amd/csrc/ht_size.hip"

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
	ht_size o;
	EXPECT(ht_size_default(ctx, &o) == HT_OK && o.mode == HT_SIZE_SHARED && o.free_pose == 1 && o.iterations == 10 && o.min_points == 12 && o.scale0 == 1.0f && o.scale_lo == 0.5f && o.scale_hi == 2.0f);
	EXPECT(ht_size_default(nullptr, &o) == HT_ERR_ARG && ht_size_default(ctx, nullptr) == HT_ERR_ARG);
	const int w = 37, h = 29, nb = 17;
	for (int mode = 0; mode < 2; mode++) for (int free_pose = 0; free_pose < 2; free_pose++) for (int B = 1; B <= 4; B += 3) for (int it = 0; it <= 64; it += 32)
	{
		o.mode = mode; o.free_pose = free_pose; o.iterations = it; o.fraction = 1 + B;
		const int N = mode == HT_SIZE_PER_SLOT ? B : 1;
		std::vector<float> poses((size_t)B * nb * HT_POSE, 1.0f), cams((size_t)B * HT_CAM, 1.0f), T((size_t)B * 7, 0.0f), sc((size_t)N, 0.0f);
		std::vector<uint16_t> depth((size_t)B * w * h, 1);
		std::vector<double> stats((size_t)(it + 1) * HT_SIZE_ROW(N, B), 0.0);
		sz_call c;
		EXPECT(ht_size_check(ctx, "check", 0, poses.data(), depth.data(), cams.data(), w, h, B, &o, sc.data(), T.data(), stats.data(), c) == HT_OK);
		EXPECT(c.c.N == N && c.c.bound == (w * h + B) / (1 + B) && c.o.free_pose == free_pose);
		ht_seg seg[6];
		EXPECT(ht_size_segments(c, nb, poses.data(), depth.data(), cams.data(), w, h, B, sc.data(), T.data(), stats.data(), seg) == 6);
		EXPECT(walk(seg[0]) == (unsigned)walk(ht_seg{ poses.data(), poses.size() * sizeof(float), false, nullptr }));
		EXPECT(seg[0].bytes == poses.size() * sizeof(float) && seg[1].bytes == depth.size() * sizeof(uint16_t) && seg[2].bytes == cams.size() * sizeof(float));
		EXPECT(seg[3].bytes == sc.size() * sizeof(float) && seg[4].bytes == T.size() * sizeof(float) && seg[5].bytes == stats.size() * sizeof(double));
		EXPECT(seg[3].out && seg[4].out && seg[5].out && !seg[0].out && !seg[1].out && !seg[2].out);
		EXPECT(walk(seg[1]) + walk(seg[2]) + walk(seg[3]) + walk(seg[4]) + walk(seg[5]) > 0);
		// both forms get as far as the context's own state and no further; nothing is written
		EXPECT(ht_estimate_scale(ctx, 0, poses.data(), depth.data(), cams.data(), w, h, B, &o, sc.data(), T.data(), stats.data()) == HT_ERR_STATE);
		EXPECT(ht_estimate_scale_dev(ctx, 0, poses.data(), depth.data(), cams.data(), w, h, B, &o, sc.data(), T.data(), stats.data(), nullptr) == HT_ERR_STATE);
		EXPECT(ht_estimate_scale(ctx, 1, nullptr, depth.data(), cams.data(), w, h, B, &o, sc.data(), T.data(), stats.data()) == HT_ERR_STATE);
		for (float v : T) EXPECT(v == 0.0f);
		for (float v : sc) EXPECT(v == 0.0f);
		for (double v : stats) EXPECT(v == 0.0);
		// refusals by argument
		EXPECT(ht_estimate_scale(ctx, 2, nullptr, depth.data(), cams.data(), w, h, B, &o, sc.data(), T.data(), stats.data()) == HT_ERR_ARG);
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), w, h, 5, &o, sc.data(), T.data(), stats.data()) == HT_ERR_ARG);
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), 0, h, B, &o, sc.data(), T.data(), stats.data()) == HT_ERR_ARG);
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, nullptr, T.data(), stats.data()) == HT_ERR_ARG);
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, sc.data(), nullptr, stats.data()) == HT_ERR_ARG);
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, sc.data(), T.data(), nullptr) == HT_ERR_ARG);
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, cams.data() + 5, T.data(), stats.data()) == HT_ERR_ARG);      // scale_out inside cams
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, T.data(), T.data(), stats.data()) == HT_ERR_ARG);            // two outputs in one place
		ht_size bad = o; bad.fraction = 0;
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, sc.data(), T.data(), stats.data()) == HT_ERR_ARG);
		bad = o; bad.iterations = 65;
		EXPECT(ht_estimate_scale_dev(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, sc.data(), T.data(), stats.data(), nullptr) == HT_ERR_ARG);
		bad = o; bad.mode = 2;
		EXPECT(ht_estimate_scale_dev(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, sc.data(), T.data(), stats.data(), nullptr) == HT_ERR_ARG);
		bad = o; bad.free_pose = 2;
		EXPECT(ht_estimate_scale_dev(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, sc.data(), T.data(), stats.data(), nullptr) == HT_ERR_ARG);
		bad = o; bad.scale0 = 2.5f;
		EXPECT(ht_estimate_scale_dev(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, sc.data(), T.data(), stats.data(), nullptr) == HT_ERR_ARG);
		bad = o; bad.scale_lo = 0.0f;
		EXPECT(ht_estimate_scale(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &bad, sc.data(), T.data(), stats.data()) == HT_ERR_ARG);
		EXPECT(ht_estimate_scale_dev(ctx, 0, nullptr, depth.data(), cams.data(), w, h, B, &o, sc.data(), (float *)((char *)T.data() + 2), stats.data(), nullptr) == HT_ERR_ARG);
	}
	ht_destroy(ctx);
	if (!fails) printf("size host checks: ok\n");
	return fails ? 1 : 0;
}
