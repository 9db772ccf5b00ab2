// HandTracker::FuseViews and HandTracker::update_views from C++: the frames of one hand seen by several posed cameras in, the fused cloud and the tracked pose out.
//   cxx_views_example model.htfx w h frames.u16 cams.f32 [planes.f32|-] [weights.cnnb start.f32]
//     frames: [V][h][w] raw uint16, cams: [V][12] raw fp32 (focal principal depth_scale position quaternion), planes: [V][4] raw fp32 or "-" for none,
//     start: centre-of-mass poses [nb][7] (what SetPose takes).  With weights and a start pose the hand is tracked through update_views (three fused passes).
// Prints the counts and, as hexadecimal floats (exact), the fused points' coordinate sums per source and the pose; tests/test_gpu_views.py compares them with the C calls'.
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
	if (argc < 6) { printf("usage: %s model.htfx w h frames.u16 cams.f32 [planes.f32|-] [weights.cnnb start.f32]\n", argv[0]); return 2; }
	try
	{
		const int w = atoi(argv[2]), h = atoi(argv[3]);
		const bool track = argc >= 9;
		HandTracker htk(argv[1], track ? argv[7] : "");
		const std::vector<char> raw = read_bytes(argv[4]);
		const std::vector<float> cams = read_floats(argv[5]);
		const size_t V = cams.size() / HT_CAM, px = (size_t)w * h;
		if (w < 1 || h < 1 || V < 1 || raw.size() != V * px * sizeof(unsigned short)) { printf("the files do not match: %zu cameras, %zu frame bytes for %dx%d\n", V, raw.size(), w, h); return 1; }
		std::vector<Image<unsigned short>> views;
		for (size_t v = 0; v < V; v++)
		{
			const float *c = &cams[v * HT_CAM];
			Pose pose; pose.position = { c[5], c[6], c[7] }; pose.orientation = { c[8], c[9], c[10], c[11] };
			std::vector<unsigned short> d(px);
			memcpy(d.data(), raw.data() + v * px * sizeof(unsigned short), px * sizeof(unsigned short));
			views.emplace_back(DCamera({ w, h }, { c[0], c[1] }, { c[2], c[3] }, c[4], pose), std::move(d));
		}
		std::vector<float4> mirrors;
		if (argc >= 7 && strcmp(argv[6], "-"))
		{
			const std::vector<float> p = read_floats(argv[6]);
			if (p.size() != V * 4) { printf("one plane per view\n"); return 1; }
			for (size_t v = 0; v < V; v++) mirrors.push_back({ p[4 * v], p[4 * v + 1], p[4 * v + 2], p[4 * v + 3] });
		}
		HandTracker::ViewOptions options(htk);
		options.fraction = 1;
		const HandTracker::FusedCloud f = htk.FuseViews(views, mirrors, &options);
		printf("views=%zu points=%zu cut=%d\n", V, f.points.size(), f.cut ? 1 : 0);
		for (size_t s = 0; s < f.per_source.size(); s++)
		{
			float sx = 0, sy = 0, sz = 0;      // in the cloud's order, so the sums are exact statements of the points
			for (size_t i = 0; i < f.points.size(); i++) if (f.source[i] == (int)s) { sx += f.points[i].x; sy += f.points[i].y; sz += f.points[i].z; }
			printf("source %zu n=%d sum %a %a %a origin %a %a %a\n", s, f.per_source[s], sx, sy, sz, f.origins[s].x, f.origins[s].y, f.origins[s].z);
		}
		if (track)
		{
			const std::vector<float> start = read_floats(argv[8]);
			std::vector<Pose> pose(start.size() / HT_POSE);
			for (size_t b = 0; b < pose.size(); b++) { const float *p = &start[b * HT_POSE]; pose[b].position = { p[0], p[1], p[2] }; pose[b].orientation = { p[3], p[4], p[5], p[6] }; }
			htk.SetPose(pose);
			const std::vector<Pose> out = htk.update_views(views, mirrors, 3, &options);
			printf("pose");
			for (const Pose &p : out) printf(" %a %a %a %a %a %a %a", p.position.x, p.position.y, p.position.z, p.orientation.x, p.orientation.y, p.orientation.z, p.orientation.w);
			printf("\n");
		}
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
	return 0;
}
