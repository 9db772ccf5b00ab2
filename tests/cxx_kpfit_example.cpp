// HandTracker::fit_keypoints from C++: a start pose and 3-D targets for the skeleton keypoints in, the fitted pose and every keypoint's residual out.
//   cxx_kpfit_example model.htfx start.f32 targets.f32      start: centre-of-mass poses [nb][7] (what SetPose takes), targets: [K][3], raw fp32
// Prints the residuals before and after as hexadecimal floats (exact), one line each; tests/test_gpu_kpfit.py compares them with the C calls'.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include "../include/ht_handtrack.hpp"
using namespace ht_mi355x;
static std::vector<float> read_floats(const char *path)
{
	std::ifstream is(path, std::ios_base::binary);
	if (!is.is_open()) throw std::runtime_error(std::string("cannot open ") + path);
	std::vector<char> b((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
	std::vector<float> f(b.size() / sizeof(float));
	memcpy(f.data(), b.data(), f.size() * sizeof(float));
	return f;
}
int main(int argc, char **argv)
{
	if (argc < 4) { printf("usage: %s model.htfx start.f32 targets.f32\n", argv[0]); return 2; }
	try
	{
		HandTracker htk(argv[1], "");
		const std::vector<ModelFeaturePoint> table = htk.handmodel.GetKeypoints(HT_KP_SKELETON);
		const std::vector<float> start = read_floats(argv[2]), xyz = read_floats(argv[3]);
		if (start.size() % HT_POSE || xyz.size() != table.size() * 3) { printf("the files do not match the model: %zu pose floats, %zu target floats, %zu keypoints\n", start.size(), xyz.size(), table.size()); return 1; }
		std::vector<Pose> pose(start.size() / HT_POSE);
		for (size_t b = 0; b < pose.size(); b++) { const float *p = &start[b * HT_POSE]; pose[b].position = { p[0], p[1], p[2] }; pose[b].orientation = { p[3], p[4], p[5], p[6] }; }
		htk.SetPose(pose);
		HandTracker::KeypointTargets targets;
		for (size_t k = 0; k < table.size(); k++) targets.xyz.push_back({ xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2] });
		HandTracker::KeypointFit options;      // slowfit's figures: 6 steps, the momenta zeroed after every step
		options.max_force = 100000.0f;
		const HandTracker::KeypointFitResult r = htk.fit_keypoints(table, targets, options);
		printf("bones=%zu keypoints=%zu\n", r.pose.size(), table.size());
		printf("resid"); for (float v : r.before) printf(" %a", v); printf("\n");
		printf("resid"); for (float v : r.after) printf(" %a", v); printf("\n");
		double a = 0, b = 0; for (size_t k = 0; k < table.size(); k++) { a += r.before[k]; b += r.after[k]; }
		printf("mean residual %.3f mm -> %.4f mm\n", 1e3 * a / table.size(), 1e3 * b / table.size());
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
	return 0;
}
