// Compile-and-link check of the accuracy additions of the C++ compatibility header: Skin, ImageFeaturePoints, handmodel.GetKeypoints, HandTracker::keypoints and
// HandTracker::depth_residual (and, on a GPU box, each of them once on the model's rest pose and a frame rendered from it).
#include <cmath>
#include <cstdio>
#include "../include/ht_handtrack.hpp"
using namespace ht_mi355x;
int main(int argc, char **argv)
{
	if (argc < 2) { printf("usage: %s model.htfx\n", argv[0]); return 2; }
	try
	{
		const DCamera cam({ 64, 48 }, { 60.f, 60.f }, { 32.f, 24.f }, 0.001f);
		try { Skin(std::vector<Pose>(17), handmodelfeaturepoints); printf("no tracker, yet skinned\n"); return 3; } catch (const std::runtime_error &) {}      // they run on a tracker's device
		HandTracker ht(argv[1], "");
		std::vector<Pose> rest = LoadHandModel(argv[1]).GetPose();      // the model's rest pose reaches back to the origin: 0.3 m further out it is in front of the camera
		for (auto &p : rest) p.position.z += 0.3f;
		ht.SetPose(rest);
		const std::vector<Pose> pose = ht.handmodel.GetPose();
		const std::vector<float3> x = Skin(pose, handmodelfeaturepoints);
		const std::vector<float2> u = ImageFeaturePoints(pose, handmodelfeaturepoints, cam);
		if (x.size() != 8 || u.size() != 8) return 4;
		for (int k = 0; k < 8; k++)
		{
			const float3 want = pose[handmodelfeaturepoints[k].bone] * handmodelfeaturepoints[k].offset;      // Skin, handtrack.h:82
			const float2 wu = { want.x / want.z * 60.f + 32.f, want.y / want.z * 60.f + 24.f };               // projectz: the camera's pose is the identity
			if (!(want.z > 0.1f) || !(std::fabs(x[k].x - want.x) <= 1e-6f) || !(std::fabs(x[k].y - want.y) <= 1e-6f) || !(std::fabs(x[k].z - want.z) <= 1e-6f) || !(std::fabs(u[k].x - wu.x) <= 1e-3f) || !(std::fabs(u[k].y - wu.y) <= 1e-3f)) return 5;
		}
		const std::vector<ModelFeaturePoint> f8 = ht.handmodel.GetKeypoints(HT_KP_FEATURE8), sk = ht.handmodel.GetKeypoints(HT_KP_SKELETON);
		printf("tables %d %d tip bone %d rel %d\n", (int)f8.size(), (int)sk.size(), f8[7].bone, f8[7].rel);
		if (f8.size() != 8 || f8[7].bone != 16 || f8[1].offset.x != -0.03f || f8[1].rel != 1 || sk.size() < 3 || sk[0].bone != 0 || sk[0].rel != 0) return 6;
		const Image<unsigned short> frame = ht.render_depth(pose, cam);
		const HandTracker::Keypoints kp = ht.keypoints(frame);
		if (kp.xyz.size() != 8 || kp.pixels.size() != 8 || kp.visibility.size() != 8) return 7;
		int seen = 0;
		for (int k = 0; k < 8; k++)
		{
			if (kp.pixels[k].x != u[k].x || kp.pixels[k].y != u[k].y || kp.visibility[k] > 4) { printf("keypoint %d: pixel %g %g against %g %g, visibility %d\n", k, kp.pixels[k].x, kp.pixels[k].y, u[k].x, u[k].y, (int)kp.visibility[k]); return 8; }
			seen += kp.visibility[k] == 0;
		}
		const HandTracker::DepthResidual r = ht.depth_residual(frame, { 0.1f, 1.0f });
		printf("visible %d of 8; residual: observed %lld rendered %lld both %lld iou %g mean %g max %g\n", seen, r.n_observed, r.n_rendered, r.n_both, r.iou, r.mean_abs, r.max_abs);
		if (r.n_both == 0 || r.n_observed != r.n_rendered || r.n_both != r.n_observed || r.iou != 1.0 || r.max_abs != 0.0 || r.n_close != r.n_both) return 9;      // the frame IS the model's rendering
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
	return 0;
}
