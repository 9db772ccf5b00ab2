// HandTracker::left_hand and PhysModel::Mirror of include/ht_handtrack.hpp, headless (the pattern of tests/cxx_joints_driver.cpp; needs the GPU):
//   driver <model> <weights.cnnb> <in.bin> <out.bin>
// in.bin: int32 w, h, nb; then { u16 depth[h*w]; f32 cam[12]; f32 start[nb][7] } twice: a frame as a right hand's tracker takes it, and the same frame flipped with
// its camera and start poses mirrored (the caller's own arithmetic), for a tracker with left_hand set.
// out.bin: for the right tracker, then the left one: f32 update[nb][7], GetPose[nb][7], GetPoseUser[nb][7], then GetMeshes(0) and GetMeshes(1), each mesh as
// { int32 nv, nt; f32 pose[7]; f32 verts[nv][3]; int32 tris[nt][3] }; then an untracked PhysModel's meshes (0 and 1) before and after Mirror(), and after a second Mirror().
#define HT_MI355X_GLOBAL_NAMES
#include <cstdio>
#include <cstring>
#include "../include/ht_formats.hpp"

static std::vector<Pose> poses_of(const float *p, int nb) { std::vector<Pose> v(nb); for (int b = 0; b < nb; b++) { v[b].position = { p[7 * b], p[7 * b + 1], p[7 * b + 2] }; v[b].orientation = { p[7 * b + 3], p[7 * b + 4], p[7 * b + 5], p[7 * b + 6] }; } return v; }
static void put_pose(FILE *f, const Pose &p) { const float r[7] = { p.position.x, p.position.y, p.position.z, p.orientation.x, p.orientation.y, p.orientation.z, p.orientation.w }; fwrite(r, 4, 7, f); }
static void put_poses(FILE *f, const std::vector<Pose> &v) { for (auto &p : v) put_pose(f, p); }
static void put_meshes(FILE *f, const std::vector<Mesh> &ms)
{
	for (auto &m : ms)
	{
		const int n[2] = { (int)m.verts.size(), (int)m.tris.size() };
		fwrite(n, 4, 2, f); put_pose(f, m.pose);
		for (auto &v : m.verts) fwrite(&v.x, 4, 3, f);
		for (auto &t : m.tris) fwrite(&t.x, 4, 3, f);
	}
}
static DCamera camera_of(const float *c, int w, int h) { Pose p; p.position = { c[5], c[6], c[7] }; p.orientation = { c[8], c[9], c[10], c[11] }; return DCamera({ w, h }, { c[0], c[1] }, { c[2], c[3] }, c[4], p); }

int main(int argc, char **argv)
{
	if (argc < 5) { printf("usage: %s <model> <cnnb> <in> <out>\n", argv[0]); return 2; }
	try
	{
		FILE *f = fopen(argv[3], "rb"); if (!f) throw std::runtime_error("cannot open input");
		int hdr[3]; if (fread(hdr, 4, 3, f) != 3) throw std::runtime_error("short input");
		const int w = hdr[0], h = hdr[1], nb = hdr[2];
		HandTracker right(argv[1], argv[2]), left(argv[1], argv[2]);
		left.left_hand = true;
		FILE *o = fopen(argv[4], "wb"); if (!o) throw std::runtime_error("cannot open output");
		for (HandTracker *htk : { &right, &left })
		{
			htk->microforce = 3.0f; htk->mainthreadpasses = 3;
			std::vector<unsigned short> depth((size_t)w * h); float cam[12]; std::vector<float> a((size_t)nb * 7);
			if (fread(depth.data(), 2, depth.size(), f) != depth.size() || fread(cam, 4, 12, f) != 12 || fread(a.data(), 4, a.size(), f) != a.size()) throw std::runtime_error("short record");
			htk->SetPose(poses_of(a.data(), nb));
			put_poses(o, htk->update(Image<unsigned short>(camera_of(cam, w, h), depth)));
			put_poses(o, htk->handmodel.GetPose()); put_poses(o, htk->handmodel.GetPoseUser());
			put_meshes(o, htk->handmodel.GetMeshes(0)); put_meshes(o, htk->handmodel.GetMeshes(1));
		}
		PhysModel fake = LoadHandModel(argv[1]);
		for (int k = 0; k < 3; k++)
		{
			if (k) fake.Mirror();
			put_meshes(o, fake.GetMeshes(0)); put_meshes(o, fake.GetMeshes(1));
		}
		fclose(o); fclose(f);
		printf("hands: %d x %d, %d bones, cnn_input %d x %d\n", w, h, nb, left.cnn_input.dim().x, left.cnn_input.dim().y);
		return 0;
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
}
