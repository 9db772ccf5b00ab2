// The joint-coordinate additions of include/ht_handtrack.hpp on a tracked hand, headless (the pattern of tests/cxx_headless_driver.cpp; needs the GPU):
//   driver <model> <weights.cnnb> <in.bin> <out.bin>
// in.bin as cxx_headless_driver.cpp reads it: int32 n, w, h, nb; then n records { u16 depth[h*w]; f32 cam[12]; f32 start[nb][7]; f32 gt[nb][7] }.
// Per record: the tracker is started at `start`, updated on the frame, and the tracked model is read out, rebuilt from its own coordinates and read again.
// out.bin: n records { f32 before[nb][7] (GetPose); f32 coords[nj][3]; f32 degrees[nj][3]; f32 gaps[nj]; f32 after[nb][7]; f32 coords_after[nj][3]; f32 gaps_after[nj] }
#define HT_MI355X_GLOBAL_NAMES
#include <cstdio>
#include <cstring>
#include "../include/ht_formats.hpp"

static std::vector<Pose> poses_of(const float *p, int nb) { std::vector<Pose> v(nb); for (int b = 0; b < nb; b++) { v[b].position = { p[7 * b], p[7 * b + 1], p[7 * b + 2] }; v[b].orientation = { p[7 * b + 3], p[7 * b + 4], p[7 * b + 5], p[7 * b + 6] }; } return v; }
static void put_poses(FILE *f, const std::vector<Pose> &v) { for (auto &p : v) { const float r[7] = { p.position.x, p.position.y, p.position.z, p.orientation.x, p.orientation.y, p.orientation.z, p.orientation.w }; fwrite(r, 4, 7, f); } }
static void put3(FILE *f, const std::vector<float3> &v) { for (auto &a : v) { const float r[3] = { a.x, a.y, a.z }; fwrite(r, 4, 3, f); } }
static DCamera camera_of(const float *c, int w, int h) { Pose p; p.position = { c[5], c[6], c[7] }; p.orientation = { c[8], c[9], c[10], c[11] }; return DCamera({ w, h }, { c[0], c[1] }, { c[2], c[3] }, c[4], p); }

int main(int argc, char **argv)
{
	if (argc < 5) { printf("usage: %s <model> <cnnb> <in> <out>\n", argv[0]); return 2; }
	try
	{
		FILE *f = fopen(argv[3], "rb"); if (!f) throw std::runtime_error("cannot open input");
		int hdr[4]; if (fread(hdr, 4, 4, f) != 4) throw std::runtime_error("short input");
		const int n = hdr[0], w = hdr[1], h = hdr[2], nb = hdr[3];
		HandTracker htk(argv[1], argv[2]);
		htk.microforce = 3.0f; htk.mainthreadpasses = 3;
		FILE *o = fopen(argv[4], "wb"); if (!o) throw std::runtime_error("cannot open output");
		size_t nj = 0;
		for (int k = 0; k < n; k++)
		{
			std::vector<unsigned short> depth((size_t)w * h); float cam[12]; std::vector<float> a((size_t)nb * 7), b((size_t)nb * 7);
			if (fread(depth.data(), 2, depth.size(), f) != depth.size() || fread(cam, 4, 12, f) != 12 || fread(a.data(), 4, a.size(), f) != a.size() || fread(b.data(), 4, b.size(), f) != b.size()) throw std::runtime_error("short record");
			htk.SetPose(poses_of(a.data(), nb));
			htk.update(Image<unsigned short>(camera_of(cam, w, h), depth));
			put_poses(o, htk.handmodel.GetPose());
			const std::vector<float3> c = htk.handmodel.GetJointCoords();
			nj = c.size();
			put3(o, c); put3(o, htk.handmodel.JointAngles());
			const std::vector<float> g = htk.handmodel.GetJointGaps(); fwrite(g.data(), 4, g.size(), o);
			htk.handmodel.SetJointCoords(c);
			put_poses(o, htk.handmodel.GetPose());
			put3(o, htk.handmodel.GetJointCoords());
			const std::vector<float> g2 = htk.handmodel.GetJointGaps(); fwrite(g2.data(), 4, g2.size(), o);
		}
		fclose(o); fclose(f);
		printf("joints: %d frames, %d bones, %zu joints\n", n, nb, nj);
		return 0;
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
}
