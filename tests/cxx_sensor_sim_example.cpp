// Compile-and-link check of the sensor-simulation additions of the C++ compatibility header: SensorNoise, RSCam::SimulateIvy, RSCam::SimulateDS4 and cache_ir
// (and, on a GPU box, a rendered hand made raw for either camera and handed to the camera's own filter).
#include <cstdio>
#include "../include/ht_handtrack.hpp"
using namespace ht_mi355x;
int main(int argc, char **argv)
{
	if (argc < 2) { printf("usage: %s model.htfx\n", argv[0]); return 2; }
	try
	{
		const SensorNoise off, ivy(HT_SENSOR_IVY, 0.001f), ds4(HT_SENSOR_DS4, 0.001f, 4.0f);
		if (off.p_hole != 0 || off.far_count != 3999 || ivy.far_count != 3999 || ivy.disparity_k != 0 || ds4.disparity_k <= 0 || ivy.sigma0_256 <= ds4.sigma0_256) { printf("defaults wrong\n"); return 3; }
		try { SensorNoise(7); printf("kind 7, yet a noise set\n"); return 3; } catch (const std::runtime_error &) {}
		try { SensorNoise(HT_SENSOR_IVY, 0.0f); printf("scale 0, yet a noise set\n"); return 3; } catch (const std::runtime_error &) {}
		RSCam cam;
		Image<unsigned short> flat(DCamera({ 160, 120 }, { 150.f, 150.f }, { 80.f, 60.f }, 0.001f));
		try { cam.SimulateIvy(flat, off); printf("no tracker, yet simulated\n"); return 3; } catch (const std::runtime_error &) {}      // it runs on a HandTracker's device
		HandTracker ht(argv[1], "");
		std::vector<Pose> rest = LoadHandModel(argv[1]).GetPose();      // 0.3 m further out the rest pose is in front of the camera
		for (auto &p : rest) p.position.z += 0.3f;
		ht.SetPose(rest);
		const Image<unsigned short> clean = ht.render_depth(ht.handmodel.GetPose(), flat.cam);
		// everything off: the hand unchanged, the 4 m background reported as "no data"
		const Image<unsigned short> same = cam.SimulateIvy(clean, off);
		int hand = 0;
		for (size_t i = 0; i < clean.raster.size(); i++)
		{
			const bool fg = clean.raster[i] != 0 && clean.raster[i] < 3999;
			hand += fg;
			if (same.raster[i] != (fg ? clean.raster[i] : 0)) { printf("pixel %d: %d from %d with everything off\n", (int)i, (int)same.raster[i], (int)clean.raster[i]); return 4; }
		}
		if (hand < 100) { printf("%d hand pixels in the frame\n", hand); return 4; }
		// the default sets: reproducible, seeded, frayed
		SensorNoise other = ivy; other.seed = 99;
		const Image<unsigned short> a = cam.SimulateIvy(clean, ivy), b = cam.SimulateIvy(clean, ivy), c = cam.SimulateIvy(clean, other);
		int changed = 0, lost = 0;
		for (size_t i = 0; i < a.raster.size(); i++) { changed += a.raster[i] != same.raster[i]; lost += a.raster[i] == 0 && same.raster[i] != 0; }
		if (a.raster != b.raster || a.raster == c.raster || changed == 0 || lost == 0 || a.dim().x != 160 || a.cam.focal().x != 150.f) { printf("ivy: changed %d lost %d\n", changed, lost); return 5; }
		Image<unsigned short> filtered = cam.FilterIvy(a);
		printf("ivy: %d hand pixels, %d changed, %d lost; filtered %dx%d first %d\n", hand, changed, lost, filtered.dim().x, filtered.dim().y, (int)filtered.raster[0]);
		if (filtered.raster[0] != 3999) return 5;
		Image<unsigned char> ir;
		const Image<unsigned short> raw = cam.SimulateDS4(clean, ds4, &ir);
		if (ir.raster != cam.cache_ir.raster || ir.raster.size() != raw.raster.size()) return 6;
		int dark = 0;
		for (size_t i = 0; i < raw.raster.size(); i++) { if ((raw.raster[i] == 0) != (ir.raster[i] < 8)) { printf("pixel %d: depth %d, ir %d\n", (int)i, (int)raw.raster[i], (int)ir.raster[i]); return 6; } dark += ir.raster[i] < 8; }
		const Image<unsigned short> kept = cam.FilterDS4(raw, cam.cache_ir);
		int left = 0;
		for (size_t i = 0; i < kept.raster.size(); i++) { if (ir.raster[i] < 8 && kept.raster[i] != 4096) return 7; left += kept.raster[i] != 4096; }
		printf("ds4: %d dark pixels, %d kept by FilterDS4\n", dark, left);
		if (dark == 0 || left == 0) return 7;
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
	return 0;
}
