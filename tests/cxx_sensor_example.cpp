// Compile-and-link check of the RSCam facade of the C++ compatibility header (and, on a GPU box, one filtered frame of each kind).
#include <cstdio>
#include "../include/ht_handtrack.hpp"
using namespace ht_mi355x;
int main(int argc, char **argv)
{
	if (argc < 2) { printf("usage: %s model.htfx\n", argv[0]); return 2; }
	int wo = 0, ho = 0;
	if (ht_sensor_out_dims(HT_SENSOR_IVY, 640, 480, 320, &wo, &ho) != HT_OK || wo != 320 || ho != 240) { printf("out_dims wrong\n"); return 3; }
	try
	{
		RSCam cam;
		Image<unsigned short> raw(DCamera({ 640, 480 }, { 610.f, 610.f }, { 320.f, 240.f }, 0.001f));
		for (size_t i = 0; i < raw.raster.size(); i++) raw.raster[i] = (unsigned short)(i % 7 ? 500 + i % 640 : 0);
		try { cam.FilterIvy(raw); printf("no tracker, yet filtered\n"); return 3; } catch (const std::runtime_error &) {}      // the filters run on a HandTracker's device
		HandTracker htk(argv[1], "");
		Image<unsigned short> ivy = cam.FilterIvy(raw);
		printf("ivy %dx%d focal %g principal %g first %d\n", ivy.dim().x, ivy.dim().y, ivy.cam.focal().x, ivy.cam.principal().y, (int)ivy.raster[0]);
		Image<unsigned short> r200(DCamera({ 320, 240 }, { 305.f, 305.f }, { 160.f, 120.f }, 0.001f));
		Image<unsigned char> ir(r200.cam);
		for (auto &d : r200.raster) d = 700; for (auto &l : ir.raster) l = 100;
		r200.pixel({ 100, 100 }) = 900; ir.pixel({ 5, 5 }) = 0;
		cam.addbackground(r200);
		Image<unsigned short> ds4 = cam.FilterDS4(r200, ir);
		printf("ds4 %dx%d flying %d dark %d behind %d\n", ds4.dim().x, ds4.dim().y, (int)ds4.pixel({ 100, 100 }), (int)ds4.pixel({ 5, 5 }), (int)ds4.pixel({ 50, 50 }));
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
	return 0;
}
