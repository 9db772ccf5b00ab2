// Compile-and-link check of SplitHands and TwoHandTracker of the C++ compatibility header (and, on a GPU box, one split frame and one two-hand update).
#include <cstdio>
#include "../include/ht_handtrack.hpp"
using namespace ht_mi355x;
int main(int argc, char **argv)
{
	if (argc < 2) { printf("usage: %s model.htfx\n", argv[0]); return 2; }
	try
	{
		Image<unsigned short> frame(DCamera({ 64, 48 }, { 61.f, 61.f }, { 32.f, 24.f }, 0.001f));
		for (auto &d : frame.raster) d = 4000;
		for (int y = 8; y < 40; y++) for (int x = 4; x < 20; x++) frame.pixel({ x, y }) = 400;                    // 4 x 8 cells at low x
		for (int y = 12; y < 36; y++) for (int x = 40; x < 60; x++) frame.pixel({ x, y }) = (unsigned short)(450 + x);      // 5 x 6 cells at high x
		try { SplitHands(frame, 100, 650, 4000); printf("no tracker, yet split\n"); return 3; } catch (const std::runtime_error &) {}      // the split runs on a tracker's device
		TwoHandTracker two(argv[1], "");
		const SplitResult s = SplitHands(frame, 100, 650, 4000, 65535, 4, HT_SPLIT_MIRROR_LEFT);
		printf("split components %d right %d cells at %d left %d cells at %d mirrored pixel %d principal %g\n", s.n_components, s.info[0][0], s.info[0][4], s.info[1][0], s.info[1][4],
		       (int)s.left.raster[(size_t)8 * 64 + 63 - 4], s.left.cam.principal().x);
		if (!s.present[0] || !s.present[1] || s.info[0][0] != 30 || s.info[1][0] != 32 || s.left.raster[(size_t)8 * 64 + 63 - 4] != 400 || s.right.raster[(size_t)12 * 64 + 40] != 490) return 4;
		two.min_pixels = 4;
		try { two.update(frame); printf("no weights, yet updated\n"); return 3; } catch (const std::runtime_error &e) { printf("update without weights: %s\n", e.what()); }
		if (argc > 2)
		{
			TwoHandTracker tracked(argv[1], argv[2]);
			tracked.min_pixels = 4;
			const TwoHandTracker::Hands hands = tracked.update(frame);
			printf("update right %d cells left %d cells poses %d %d\n", hands.info[0][0], hands.info[1][0], (int)hands.right.size(), (int)hands.left.size());
			if (!hands.present[0] || !hands.present[1] || hands.info[0][0] != 30 || hands.info[1][0] != 32 || hands.right.size() != hands.left.size() || hands.right.empty()) return 5;
			tracked.right_is_low_x = true;
			const TwoHandTracker::Hands swapped = tracked.update(frame);
			if (swapped.info[0][0] != 32 || swapped.info[1][0] != 30) return 6;
			for (int y = 8; y < 40; y++) for (int x = 4; x < 20; x++) frame.pixel({ x, y }) = 4000;      // the hand at low x leaves
			const TwoHandTracker::Hands one = tracked.update(frame);
			printf("one hand: right %d left %d\n", (int)one.present[0], (int)one.present[1]);
			if (one.present[0] || !one.present[1] || one.info[1][0] != 30) return 7;      // (right_is_low_x: what is left at high x is the left hand)
		}
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
	return 0;
}
