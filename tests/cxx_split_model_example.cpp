// Compile-and-link check of SplitHandsByModel and TwoHandTracker::split_mode of the C++ compatibility header (and, on a GPU box, one frame in which two hands touch:
// one blob, which the blob split gives to one hand and the model split cuts in two).
#include <cstdio>
#include "../include/ht_handtrack.hpp"
using namespace ht_mi355x;
int main(int argc, char **argv)
{
	if (argc < 2) { printf("usage: %s model.htfx [weights.cnnb]\n", argv[0]); return 2; }
	try
	{
		Image<unsigned short> frame(DCamera({ 64, 48 }, { 61.f, 61.f }, { 32.f, 24.f }, 0.001f));
		for (auto &d : frame.raster) d = 4000;
		for (int y = 8; y < 40; y++) for (int x = 8; x < 56; x++) frame.pixel({ x, y }) = 450;      // one blob of 12 x 8 cells across the optical axis
		TwoHandTracker two(argv[1], "");
		int nb = 0; ht_model_info(two.context(), &nb, nullptr, nullptr);
		// every body of the right hand 0.08 m right of the axis, every body of the left hand as far left of it, 0.45 m away
		Pose pr, pl; pr.position = { 0.08f, 0.f, 0.45f }; pl.position = { -0.08f, 0.f, 0.45f }; pr.orientation = pl.orientation = { 0.f, 0.f, 0.f, 1.f };
		const std::vector<Pose> right((size_t)nb, pr), left((size_t)nb, pl);
		const SplitResult blobs = SplitHands(frame, 100, 650, 4000, 65535, 4);
		const SplitModelResult s = SplitHandsByModel(frame, right, left, 100, 650, 4000, std::numeric_limits<float>::infinity(), HT_SPLIT_MODEL_MERGED, 65535, 4, HT_SPLIT_MIRROR_LEFT);
		printf("blob split components %d present %d %d; model split source %d right %d cells from %d left %d cells to %d mirrored pixel %d\n", blobs.n_components, (int)blobs.present[0], (int)blobs.present[1], s.source,
		       s.info[0][0], s.info[0][4], s.info[1][0], s.info[1][6], (int)s.left.raster[(size_t)8 * 64 + 63 - 8]);
		if (blobs.n_components != 1 || (blobs.present[0] && blobs.present[1])) return 4;
		// the cells whose first pixel is on the axis or right of it are the right hand's (a tie goes to the right hand)
		if (s.source != 1 || !s.present[0] || !s.present[1] || s.info[0][0] != 48 || s.info[1][0] != 48 || s.info[0][4] != 8 || s.info[1][6] != 7) return 5;
		if (s.left.raster[(size_t)8 * 64 + 63 - 8] != 450 || s.right.raster[(size_t)8 * 64 + 32] != 450 || s.right.raster[(size_t)8 * 64 + 31] != 4000) return 6;
		try { SplitHandsByModel(frame, right, left, 100, 650, 4000, -1.0f); printf("a negative max_dist, yet split\n"); return 3; } catch (const std::runtime_error &e) { printf("refused: %s\n", e.what()); }
		if (argc > 2)
		{
			TwoHandTracker tracked(argv[1], argv[2]);
			tracked.min_pixels = 4;
			tracked.SetPose(right, left);
			const TwoHandTracker::Hands lost = tracked.update(frame);      // split_mode Blobs, the default: one hand is absent
			tracked.SetPose(right, left);
			tracked.split_mode = TwoHandTracker::ModelWhenMerged;
			const TwoHandTracker::Hands both = tracked.update(frame);
			tracked.SetPose(right, left);
			tracked.split_mode = TwoHandTracker::ModelAlways; tracked.max_dist = 0.5f;
			const TwoHandTracker::Hands always = tracked.update(frame);
			printf("update blobs: source %d present %d %d; merged: source %d right %d left %d; always: source %d right %d left %d\n", lost.source, (int)lost.present[0], (int)lost.present[1], both.source,
			       both.info[0][0], both.info[1][0], always.source, always.info[0][0], always.info[1][0]);
			if (lost.source != 0 || (lost.present[0] && lost.present[1])) return 7;
			if (both.source != 1 || both.info[0][0] != 48 || both.info[1][0] != 48 || always.source != 1 || always.info[0][0] != 48 || always.info[1][0] != 48) return 8;
		}
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
	return 0;
}
