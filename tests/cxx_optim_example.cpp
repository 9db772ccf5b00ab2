// The optimiser additions of the C++ compatibility header: Optimizer, CNN::GradBatch, CNN::Step (and CNN::TrainOpt, compiled only: it takes device pools).
// in.cnnb, samples.bin (n x 4096 inputs, then n x 2304 labels, float32), n -> two momentum steps, each on all n samples; out.cnnb takes the stepped weights
// and out.mse the 2 x n losses, for tests/test_gpu_optim.py to hold against the C calls.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include "../include/ht_handtrack.hpp"
using namespace ht_mi355x;
int main(int argc, char **argv)
{
	if (argc < 6) { printf("usage: %s in.cnnb samples.bin n out.cnnb out.mse\n", argv[0]); return 2; }
	try
	{
		const size_t n = (size_t)atoi(argv[3]);
		std::vector<float> x(n * HT_CNN_IN), t(n * HT_CNN_OUT);
		std::ifstream is(argv[2], std::ios_base::binary);
		is.read((char *)x.data(), (std::streamsize)(x.size() * sizeof(float)));
		is.read((char *)t.data(), (std::streamsize)(t.size() * sizeof(float)));
		if (!is) { printf("short samples file\n"); return 3; }
		Optimizer o(HT_OPT_MOMENTUM);
		if (o.opt.kind != HT_OPT_MOMENTUM || o.opt.momentum != 0.9f || o.opt.lr != 0.001f || o.opt.grad_scale != 1.0f || o.opt.clip_norm != 0.0f) return 4;
		try { Optimizer bad(7); return 5; } catch (const std::runtime_error &) {}
		o.opt.lr = 0.002f; o.opt.grad_scale = 0.5f;
		CNN cnn = PoseInitializerCNN(argv[1]);
		std::ofstream ms(argv[5], std::ios_base::binary);
		for (int k = 0; k < 2; k++)
		{
			const std::vector<float> mse = cnn.GradBatch(x, t);
			cnn.Step(o);
			ms.write((const char *)mse.data(), (std::streamsize)(mse.size() * sizeof(float)));
		}
		cnn.saveb(std::string(argv[4]));
		if (false) cnn.TrainOpt(nullptr, nullptr, 0, std::vector<int>(), 1, 1, o);      // compiled, not run
		printf("two momentum steps on %d samples\n", (int)n);
	}
	catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
	return 0;
}
