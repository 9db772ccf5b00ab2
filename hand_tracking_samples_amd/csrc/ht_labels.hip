// ht_labels.hip -- training samples on the device: the net's expected output (GatherHandExpectedCNN) for a batch of poses, and the net's input of
// a batch of 64x64 tiles.  Together with ht_render_depth_dev, ht_segment_vr_dev and ht_cnn_train_dev they keep train-cnn's loop on the GPU.
//
// Reference computations:
//   GatherHandExpectedCNN          handtrack.h:160-173 (ImageFeaturePoints :92-96, HandPoseToKeyAngleSet :132-151)
//   RenderHeatMap / Normalize      misc_image.h:246-272 (2-D landmark maps), Render1DHeatMaps misc_image.h:281-295 (1-D key-angle maps)
//   compress                       train-hand-pose-cnn/train-cnn.cpp:31-50 (poses into the segment's camera frame, the camera at the identity)
//   cnn_input of a tile            handtrack.h:700
// The host statement of the labels is ht_expected_cnn_full (ht_api.hip); every value below follows its expression tree, so the labels are
// bit-identical to it (tests/test_gpu_labels.py; DESIGN section 18 has the parity argument).
//
// Mapping: one wave per frame, four frames per block of 256 threads.
//   lanes 0..7    landmark k: projection, the 5x5 window of its 2-D map into the frame's LDS byte image, sum, normalisation
//   lanes 8..23   key angle k - 8 (nine are defined, the rest are 0), into LDS and `vals`
//   lanes 0..15   after a barrier: the 1-D map row of key angle k
//   all lanes     the 2304 bytes as k / 255 through a 256-entry LDS table, written as coalesced float4 rows (576 per frame, 9 per lane)
#include <limits.h>
#include "ht_device.hpp"
#include "ht_host.hpp"
#include "ht_expf.hpp"

#define LB_FRAMES 4             // frames (waves) per block
#define LB_THREADS (64 * LB_FRAMES)

// x86's truncating float -> int conversion (cvttss2si), which the host statement compiles to: NaN and out-of-range values give INT_MIN.
// A plain (int) cast of such a value is undefined in C and is not what the host does.
__device__ __forceinline__ long long lb_trunc(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (long long)(int)f : (long long)INT_MIN; }
__device__ __forceinline__ unsigned char lb_gray(float x) { float v = x * 255.0f; v = fmin_std(fmax_std(v, 0.0f), 255.0f); return (unsigned char)v; }      // gray_of

__global__ __launch_bounds__(LB_THREADS) void k_expected_cnn(const float *__restrict__ poses, const float *__restrict__ cams, int nb, int B, int segment_frame, float sub,
                                                             float *__restrict__ expected, float *__restrict__ image_points, float *__restrict__ vals_out)
{
	__shared__ __attribute__((aligned(16))) unsigned char img[LB_FRAMES][HT_CNN_OUT];
	__shared__ float s_vals[LB_FRAMES][16];
	__shared__ float s_div[256];                     // k / 255.0f, correctly rounded (the host's img[i] / 255.0f)
	__shared__ uint64_t s_exptab[32];
	const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const long long f = (long long)blockIdx.x * LB_FRAMES + wv;
	const bool live = f < B;
	s_div[threadIdx.x] = (float)threadIdx.x / 255.0f;
	if (threadIdx.x < 32) { const uint64_t t[32] = HT_EXPF_TABLE; s_exptab[threadIdx.x] = t[threadIdx.x]; }
	unsigned char *h = img[wv];
	for (int i = lane; i < HT_CNN_OUT / 16; i += 64) reinterpret_cast<uint4 *>(h)[i] = make_uint4(0, 0, 0, 0);
	__syncthreads();
	const float *pose = poses + (live ? (size_t)f * nb * HT_POSE : 0);
	const float *cam = cams + (live ? (size_t)f * HT_CAM : 0);
	xf campose = XF(V3(cam[5], cam[6], cam[7]), V4(cam[8], cam[9], cam[10], cam[11]));
	const xf cinv = inverse(campose);
	if (segment_frame) campose = XF(V3(0.0f, 0.0f, 0.0f), V4(0.0f, 0.0f, 0.0f, 1.0f));      // compress: the camera at the identity, ...
	const xf ci = inverse(campose);
	auto P = [&](int b) {
		const float *p = pose + HT_POSE * b;
		const xf x = XF(V3(p[0], p[1], p[2]), V4(p[3], p[4], p[5], p[6]));
		return segment_frame ? mul(cinv, x) : x;      // ... every pose re-expressed as cam.pose.inverse() * p
	};
	if (live && lane < 8)
	{
		const int k = lane;
		const int b = k == 0 || k == 1 || k == 2 ? 1 : 3 * k - 5;      // fbone = { 1, 1, 1, 4, 7, 10, 13, 16 }
		const v3 off = V3(k == 1 ? -0.03f : k == 2 ? 0.03f : 0.0f, 0.0f, k == 1 || k == 2 ? -0.03f : 0.0f);
		const float fx = cam[0] / sub, fy = cam[1] / sub, px = cam[2] / sub, py = cam[3] / sub;      // hcam = camsub(cam, sub): 4 of a 64x64 tile, 8 of a 128x128 one (HT_LABELS_SIDE128)
		const v3 v = apply(ci, apply(P(b), off));
		const float ux = v.x / v.z * fx + px, uy = v.y / v.z * fy + py;
		if (image_points) { image_points[(size_t)f * 16 + 2 * k] = ux; image_points[(size_t)f * 16 + 2 * k + 1] = uy; }
		// the window [h - 2, h + 3) clipped to the map, in wide integers: empty for NaN, infinite or far-off projections
		const long long hx = lb_trunc(ux), hy = lb_trunc(uy);
		const int x0 = (int)(hx - 2 > 0 ? hx - 2 : 0), x1 = (int)(hx + 3 < 16 ? hx + 3 : 16), y0 = (int)(hy - 2 > 0 ? hy - 2 : 0), y1 = (int)(hy + 3 < 16 ? hy + 3 : 16);
		unsigned char *m = h + 256 * k;
		int sum = 0;
		for (int y = y0; y < y1; y++) for (int x = x0; x < x1; x++)
		{
			const float dx = ux - (float)x, dy = uy - (float)y;
			const unsigned char g = lb_gray(ht_expf_glibc(-(dx * dx + dy * dy) / (2.0f * 0.33f), s_exptab));
			m[y * 16 + x] = g; sum += g;
		}
		if (sum) for (int y = y0; y < y1; y++) for (int x = x0; x < x1; x++) m[y * 16 + x] = (unsigned char)(m[y * 16 + x] * 255 / sum);
	}
	if (live && lane >= 8 && lane < 24)
	{
		const int j = lane - 8;
		float val = 0.0f;
		if (j < 9)
		{
			const v4 q1 = P(1).q, palmq = qmul(ci.q, q1);
			if (j == 0) val = (float)(atan2((double)qxdir(palmq).x, (double)-qxdir(palmq).z) / (double)(3.14159f * 2.0f) + (double)0.5f);
			else if (j == 1) val = (float)(asin((double)clamp_std(qzdir(palmq).z, -1.0f, 1.0f)) / (double)3.14159f + (double)0.5f);
			else if (j == 2) val = (float)(asin((double)clamp_std(qzdir(palmq).x, -1.0f, 1.0f)) / (double)3.14159f + (double)0.5f);
			else if (j == 3) val = (float)(acos((double)dot(qxdir(q1), qzdir(P(4).q))) / (double)3.14159f);      // unclamped, as handtrack.h:143: NaN past 1
			else if (j < 8) val = (float)(acos((double)clamp_std(dot(qydir(q1), qydir(P(3 * j - 6).q)), -1.0f, 1.0f)) / (double)3.14159f);      // bones 6, 9, 12, 15
			else { const v3 pz = qzdir(palmq); val = (float)((double)0.5f + atan2((double)-pz.x, (double)-pz.y) / (double)(3.14159f * 2.0f)); }
		}
		s_vals[wv][j] = val;
		if (vals_out) vals_out[(size_t)f * 16 + j] = val;
	}
	__syncthreads();
	if (live && lane < 16)
	{
		const int y = lane;
		const float v = s_vals[wv][y] * (float)(16 - 1);
		const long long c = lb_trunc(v);      // NaN (the thumb angle past 1): INT_MIN, an empty row, as on the host
		const int x0 = (int)(c - 2 > 0 ? c - 2 : 0), x1 = (int)(c + 3 < 16 ? c + 3 : 16);
		unsigned char *m = h + 2048 + 16 * y;
		int sum = 0;
		for (int x = x0; x < x1; x++)
		{
			const double dd = (double)((float)x - v);
			const float d2 = (float)(dd * dd);      // pow(d, 2.0): the square of a float is exact in double
			const unsigned char g = lb_gray((float)exp((double)(-d2 / (2.0f * 0.5f))));
			m[x] = g; sum += g;
		}
		for (int x = x0; sum && x < x1; x++) m[x] = (unsigned char)(m[x] * 255 / sum);
	}
	__syncthreads();
	if (!live) return;
	float4 *out = reinterpret_cast<float4 *>(expected + (size_t)f * HT_CNN_OUT);
	const uchar4 *src = reinterpret_cast<const uchar4 *>(h);
	for (int i = lane; i < HT_CNN_OUT / 4; i += 64)
	{
		const uchar4 u = src[i];
		out[i] = make_float4(s_div[u.x], s_div[u.y], s_div[u.z], s_div[u.w]);
	}
}

static int lb_check_args(ht_ctx *ctx, const void *poses, const void *cams, int B, const void *expected)
{
	if (!poses || !cams || !expected || B < 0) { ctx->err = "ht_expected_cnn: bad argument"; return HT_ERR_ARG; }
	if (ctx->cnn_only) { ctx->err = "this context was created without a hand model (CNN only)"; return HT_ERR_STATE; }
	if (ctx->model.nb < 17) { ctx->err = "ht_expected_cnn: the labels read bones up to 16; the context's model has fewer than 17"; return HT_ERR_ARG; }
	return HT_OK;
}

extern "C" int ht_expected_cnn_dev(ht_ctx *ctx, const float *d_poses, const float *d_cams, int B, int flags, float *d_expected, float *d_image_points, float *d_vals, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = lb_check_args(ctx, d_poses, d_cams, B, d_expected); if (r) return r; }
	if (flags & ~(HT_LABELS_SEGMENT_FRAME | HT_LABELS_SIDE128)) { ctx->err = "ht_expected_cnn: unknown flags"; return HT_ERR_ARG; }
	if (((uintptr_t)d_expected & 15) != 0) { ctx->err = "ht_expected_cnn_dev: d_expected must be 16-byte aligned (the labels are written as float4 rows)"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const int blocks = (int)(((long long)B + LB_FRAMES - 1) / LB_FRAMES);
	hipLaunchKernelGGL(k_expected_cnn, dim3(blocks), dim3(LB_THREADS), 0, s, d_poses, d_cams, ctx->model.nb, B, (flags & HT_LABELS_SEGMENT_FRAME) ? 1 : 0, (float)ht_net_of(ctx, (flags & HT_LABELS_SIDE128) ? 128 : 64)->dims.sub, d_expected, d_image_points, d_vals);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

// the synchronous variant stages through the context's buffer (ht_staged_call; no tracker slot: B is not bounded by max_batch)
extern "C" int ht_expected_cnn_batch(ht_ctx *ctx, const float *poses, const float *cams, int B, int flags, float *expected, float *image_points, float *vals)
{
	CHECK_READY(ctx);
	{ const int r = lb_check_args(ctx, poses, cams, B, expected); if (r) return r; }
	if (flags & ~(HT_LABELS_SEGMENT_FRAME | HT_LABELS_SIDE128)) { ctx->err = "ht_expected_cnn: unknown flags"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	const size_t n = (size_t)B;
	ht_seg seg[5] = { { (void *)poses, n * ctx->model.nb * HT_POSE * sizeof(float), false }, { (void *)cams, n * HT_CAM * sizeof(float), false },
	                  { expected, n * HT_CNN_OUT * sizeof(float), true }, { image_points, n * 16 * sizeof(float), true }, { vals, n * 16 * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 5, [&](hipStream_t s)
	                      { return ht_expected_cnn_dev(ctx, (const float *)seg[0].dev, (const float *)seg[1].dev, B, flags, (float *)seg[2].dev, (float *)seg[3].dev, (float *)seg[4].dev, s); });
}

// cnn_input (handtrack.h:700) of B tiles of a net's input size.  A 64x64 tile: k_prepare without a point cloud, as the full-frame update path runs it
// (ht_solver_api.hip); a larger one: the whole-frame transform that ht_update_direct_* feeds the 128x128-input net with (k_cnn_input)
static int cnn_input_dev(ht_ctx *ctx, const char *fn, const ht_net *net, const uint16_t *d_tiles, const float *d_cams, int B, float *d_cnn_in, void *stream)
{
	const std::string f(fn);
	if (!net) return HT_ERR_ARG;
	if (!d_tiles || !d_cams || !d_cnn_in || B < 0) { ctx->err = f + ": bad argument"; return HT_ERR_ARG; }
	if (((uintptr_t)d_tiles & 15) != 0 || ((uintptr_t)d_cnn_in & 15) != 0) { ctx->err = f + ": d_tiles and d_cnn_in must be 16-byte aligned (the input transform reads eight pixels per 128-bit load and writes float4)"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const size_t npx = net->dims.in;
	if (net->dims.side == 64)
	{
		const ht_prepare_extra pz = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr };
		ht_launch_prepare(d_tiles, d_cams, ctx->par.drangey, ctx->par.subsample_fraction, d_cnn_in, nullptr, nullptr, 0, B, s, &pz);
	}
	else for (int b0 = 0; b0 < B; b0 += 32768)      // (a launch takes one tile per block row, at most 65535)
		ht_launch_cnn_input(d_tiles + (size_t)b0 * npx, d_cams + (size_t)b0 * HT_CAM, (int)npx, ctx->par.drangey, d_cnn_in + (size_t)b0 * npx, B - b0 < 32768 ? B - b0 : 32768, s);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_cnn_input_dev(ht_ctx *ctx, const uint16_t *d_tiles, const float *d_cams, int B, float *d_cnn_in, void *stream)
{
	CHECK_READY(ctx);
	return cnn_input_dev(ctx, "ht_cnn_input_dev", ht_net_of(ctx, 64), d_tiles, d_cams, B, d_cnn_in, stream);
}
extern "C" int ht_cnn_input_sized_dev(ht_ctx *ctx, int side, const uint16_t *d_tiles, const float *d_cams, int B, float *d_cnn_in, void *stream)
{
	CHECK_READY(ctx);
	const ht_net *net = ht_net_of(ctx, side);
	return cnn_input_dev(ctx, ht_form_name(ctx, net, "ht_cnn_input_dev", "ht_cnn_input_sized_dev"), net, d_tiles, d_cams, B, d_cnn_in, stream);
}
