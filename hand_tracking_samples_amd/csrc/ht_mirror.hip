// ht_mirror.hip -- left hands: the mirror M (x -> -x of the camera's space) of depth frames, cameras and poses (an addition).
//
// The model, the nets and every tracker kernel are a right hand's.  A left hand seen by a camera is the mirror image of a right hand seen by the mirrored camera, so
// a slot's state stays the right hand's and only the boundary mirrors: frames, cameras and start poses on the way in, poses on the way out (ht_update_hands_*,
// ht_solver_api.hip).  The whole semantics, all sign flips and one subtraction:
//   frame   [h][w] u16   F'[y][x] = F[y][w-1-x]
//   camera  12 floats    focal, cy, depth_scale unchanged; cx' = (float)(w-1) - cx (DCamera::deprojectz's whole-pixel convention, misc_image.h:48); its pose as a pose
//   pose    7 floats     (px,py,pz, qx,qy,qz,qw) -> (-px,py,pz, qx,-qy,-qz,qw): the pose of a bone whose geometry is x-negated in its own frame
// A sign flip is the sign BIT's (-0.0 and NaNs follow it); everything else is moved as bits.  Frames whose flag is 0 are copied.
//
// Mapping.  All three are byte movers.
//   k_mirror_frames<N>  one thread moves N dwords = 2N pixels: one load (global_load_dwordx4 / x2 / dword), the pixels reversed in registers (the dwords in reverse
//                    order, each rotated by 16 bits), one store of the same width at the mirrored place of the same row.  Lane i reads base + 16 i and writes
//                    rowend - 16 i: both sides of a wave's access are whole contiguous lines, no LDS.  Thread r of blockIdx.x owns vector r of every frame
//                    blockIdx.y, blockIdx.y + gridDim.y, ...: its row position is worked out once.  The width follows what the call's sizes and pointers allow
//                    (ht_frame_vec_pixels, ht_frame_vec.hpp): 16 bytes for w % 8 == 0 and 16-byte aligned buffers, 8 for w % 4 == 0 and 8-byte alignment (rows are 8-byte
//                    multiples wherever the update takes a frame), 4, and a pixel-per-thread form (k_mirror_frames<0>) for a buffer aligned to two bytes only
//                    or an odd width.  No path assumes more alignment than was checked.
//   k_mirror_cams /  one thread per float, in place or not (every element is read and written by the same thread).
//   k_mirror_poses
#include <string.h>
#include "ht_host.hpp"
#include "ht_frame_vec.hpp"
#include "ht_mirror.hpp"

#define MR_THREADS 256

__device__ __forceinline__ bool mr_left(const unsigned char *hands, unsigned f) { return !hands || hands[f] != 0; }

template <int N> __global__ __launch_bounds__(MR_THREADS) void k_mirror_frames(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, unsigned per_row, unsigned per_frame, unsigned B,
                                                                               const unsigned char *__restrict__ hands)
{
	const unsigned r = blockIdx.x * MR_THREADS + threadIdx.x;
	if (r >= per_frame) return;
	const unsigned xv = r % per_row, rm = r - xv + (per_row - 1u - xv);      // the same row, counted from its other end
	const ht_dwords<N> *src = (const ht_dwords<N> *)in; ht_dwords<N> *dst = (ht_dwords<N> *)out;
	for (unsigned f = blockIdx.y; f < B; f += gridDim.y)
	{
		const bool left = mr_left(hands, f);
		const size_t base = (size_t)f * per_frame;
		const ht_dwords<N> a = src[base + r];
		ht_dwords<N> m, o;
		ht_reverse(a, m);
#pragma unroll
		for (int i = 0; i < N; i++) o.v[i] = left ? m.v[i] : a.v[i];
		dst[base + (left ? rm : r)] = o;
	}
}
// a pixel per thread: buffers aligned to two bytes only, odd widths
template <> __global__ __launch_bounds__(MR_THREADS) void k_mirror_frames<0>(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, unsigned per_row, unsigned per_frame, unsigned B,
                                                                             const unsigned char *__restrict__ hands)
{
	const unsigned r = blockIdx.x * MR_THREADS + threadIdx.x;
	if (r >= per_frame) return;
	const unsigned xv = r % per_row, rm = r - xv + (per_row - 1u - xv);
	for (unsigned f = blockIdx.y; f < B; f += gridDim.y)
	{
		const size_t base = (size_t)f * per_frame;
		out[base + (mr_left(hands, f) ? rm : r)] = in[base + r];
	}
}

// cameras [B][12]: principal x at 2, the pose at 5..11 (position 5 6 7, quaternion xyzw 8 9 10 11)
__global__ __launch_bounds__(MR_THREADS) void k_mirror_cams(const unsigned *in, unsigned *out, float wm1, unsigned n, const unsigned char *__restrict__ hands)
{
	const unsigned i = blockIdx.x * MR_THREADS + threadIdx.x;
	if (i >= n) return;
	const unsigned f = i / HT_CAM, k = i - f * HT_CAM;
	unsigned v = in[i];
	if (mr_left(hands, f)) v = ht_mirror_cam_word(v, k, wm1);
	out[i] = v;
}
// poses [B][per_frame][7]: px, qy, qz change sign
__global__ __launch_bounds__(MR_THREADS) void k_mirror_poses(const unsigned *in, unsigned *out, unsigned per_frame7, unsigned n, const unsigned char *__restrict__ hands)
{
	const unsigned i = blockIdx.x * MR_THREADS + threadIdx.x;
	if (i >= n) return;
	const unsigned k = i % HT_POSE;
	unsigned v = in[i];
	if ((k == 0 || k == 4 || k == 5) && mr_left(hands, hands ? i / per_frame7 : 0u)) v ^= 0x80000000u;
	out[i] = v;
}

// ---- launch layer ----------------------------------------------------------------------------------------------------------------------------------------------
void ht_launch_mirror_frames(const uint16_t *in, int w, int h, int B, const unsigned char *hands, uint16_t *out, hipStream_t s)
{
	ht_frame_vec_dispatch(ht_frame_vec_pixels((uintptr_t)in | (uintptr_t)out, w), [&](auto px)
	{
		const ht_frame_grid g(w, h, B, px, MR_THREADS);
		hipLaunchKernelGGL(k_mirror_frames<px / 2>, g.grid, dim3(MR_THREADS), 0, s, in, out, g.per_row, g.per_frame, (unsigned)B, hands);
	});
}
void ht_launch_mirror_cams(const float *in, int w, int B, const unsigned char *hands, float *out, hipStream_t s)
{
	const unsigned n = (unsigned)B * HT_CAM;
	hipLaunchKernelGGL(k_mirror_cams, dim3((n + MR_THREADS - 1) / MR_THREADS), dim3(MR_THREADS), 0, s, (const unsigned *)in, (unsigned *)out, (float)(w - 1), n, hands);
}
void ht_launch_mirror_poses(const float *in, int per_frame, int B, const unsigned char *hands, float *out, hipStream_t s)
{
	const unsigned n = (unsigned)B * (unsigned)per_frame * HT_POSE;
	hipLaunchKernelGGL(k_mirror_poses, dim3((n + MR_THREADS - 1) / MR_THREADS), dim3(MR_THREADS), 0, s, (const unsigned *)in, (unsigned *)out, (unsigned)per_frame * HT_POSE, n, hands);
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------------------------
// Every check runs before anything grows or launches.  B is not bounded by max_batch: no tracker slot is used.
static int mr_check_frames(ht_ctx *ctx, const void *in, const void *out, int w, int h, int B)
{
	if (!in || !out || B < 0) { ctx->err = "ht_mirror_frames: bad argument"; return HT_ERR_ARG; }
	if (!ht_frame_dims_ok(w, h)) { ctx->err = "ht_mirror_frames: w and h between 1 and 4096"; return HT_ERR_ARG; }
	const size_t bytes = (size_t)B * w * h * sizeof(uint16_t);
	if (ht_ranges_overlap(in, bytes, out, bytes)) { ctx->err = "ht_mirror_frames: the frames are not mirrored in place: depth and depth_out must not overlap"; return HT_ERR_ARG; }
	return HT_OK;
}
static int mr_check_floats(ht_ctx *ctx, const char *fn, const void *in, const void *out, long long B, long long per)
{
	if (!in || !out || B < 0 || per < 1) { ctx->err = std::string(fn) + ": bad argument"; return HT_ERR_ARG; }
	if (B * per > 0x7fffffffLL) { ctx->err = std::string(fn) + ": more than 2^31 floats in one call"; return HT_ERR_ARG; }
	return HT_OK;
}
extern "C" int ht_mirror_frames_dev(ht_ctx *ctx, const uint16_t *d_depth, int w, int h, int B, const unsigned char *d_hands, uint16_t *d_depth_out, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = mr_check_frames(ctx, d_depth, d_depth_out, w, h, B); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	{ ht_prof_scope ps(ctx, "k_mirror_frames", s); ht_launch_mirror_frames(d_depth, w, h, B, d_hands, d_depth_out, s); }
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_mirror_cams_dev(ht_ctx *ctx, const float *d_cams, int w, int B, const unsigned char *d_hands, float *d_cams_out, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = mr_check_floats(ctx, "ht_mirror_cams", d_cams, d_cams_out, B, HT_CAM); if (r) return r; }
	if (!ht_frame_dims_ok(w, 1)) { ctx->err = "ht_mirror_cams: w between 1 and 4096"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	{ ht_prof_scope ps(ctx, "k_mirror_cams", s); ht_launch_mirror_cams(d_cams, w, B, d_hands, d_cams_out, s); }
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_mirror_poses_dev(ht_ctx *ctx, const float *d_poses, int per_frame, int B, const unsigned char *d_hands, float *d_poses_out, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = mr_check_floats(ctx, "ht_mirror_poses", d_poses, d_poses_out, B, (long long)per_frame * HT_POSE); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	{ ht_prof_scope ps(ctx, "k_mirror_poses", s); ht_launch_mirror_poses(d_poses, per_frame, B, d_hands, d_poses_out, s); }
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
// The host forms: input, flags and output through the context's staging (ht_staged_call), the same kernels.  The staging's segments are 256-byte aligned, so
// these always take the widest path the width allows.
extern "C" int ht_mirror_frames(ht_ctx *ctx, const uint16_t *depth, int w, int h, int B, const unsigned char *hands, uint16_t *depth_out)
{
	CHECK_READY(ctx);
	{ const int r = mr_check_frames(ctx, depth, depth_out, w, h, B); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t bytes = (size_t)B * w * h * sizeof(uint16_t);
	ht_seg seg[3] = { { (void *)depth, bytes, false }, { (void *)hands, (size_t)B, false }, { depth_out, bytes, true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return ht_mirror_frames_dev(ctx, (const uint16_t *)seg[0].dev, w, h, B, (const unsigned char *)seg[1].dev, (uint16_t *)seg[2].dev, s); });
}
extern "C" int ht_mirror_cams(ht_ctx *ctx, const float *cams, int w, int B, const unsigned char *hands, float *cams_out)
{
	CHECK_READY(ctx);
	{ const int r = mr_check_floats(ctx, "ht_mirror_cams", cams, cams_out, B, HT_CAM); if (r) return r; }
	if (!ht_frame_dims_ok(w, 1)) { ctx->err = "ht_mirror_cams: w between 1 and 4096"; return HT_ERR_ARG; }
	if (B == 0) return HT_OK;
	const size_t bytes = (size_t)B * HT_CAM * sizeof(float);
	ht_seg seg[3] = { { (void *)cams, bytes, false }, { (void *)hands, (size_t)B, false }, { cams_out, bytes, true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return ht_mirror_cams_dev(ctx, (const float *)seg[0].dev, w, B, (const unsigned char *)seg[1].dev, (float *)seg[2].dev, s); });
}
extern "C" int ht_mirror_poses(ht_ctx *ctx, const float *poses, int per_frame, int B, const unsigned char *hands, float *poses_out)
{
	CHECK_READY(ctx);
	{ const int r = mr_check_floats(ctx, "ht_mirror_poses", poses, poses_out, B, (long long)per_frame * HT_POSE); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t bytes = (size_t)B * per_frame * HT_POSE * sizeof(float);
	ht_seg seg[3] = { { (void *)poses, bytes, false }, { (void *)hands, (size_t)B, false }, { poses_out, bytes, true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return ht_mirror_poses_dev(ctx, (const float *)seg[0].dev, per_frame, B, (const unsigned char *)seg[1].dev, (float *)seg[2].dev, s); });
}
