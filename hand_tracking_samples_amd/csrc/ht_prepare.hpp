// ht_prepare.hpp -- what the kernels that turn depth words into points make of one, each stated once: k_prepare, k_prepare_frame, k_cnn_input (ht_cnn.hip) and
// k_fuse_views (ht_views.hip), and k_fuse_views' walk of a frame, which k_calib_cloud (ht_calib.hip) takes too.  Device code; include after ht_device.hpp.
#pragma once
#include "ht_device.hpp"

__device__ __forceinline__ float depth_metres(unsigned px, float dscale) { return (float)(int)px * dscale; }
__device__ __forceinline__ float cnn_input_value(float d, float drangey) { return clamp_std(1.0f - (d - 0.1f) / (drangey - 0.1f), 0.0f, 1.0f); }      // handtrack.h:700
__device__ __forceinline__ bool depth_in_range(float d, float lo, float hi) { return d >= lo && d < hi; }                                              // FallsWithinRange misc_image.h:24
__device__ __forceinline__ bool depth_in_range(float d, float drangey) { return depth_in_range(d, 0.1f, drangey); }                                       // the tracker's range {0.1, drangey} (handtrack.h:703)
__device__ __forceinline__ float4 deproject_point(float x, float y, float d, float fx, float fy, float cx, float cy) { return make_float4(((x - cx) / fx) * d, ((y - cy) / fy) * d, 1.0f * d, 0.0f); }      // deprojectz misc_image.h:48
// exclusive prefix of cnt over the block's 256 threads (every thread calls it): the thread's base; total: the block's sum
__device__ __forceinline__ int block_prefix256(int cnt, int lane, int wave, int &total)
{
	int incl = cnt;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) { int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
	__shared__ int wsum[4];
	if (lane == 63) wsum[wave] = incl;
	__syncthreads();
	int base = incl - cnt;
	for (int i = 0; i < wave; i++) base += wsum[i];
	total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
	return base;
}

// ---- a view's frame as a cloud: k_fuse_views' walk (ht_views.hip), shared with k_calib_cloud (ht_calib.hip) -----------------------------------------------------------
#define FV_THREADS 256
// a view: its intrinsics, its pose in tracking space (posed: not exactly identity), its mirror plane (mirror: it has one; bad: a plane that is neither "none" nor usable)
struct fv_view { float fx, fy, cx, cy, dscale; v3 pos; v4 q; v4 plane; bool posed, mirror, bad; };
// fv_side: what becomes of in-range pixel i with depth d: 0 dropped (coplanar), 1 direct, 2 mirrored; p: the point in the view's camera space, pd: its plane distance.
// MIRROR is the view's, so a view without a plane pays for none
template <bool MIRROR> __device__ __forceinline__ int fv_side(const fv_view &c, float eps, int i, int w, float d, float4 &p, float &pd)
{
	p = deproject_point((float)(i % w), (float)(i / w), d, c.fx, c.fy, c.cx, c.cy);
	if (!MIRROR) return 1;
	pd = dot_plane(c.plane, V3(p.x, p.y, p.z));                    // dot(float4(p, 1), plane), PlaneSplit misc_image.h:468
	return pd <= -eps ? 2 : pd > eps ? 1 : 0;                      // under (virtual) | over (direct) | coplanar
}
// The block's own view, one walk: tile by tile the kept pixels are ranked (the tiles before + the block's prefix + the thread's own) and every fraction-th goes to
// out[base + rank / fraction] while that is below cap.  Returns the view's kept pixels; nd / nm: the direct and mirrored points this thread wrote
#define FV_PER 4
template <bool MIRROR> __device__ __forceinline__ int fv_emit(const fv_view &c, const uint16_t *__restrict__ src, int npx, int w, float lo, float hi, float eps, int fraction, int base, int cap, int v,
                                                               float4 *__restrict__ out, int &nd, int &nm)
{
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	int before = 0;
	for (int tile = 0; tile < npx; tile += FV_THREADS * FV_PER)
	{
		const int i0 = tile + FV_PER * t;
		float d[FV_PER], pd[FV_PER]; float4 p[FV_PER]; int k[FV_PER];
		int cnt = 0;
#pragma unroll
		for (int j = 0; j < FV_PER; j++)
		{
			k[j] = 0; pd[j] = 0.0f;
			d[j] = i0 + j < npx ? depth_metres(src[i0 + j], c.dscale) : -1.0f;      // (no range holds a negative depth: range_lo >= 0)
			if (depth_in_range(d[j], lo, hi)) k[j] = fv_side<MIRROR>(c, eps, i0 + j, w, d[j], p[j], pd[j]);
			cnt += k[j] != 0 ? 1 : 0;
		}
		int total;
		int rank = before + block_prefix256(cnt, lane, wave, total);
#pragma unroll
		for (int j = 0; j < FV_PER; j++) if (k[j])
		{
			const int idx = base + rank / fraction;
			if (rank % fraction == 0 && idx < cap)
			{
				v3 q = V3(p[j].x, p[j].y, p[j].z);
				if (k[j] == 2) q = q + xyz(c.plane) * (pd[j] * -2.0f);      // Mirror misc_image.h:477
				if (c.posed) q = c.pos + qrot(c.q, q);
				out[idx] = make_float4(q.x, q.y, q.z, (float)(2 * v + (k[j] - 1)));
				nd += k[j] == 1 ? 1 : 0; nm += k[j] == 2 ? 1 : 0;
			}
			rank++;
		}
		before += total;
		__syncthreads();      // the prefix's wave sums are free for the next tile
	}
	return before;
}
