// ht_sensor.hip -- the camera front end on the device: the depth filters RSCam::GetDepth runs before a frame reaches the tracker, for a batch of raw frames.
//
// Reference computations (all integer arithmetic, the constants are the reference's own; it assumes millimetre counts, dcam.h:180):
//   RSCam::FilterIvy               include/dcam.h:209-226 (SR300 / F200: DownSampleFst until at most image_width_max_allowed wide, then 0 -> 4 m)
//   RSCam::FilterDS4               include/dcam.h:174-208 (R200: dark-IR and near pixels -> 4096, the flying-pixel pass in raster order, the background model)
//   RSCam::addbackground           include/dcam.h:157-162
//   DownSampleFst, DCamera / int   include/misc_image.h:81-94,136 and :62 (the first pixel of every 2x2; focal and principal halved, depth_scale and pose kept)
//
// FilterDS4's second pass rewrites the frame in place while it walks it: pixel i reads p[i-1], p[i-2], p[i-w], p[i-2w] as ALREADY rewritten and p[i+1], p[i+2],
// p[i+w], p[i+2w] as the first pass left them, so a pixel's fate depends on the fates of earlier pixels without bound (tests/test_sensor_ref.py has frames on
// which one dark pixel at x = 2 decides the last pixel of its row).  The decomposition here is exact:
//   rows      go top to bottom.  For row y the vertical verdict V(x) = has(w) && has(2w) reads rows y-1, y-2 as finished and rows y+1, y+2 as pass 1 left them:
//             one bit per pixel, known before the row starts.
//   a row     kill(x) is a function of the state s = (kill(x-1), kill(x-2)) and of values known up front: has(1) = near(right) || (kill(x-1) ? near(4096) :
//             near(left)), has(2) likewise.  So pixel x is a transition of a 4-state automaton, s -> (kill(x), kill(x-1)): four 2-bit entries, one byte; the two
//             border pixels at either end of a row are the transition (k1, k2) -> (0, k1).  Transitions compose associatively, so a prefix scan over the row
//             gives every pixel's state: every lane composes its own consecutive pixels, one shuffle scan over the wave's 64 lane totals gives the state each
//             lane starts from (the row starts in state 0), and the lane walks its pixels once more from that state.  No iteration to a fixed point.
//   mapping   one wave per frame (one block of 64 lanes), lane l owning the pixels [l * P, l * P + P) of a row, P = ceil(w / 64): the carry across a lane's own
//             pixels is the sequential composition, the carry across lanes is the scan, and no carry crosses a wave.  LDS: a rolling window of five rows of
//             u16 (rows y-2 .. y+2) and one row of transition bytes, 11 bytes per pixel of width (3.5 KB at 320).
// Pass 1, pass 3 (the background model), the halving and FilterIvy are pointwise.
//
// ht_sensor_simulate, the way back -- rendered frames made raw -- is an addition with no reference code; it has the second half of this file.
#include <limits.h>
#include <string.h>
#include "ht_device.hpp"
#include "ht_host.hpp"
#include "ht_frame_vec.hpp"
#include "ht_mix.hpp"

#define SN_DARK 4096            // what a dropped pixel becomes (dcam.h:186,196,203), and what the background model starts at (:159)
#define SN_THREADS 256          // the pointwise kernels

// x86's truncating float -> int conversion, then the low 16 bits: what (unsigned short)(4.0f / depth_scale) (dcam.h:216) compiles to on the reference's
// platform.  NaN and out-of-range quotients give INT_MIN there, whose low 16 bits are 0 (ht_labels.hip: lb_trunc).
__device__ __forceinline__ unsigned short sn_fill(float depth_scale)
{
	const float q = 4.0f / depth_scale;
	const int v = (q >= -2147483648.0f && q < 2147483648.0f) ? (int)q : INT_MIN;
	return (unsigned short)((unsigned)v & 0xFFFFu);
}

// cams_out = cams / 2, k times (misc_image.h:62): focal and principal halved, depth_scale and pose kept
__global__ __launch_bounds__(SN_THREADS) void k_sensor_cams(const float *__restrict__ cams, int n, int k, float *__restrict__ cams_out)
{
	const int i = blockIdx.x * SN_THREADS + threadIdx.x;
	if (i >= n) return;
	float v = cams[i];
	if (i % HT_CAM < 4) for (int j = 0; j < k; j++) v = v / 2.0f;
	cams_out[i] = v;
}

// FilterIvy: output pixel (x, y) is input pixel (x << k, y << k) (DownSampleFst k times keeps the first of every 2^k x 2^k), then 0 -> the 4 m background
__global__ __launch_bounds__(SN_THREADS) void k_sensor_ivy(const uint16_t *__restrict__ depth, const float *__restrict__ cams, int w, int wo, int ho, int k, size_t total,
                                                           uint16_t *__restrict__ out)
{
	const size_t per = (size_t)wo * ho;
	for (size_t i = (size_t)blockIdx.x * SN_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * SN_THREADS)
	{
		const size_t f = i / per; const int r = (int)(i - f * per);
		const int y = r / wo, x = r - y * wo;
		unsigned short d = depth[f * ((size_t)w * ((size_t)ho << k)) + (size_t)(y << k) * w + (x << k)];
		if (d == 0) d = sn_fill(cams[f * HT_CAM + 4]);
		out[i] = d;
	}
}

// addbackground: background[i] = min(background[i], (unsigned short)(dp[i] - fudge)), the subtraction in int, the cast wrapping; init: the old model is 4096
__global__ __launch_bounds__(SN_THREADS) void k_sensor_background(const uint16_t *__restrict__ depth, size_t total, int fudge, int init, uint16_t *__restrict__ background)
{
	for (size_t i = (size_t)blockIdx.x * SN_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * SN_THREADS)
	{
		const unsigned short old = init ? (unsigned short)SN_DARK : background[i];
		const unsigned short v = (unsigned short)((unsigned)((int)depth[i] - fudge) & 0xFFFFu);
		background[i] = v < old ? v : old;
	}
}

// ---- FilterDS4 ----
// A transition is a byte: bits 2s, 2s+1 hold the state that state s goes to; a state is kill(x-1) | kill(x-2) << 1.
#define SN_IDENT 0xE4u          // s -> s
#define SN_BORDER 0x88u         // (k1, k2) -> (0, k1): a pixel the pass skips
__device__ __forceinline__ unsigned sn_compose(unsigned f, unsigned g)      // f first, then g
{
	unsigned r = 0;
#pragma unroll
	for (int s = 0; s < 4; s++) r |= ((g >> (((f >> (2 * s)) & 3u) * 2)) & 3u) << (2 * s);
	return r;
}
__device__ __forceinline__ bool sn_near(int a, int b) { const int d = a - b; return (d < 0 ? -d : d) < 10; }      // hasneighbor's test, dcam.h:181

__global__ __launch_bounds__(64) void k_sensor_ds4(const uint16_t *__restrict__ depth, const uint8_t *__restrict__ ir, const uint16_t *__restrict__ background, int w, int h,
                                                   uint16_t *__restrict__ out)
{
	extern __shared__ uint16_t sn_lds[];
	const int lane = threadIdx.x;
	const int wp = (w + 1) & ~1;
	uint16_t *ring = sn_lds;                              // [5][wp]: row r lives in slot r % 5
	uint8_t *tr = (uint8_t *)(sn_lds + 5 * wp);           // [w]: the row's transitions
	const size_t f0 = (size_t)blockIdx.x * w * h;
	const uint16_t *D = depth + f0; const uint8_t *I = ir + f0; const uint16_t *G = background ? background + f0 : nullptr; uint16_t *O = out + f0;
	const int P = (w + 63) >> 6, x0 = lane * P, x1 = min(w, x0 + P);
	// pass 1 on the way in (dcam.h:182-188)
	auto load_row = [&](int r)
	{
		uint16_t *dst = ring + (r % 5) * wp;
		for (int x = lane; x < w; x += 64) { const unsigned short d = D[r * w + x]; dst[x] = (d < 30 || I[r * w + x] < 8) ? (unsigned short)SN_DARK : d; }
	};
	load_row(0);
	if (h > 1) load_row(1);
	for (int y = 0; y < h; y++)
	{
		if (y + 2 < h) load_row(y + 2);      // into the slot of row y - 3
		__syncthreads();
		uint16_t *c = ring + (y % 5) * wp;
		if (y >= 2 && y < h - 2)             // pass 2 (dcam.h:189-198) on row y
		{
			const uint16_t *u1 = ring + ((y - 1) % 5) * wp, *u2 = ring + ((y - 2) % 5) * wp, *d1 = ring + ((y + 1) % 5) * wp, *d2 = ring + ((y + 2) % 5) * wp;
			unsigned T = SN_IDENT;
			if (x0 < x1)
			{
				int a = c[max(x0 - 2, 0)], b = c[max(x0 - 1, 0)], m = c[x0], r1 = c[min(x0 + 1, w - 1)];      // p[x-2], p[x-1], p[x], p[x+1] as pass 1 left them
				for (int x = x0; x < x1; x++)
				{
					const int r2 = c[min(x + 2, w - 1)];
					unsigned t = SN_BORDER;
					if (x >= 2 && x < w - 2)
					{
						const bool V = (sn_near(u1[x], m) || sn_near(d1[x], m)) && (sn_near(u2[x], m) || sn_near(d2[x], m));
						const bool nr1 = sn_near(r1, m), nr2 = sn_near(r2, m), n4 = sn_near(SN_DARK, m);
						const bool h10 = nr1 || sn_near(b, m), h11 = nr1 || n4, h20 = nr2 || sn_near(a, m), h21 = nr2 || n4;      // has(1), has(2) with the left pixel kept / killed
						t |= (unsigned)!(V && h10 && h20) | (unsigned)!(V && h11 && h20) << 2 | (unsigned)!(V && h10 && h21) << 4 | (unsigned)!(V && h11 && h21) << 6;
					}
					tr[x] = (uint8_t)t;
					T = sn_compose(T, t);
					a = b; b = m; m = r1; r1 = r2;
				}
			}
			// inclusive scan of the lane totals; the row starts in state 0, so lane l starts in what the lanes before it make of state 0
			unsigned v = T;
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) { const unsigned o = __shfl_up(v, d); if (lane >= d) v = sn_compose(o, v); }
			const unsigned e = __shfl_up(v, 1);
			unsigned s = lane ? (e & 3u) : 0u;
			__syncthreads();                 // every lane has read row y as pass 1 left it
			for (int x = x0; x < x1; x++) { s = ((unsigned)tr[x] >> (2 * s)) & 3u; if (s & 1u) c[x] = (unsigned short)SN_DARK; }
			__syncthreads();
		}
		// pass 3 (dcam.h:199-204) on the way out
		for (int x = lane; x < w; x += 64) { unsigned short v = c[x]; if (G && v > G[y * w + x]) v = (unsigned short)SN_DARK; O[y * w + x] = v; }
	}
}

// ---- host ----

// k halvings until w >> k <= max_width, and every refusal that needs no context
static int sn_dims(int kind, int w, int h, int max_width, int *k_out, int *w_out, int *h_out)
{
	if ((kind != HT_SENSOR_IVY && kind != HT_SENSOR_DS4) || !ht_frame_dims_ok(w, h) || max_width < 1) return HT_ERR_ARG;
	int k = 0;
	while ((w >> k) > max_width) k++;
	if (kind == HT_SENSOR_DS4 && k > 0) return HT_ERR_ARG;      // the reference indexes the full-size frame with an IR image it has already halved (dcam.h:170-171,184)
	if ((w & ((1 << k) - 1)) || (h & ((1 << k) - 1))) return HT_ERR_ARG;      // DownSample reads past the image there (misc_image.h:87-88)
	if (k_out) *k_out = k;
	if (w_out) *w_out = w >> k;
	if (h_out) *h_out = h >> k;
	return HT_OK;
}
extern "C" int ht_sensor_out_dims(int kind, int w, int h, int max_width, int *w_out, int *h_out)
{
	if (!w_out || !h_out) return HT_ERR_ARG;
	return sn_dims(kind, w, h, max_width, nullptr, w_out, h_out);
}

// the checks both forms of the filter share, all made before anything is launched or grown
static int sn_check_filter(ht_ctx *ctx, int kind, const void *depth, const void *ir, const void *cams, int w, int h, int B, int max_width, const void *background,
                           const void *depth_out, const void *cams_out, int *k, int *wo, int *ho)
{
	const char *bad = nullptr;
	if (sn_dims(kind, w, h, max_width, k, wo, ho)) bad = kind == HT_SENSOR_DS4 && w > max_width && max_width >= 1 ? "a DS4 frame wider than max_width" : "kind, frame size or max_width";
	else if (B < 0) bad = "B";
	else if (!depth || !cams || !depth_out || !cams_out) bad = "a NULL buffer";
	else if (kind == HT_SENSOR_DS4 && !ir) bad = "DS4 needs the IR image";
	else if (kind == HT_SENSOR_IVY && background) bad = "FilterIvy has no background model";
	else if (ht_ranges_overlap(depth, (size_t)B * w * h * sizeof(uint16_t), depth_out, (size_t)B * *wo * *ho * sizeof(uint16_t))) bad = "depth_out aliases depth";
	if (bad) { ctx->err = std::string("ht_sensor_filter: bad argument (") + bad + ")"; return HT_ERR_ARG; }
	return HT_OK;
}

static inline unsigned sn_grid(size_t total) { const size_t b = (total + SN_THREADS - 1) / SN_THREADS; return (unsigned)(b < (1u << 20) ? b : (1u << 20)); }

extern "C" int ht_sensor_filter_dev(ht_ctx *ctx, int kind, const uint16_t *d_depth, const uint8_t *d_ir, const float *d_cams, int w, int h, int B, int max_width,
                                    const uint16_t *d_background, uint16_t *d_depth_out, float *d_cams_out, void *stream)
{
	CHECK_READY(ctx);
	int k, wo, ho;
	{ const int r = sn_check_filter(ctx, kind, d_depth, d_ir, d_cams, w, h, B, max_width, d_background, d_depth_out, d_cams_out, &k, &wo, &ho); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const int ncam = B * HT_CAM;
	hipLaunchKernelGGL(k_sensor_cams, dim3((ncam + SN_THREADS - 1) / SN_THREADS), dim3(SN_THREADS), 0, s, d_cams, ncam, k, d_cams_out);
	if (kind == HT_SENSOR_IVY)
	{
		const size_t total = (size_t)B * wo * ho;
		hipLaunchKernelGGL(k_sensor_ivy, dim3(sn_grid(total)), dim3(SN_THREADS), 0, s, d_depth, d_cams, w, wo, ho, k, total, d_depth_out);
	}
	else
	{
		const int wp = (w + 1) & ~1;
		const size_t lds = (size_t)5 * wp * sizeof(uint16_t) + (size_t)w;      // 44 KB at the widest frame
		hipLaunchKernelGGL(k_sensor_ds4, dim3(B), dim3(64), lds, s, d_depth, d_ir, d_background, w, h, d_depth_out);
	}
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

extern "C" int ht_sensor_filter(ht_ctx *ctx, int kind, const uint16_t *depth, const uint8_t *ir, const float *cams, int w, int h, int B, int max_width,
                                const uint16_t *background, uint16_t *depth_out, float *cams_out)
{
	CHECK_READY(ctx);
	int k, wo, ho;
	{ const int r = sn_check_filter(ctx, kind, depth, ir, cams, w, h, B, max_width, background, depth_out, cams_out, &k, &wo, &ho); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t n = (size_t)B, npx = n * w * h;      // staged through the context's buffer (no tracker slot: B is not bounded by max_batch)
	ht_seg seg[6] = { { (void *)depth, npx * sizeof(uint16_t), false }, { kind == HT_SENSOR_DS4 ? (void *)ir : nullptr, npx, false }, { (void *)cams, n * HT_CAM * sizeof(float), false },
	                  { (void *)background, npx * sizeof(uint16_t), false }, { depth_out, n * wo * ho * sizeof(uint16_t), true }, { cams_out, n * HT_CAM * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 6, [&](hipStream_t s)
	                      { return ht_sensor_filter_dev(ctx, kind, (const uint16_t *)seg[0].dev, (const uint8_t *)seg[1].dev, (const float *)seg[2].dev, w, h, B, max_width,
	                                                    (const uint16_t *)seg[3].dev, (uint16_t *)seg[4].dev, (float *)seg[5].dev, s); });
}

static int sn_check_background(ht_ctx *ctx, const void *depth, int w, int h, int B, const void *background)
{
	if (!depth || !background || !ht_frame_dims_ok(w, h) || B < 0 || ht_ranges_overlap(depth, (size_t)B * w * h * sizeof(uint16_t), background, (size_t)B * w * h * sizeof(uint16_t)))
	{ ctx->err = "ht_sensor_background: bad argument"; return HT_ERR_ARG; }
	return HT_OK;
}
extern "C" int ht_sensor_background_dev(ht_ctx *ctx, const uint16_t *d_depth, int w, int h, int B, int fudge, int init, uint16_t *d_background, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = sn_check_background(ctx, d_depth, w, h, B, d_background); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	const size_t total = (size_t)B * w * h;
	hipLaunchKernelGGL(k_sensor_background, dim3(sn_grid(total)), dim3(SN_THREADS), 0, s, d_depth, total, fudge, init, d_background);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_sensor_background(ht_ctx *ctx, const uint16_t *depth, int w, int h, int B, int fudge, int init, uint16_t *background)
{
	CHECK_READY(ctx);
	{ const int r = sn_check_background(ctx, depth, w, h, B, background); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t bytes = (size_t)B * w * h * sizeof(uint16_t);
	ht_seg seg[2] = { { (void *)depth, bytes, false }, { background, bytes, true } };      // the model goes both ways: up here unless it starts afresh, down with the outputs
	return ht_staged_call(ctx, seg, 2, [&](hipStream_t s)
	                      {
		                      if (!init) HIPCHK(ctx, hipMemcpyAsync(seg[1].dev, background, bytes, hipMemcpyHostToDevice, s));
		                      return ht_sensor_background_dev(ctx, (const uint16_t *)seg[0].dev, w, h, B, fudge, init, (uint16_t *)seg[1].dev, s);
	                      });
}

// ---- ht_sensor_simulate: raw camera frames from rendered depth (an addition; the definition is include/ht_mi355x.h's) -------------------------
// A 3x3 stencil over u16 frames plus one 64-bit mix per pixel (two with an IR image).
//   mapping   one thread makes N consecutive pixels of a row: it loads its own N pixels of rows y-1, y, y+1 as one vector each (global_load_dwordx4 at N = 8)
//             and the single pixels left and right of them, six u16 loads.  Lane i reads base + 16 i of three rows, whole contiguous lines; rows y-1 and y+1 are
//             the rows the threads of the neighbouring rows load as their own, so every line comes from memory once and from the cache twice more.  No LDS: a
//             tile with its halo would carry the same lines through one more copy, and the stage's time is its arithmetic, not its loads.
//             N follows what the width and the pointers allow, by the one width rule (ht_frame_vec_pixels): 8 pixels (16 bytes) for w % 8 == 0 and 16-byte aligned frames (the IR
//             image, whose store is N bytes, 8-byte aligned), 4, 2, and a pixel per thread for an odd width or buffers aligned to their element only.
//   frames    thread r of blockIdx.x owns vector r of every frame blockIdx.y, blockIdx.y + gridDim.y, ...: its place in the frame is worked out once.  The frame's
//             key is wave-uniform (scalar unit); the pixel's mix is the only 64-bit multiply chain in the lane.
//   noise set by value in the kernel's arguments (80 bytes, scalar registers).

#define SS_THREADS 256
template <int N> struct alignas(N) ss_ir { uint8_t v[N]; };

HT_HD bool ss_fg(int q, int far_count) { return (unsigned)(q - 1) < (unsigned)(far_count - 1); }      // q != 0 && q < far_count; -1 (outside the image) is not
HT_HD int ss_abs(int a) { return a < 0 ? -a : a; }
HT_HD int ss_noise(const ht_sensor_noise &nz, int d, int g)
{
	const int s = nz.sigma0_256 + (int)(((unsigned long long)(unsigned)nz.sigma2 * ((unsigned)d * (unsigned)d)) >> 20);      // d <= 65535, sigma2 <= 4096: the shift leaves at most 2^24
	const int n = s * g + 4736;                    // |s * g| < 2^31 - 4736 for every set the call accepts
	int q = n / 9472; if (n - q * 9472 < 0) q--;      // floor
	const int r = d + q;
	return r < 1 ? 1 : r > 65535 ? 65535 : r;
}
// p and its 8 neighbours in raster order (-1: outside the image) -> the output depth and, with want_ir, the IR value
HT_HD void ss_pixel(const ht_sensor_noise &nz, int kind, unsigned long long key, unsigned i, bool want_ir, int p, const int (&nb)[8], uint16_t &dout, uint8_t &iout)
{
	const bool fg = ss_fg(p, nz.far_count), wall = kind == HT_SENSOR_DS4 && nz.wall_count > 0;
	unsigned long long H = 0;
	if (fg || wall || want_ir) H = ht_mix64(key ^ ((unsigned long long)(i + 1u) * 0xD6E8FEB86659FD93ull));
	const int g = (int)((H >> 40) & 63u) + (int)((H >> 46) & 63u) + (int)((H >> 52) & 63u) + (int)(H >> 58) - 126;
	int d1 = 0;
	if (fg)
	{
		int best = -1, far = 0;
#pragma unroll
		for (int k = 0; k < 8; k++)
		{
			const int q = nb[k];
			const int v = ss_fg(q, nz.far_count) ? q : nz.fly_bg_count, diff = ss_abs(v - p);
			if (q >= 0 && diff > best) { best = diff; far = v; }      // the first of the largest
		}
		const int ua = (int)(H & 0xFFFFu), t = (int)((H >> 16) & 0xFFu), ub = (int)((H >> 24) & 0xFFFFu);
		bool drop = ub >= 65536 - nz.p_hole;
		int base = p;
		if (best > nz.edge_step)
		{
			if (ua < nz.p_edge_drop) drop = true;
			else if (ua < nz.p_edge_drop + nz.p_edge_fly) base = p + (((far - p) * t) >> 8);
		}
		else
		{
			const int gx = ss_fg(nb[3], nz.far_count) && ss_fg(nb[4], nz.far_count) ? ss_abs(nb[4] - nb[3]) : 0;
			const int gy = ss_fg(nb[1], nz.far_count) && ss_fg(nb[6], nz.far_count) ? ss_abs(nb[6] - nb[1]) : 0;
			if ((gx > gy ? gx : gy) > nz.slope_step && ub < nz.p_slope_drop) drop = true;
		}
		if (!drop) d1 = ss_noise(nz, base, g);
	}
	else if (wall) d1 = ss_noise(nz, nz.wall_count, g);
	if (kind == HT_SENSOR_DS4 && nz.disparity_k > 0 && d1 != 0)
	{
		const unsigned K2 = 2u * (unsigned)nz.disparity_k, disp = (K2 + (unsigned)d1) / (2u * (unsigned)d1);      // K <= 2^30: 2K + d1 < 2^32
		if (disp == 0) d1 = 0;
		else { const unsigned back = (K2 + disp) / (2u * disp); d1 = (int)(back < 65535u ? back : 65535u); }
	}
	dout = (uint16_t)d1;
	if (want_ir)
	{
		const unsigned long long H2 = ht_mix64(H ^ 0xA0761D6478BD642Full);
		if (d1 != 0)
		{
			const unsigned dd = (unsigned)d1 * (unsigned)d1;
			const int gi = (int)((H2 >> 8) & 63u) + (int)((H2 >> 14) & 63u) - 63;
			const long long v = (long long)nz.ir_floor + (long long)((unsigned)nz.ir_gain / ((dd >> 8) + 1u)) + (long long)((gi * nz.ir_noise) >> 6);
			iout = (uint8_t)(v < 8 ? 8 : v > 255 ? 255 : v);
		}
		else iout = (uint8_t)(H2 & 7u);
	}
}

// vector (x0 .. x0 + N - 1, y) of frame f; host and device, so that a CPU build can walk the same code
template <int N> HT_HD void ss_vector(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, uint8_t *__restrict__ ir, int kind, int w, int h, int y, int x0, unsigned f, const ht_sensor_noise &nz)
{
	const bool lf = x0 > 0, rt = x0 + N < w, have[3] = { y > 0, true, y + 1 < h };
	const size_t frame_px = (size_t)w * h, o = (size_t)y * w + x0;
	const bool want_ir = ir != nullptr;
	const unsigned long long key = ht_mix64(nz.seed ^ ((nz.first_index + f) * 0x9E3779B97F4A7C15ull));
	const uint16_t *F = in + (size_t)f * frame_px + o;
	int a[3][N + 2];
#pragma unroll
	for (int j = 0; j < 3; j++)
	{
		if (have[j])
		{
			const uint16_t *row = F + (ptrdiff_t)(j - 1) * w;      // inside the frame: have[j]
			const ht_pixels<N> v = *(const ht_pixels<N> *)row;
#pragma unroll
			for (int k = 0; k < N; k++) a[j][k + 1] = v.v[k];
			a[j][0] = lf ? (int)row[-1] : -1;
			a[j][N + 1] = rt ? (int)row[N] : -1;
		}
		else
		{
#pragma unroll
			for (int k = 0; k < N + 2; k++) a[j][k] = -1;
		}
	}
	ht_pixels<N> po; ss_ir<N> io;
#pragma unroll
	for (int k = 0; k < N; k++)
	{
		const int nb[8] = { a[0][k], a[0][k + 1], a[0][k + 2], a[1][k], a[1][k + 2], a[2][k], a[2][k + 1], a[2][k + 2] };
		io.v[k] = 0;
		ss_pixel(nz, kind, key, (unsigned)o + (unsigned)k, want_ir, a[1][k + 1], nb, po.v[k], io.v[k]);
	}
	*(ht_pixels<N> *)(out + (size_t)f * frame_px + o) = po;
	if (want_ir) *(ss_ir<N> *)(ir + (size_t)f * frame_px + o) = io;
}
template <int N> __global__ __launch_bounds__(SS_THREADS) void k_sensor_simulate(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, uint8_t *__restrict__ ir, int kind, int w, int h,
                                                                                 unsigned per_row, unsigned per_frame, unsigned B, const ht_sensor_noise nz)
{
	const unsigned r = blockIdx.x * SS_THREADS + threadIdx.x;
	if (r >= per_frame) return;
	const int y = (int)(r / per_row), x0 = (int)(r - (unsigned)y * per_row) * N;
	for (unsigned f = blockIdx.y; f < B; f += gridDim.y) ss_vector<N>(in, out, ir, kind, w, h, y, x0, f, nz);
}

// x86's truncating float -> int conversion, then the low 16 bits (sn_fill above, on the host)
static int ss_trunc16(float q)
{
	const int v = (q >= -2147483648.0f && q < 2147483648.0f) ? (int)q : INT_MIN;
	return (int)((unsigned)v & 0xFFFFu);
}
extern "C" int ht_sensor_noise_default(int kind, float depth_scale, float far, ht_sensor_noise *out)
{
	if (!out || (kind != HT_SENSOR_IVY && kind != HT_SENSOR_DS4) || !(depth_scale > 0.0f) || !(far > 0.0f)) return HT_ERR_ARG;
	const int far_count = ss_trunc16(far / depth_scale);
	if (far_count == 0) return HT_ERR_ARG;
	const bool ds4 = kind == HT_SENSOR_DS4;
	const double c = 1.0 / (double)depth_scale;      // counts per metre
	auto rnd = [](double v, double hi) { return (int)(v < 0.0 ? 0.0 : v > hi ? hi : v + 0.5); };
	ht_sensor_noise n;
	memset(&n, 0, sizeof n);
	n.far_count = far_count;
	n.sigma0_256 = rnd(256.0 * (ds4 ? 0.0002 : 0.0005) * c, 65536.0);
	n.sigma2 = rnd(268435456.0 * (ds4 ? 0.004 : 0.002) / c, 4096.0);
	n.edge_step = rnd(0.020 * c, 65535.0); n.slope_step = rnd(0.015 * c, 65535.0);
	n.p_edge_drop = rnd(65536.0 * (ds4 ? 0.25 : 0.35), 65536.0); n.p_edge_fly = rnd(65536.0 * (ds4 ? 0.35 : 0.25), 65536.0);
	n.p_slope_drop = 32768; n.p_hole = rnd(65536.0 * (ds4 ? 0.01 : 0.002), 65536.0);
	n.fly_bg_count = far_count < 65535 ? far_count : 65535;
	n.disparity_k = ds4 ? rnd(305.0 * 0.070 * 32.0 * c, 1073741824.0) : 0;
	n.wall_count = 0;
	n.ir_floor = 16; n.ir_gain = rnd(c * c / 8.0, 2147483647.0); n.ir_noise = 8;
	*out = n;
	return HT_OK;
}

// every check both forms share, made before anything is launched or grown
static int ss_check(ht_ctx *ctx, int kind, const void *depth, int w, int h, int B, const ht_sensor_noise *nz, const void *depth_out, const void *ir_out)
{
	const char *bad = nullptr;
	auto in = [](int v, long long hi) { return v >= 0 && (long long)v <= hi; };
	if (kind != HT_SENSOR_IVY && kind != HT_SENSOR_DS4) bad = "kind";
	else if (!ht_frame_dims_ok(w, h)) bad = "w and h between 1 and 4096";
	else if (B < 0) bad = "B";
	else if (!depth || !depth_out || !nz) bad = "a NULL buffer";
	else if (kind == HT_SENSOR_DS4 && !ir_out) bad = "DS4 needs ir_out";
	else if (nz->far_count < 1 || nz->far_count > 65536) bad = "far_count between 1 and 65536";
	else if (!in(nz->p_edge_drop, 65536) || !in(nz->p_edge_fly, 65536) || !in(nz->p_slope_drop, 65536) || !in(nz->p_hole, 65536) || nz->p_edge_drop + nz->p_edge_fly > 65536)
		bad = "a probability outside [0, 65536], or p_edge_drop + p_edge_fly above it";
	else if (!in(nz->sigma0_256, 65536) || !in(nz->sigma2, 4096) || !in(nz->edge_step, 65535) || !in(nz->slope_step, 65535) || !in(nz->fly_bg_count, 65535) || !in(nz->wall_count, 65535) ||
	         !in(nz->disparity_k, 1 << 30) || !in(nz->ir_floor, 65536) || nz->ir_gain < 0 || !in(nz->ir_noise, 65536))
		bad = "a noise figure outside its range";
	else if (ht_ranges_overlap(depth, (size_t)B * w * h * sizeof(uint16_t), depth_out, (size_t)B * w * h * sizeof(uint16_t))) bad = "depth_out overlaps depth";
	if (bad) { ctx->err = std::string("ht_sensor_simulate: bad argument (") + bad + ")"; return HT_ERR_ARG; }
	return HT_OK;
}

extern "C" int ht_sensor_simulate_dev(ht_ctx *ctx, int kind, const uint16_t *d_depth, int w, int h, int B, const ht_sensor_noise *noise, uint16_t *d_depth_out, uint8_t *d_ir_out, void *stream)
{
	CHECK_READY(ctx);
	{ const int r = ss_check(ctx, kind, d_depth, w, h, B, noise, d_depth_out, d_ir_out); if (r) return r; }
	if (B == 0) return HT_OK;
	hipStream_t s = ht_user_stream(ctx, stream);
	{
		ht_prof_scope ps(ctx, "k_sensor_simulate", s);
		// the IR image's store is N bytes: its address counts doubled
		ht_frame_vec_dispatch(ht_frame_vec_pixels((uintptr_t)d_depth | (uintptr_t)d_depth_out | ((uintptr_t)d_ir_out << 1), w), [&](auto px)
		{
			const ht_frame_grid g(w, h, B, px, SS_THREADS);
			hipLaunchKernelGGL(k_sensor_simulate<px>, g.grid, dim3(SS_THREADS), 0, s, d_depth, d_depth_out, d_ir_out, kind, w, h, g.per_row, g.per_frame, (unsigned)B, *noise);
		});
	}
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}

extern "C" int ht_sensor_simulate(ht_ctx *ctx, int kind, const uint16_t *depth, int w, int h, int B, const ht_sensor_noise *noise, uint16_t *depth_out, uint8_t *ir_out)
{
	CHECK_READY(ctx);
	{ const int r = ss_check(ctx, kind, depth, w, h, B, noise, depth_out, ir_out); if (r) return r; }
	if (B == 0) return HT_OK;
	const size_t npx = (size_t)B * w * h;
	ht_seg seg[3] = { { (void *)depth, npx * sizeof(uint16_t), false }, { depth_out, npx * sizeof(uint16_t), true }, { ir_out, npx, true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return ht_sensor_simulate_dev(ctx, kind, (const uint16_t *)seg[0].dev, w, h, B, noise, (uint16_t *)seg[1].dev, (uint8_t *)seg[2].dev, s); });
}
