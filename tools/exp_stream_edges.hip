// exp_stream_edges.hip -- experiment: what does one fork / join edge between two streams of one device cost on gfx950, by the flags of its event and by who records it, and
// does every form still make the producer's writes visible to a consumer kernel on the other stream?  ("Streams"; profiles/r30_stream_edges.md.)
// The fit step's shape on a main stream and a non-blocking side stream, 200 times between two timing events on the main stream:
//     K1 (main) -> fork -> { K2 (main) || K3 (side) } -> join -> K4 (main)
// K1 ~100 us and K4 ~20 us; K2 / K3 are ~100 / ~20 us ("hidden": the join's record is long done when K2 ends) and ~20 / ~100 us ("exposed": K4 waits for the join itself).
// Every kernel is a dependent FMA chain of a fixed trip count on one wave per block (the counts are set once at the start from one timed launch); nothing spins or polls.
// Variants:  one_stream (yardstick: no edges, everything in order)
//            plain              hipEventDisableTiming, hipEventRecord + hipStreamWaitEvent                       (the library's edges up to round 29)
//            nofence            ... | hipEventDisableSystemFence
//            todevice           ... | hipEventReleaseToDevice
//            stop_plain / stop_nofence / stop_todevice: the same three kinds of event handed to K1 (fork) and K3 (join) as the stopEvent of hipExtLaunchKernelGGL, no record
// Reported per variant and case: mean us per repetition minus the ideal K1 + max(K2, K3) + K4 (each kernel's own time from 200 back-to-back launches on one stream), for
// each of ROUNDS rounds.  Visibility in the same run: K1 writes a counter pattern into a 32 MB buffer at its very end (blocks on every XCD); K3 and K4 read all of it at
// their very start and compare; K3 writes a second buffer (8 MB) at its end that K4 checks.  The pattern changes every repetition, so a stale line cannot pass.  A variant
// with a mismatch is reported with its count and the program exits with status 1.
//   hipcc --offload-arch=gfx950 -O2 tools/exp_stream_edges.hip -o exp_stream_edges && ./exp_stream_edges > profiles/r30_stream_edges_probe.json
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

#define CHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } } while (0)

struct job
{
	const uint4 *rd0; size_t rd0_n; uint32_t rd0_pat;      // read and compare first (n in uint4), word k must be pat + k
	const uint4 *rd1; size_t rd1_n; uint32_t rd1_pat;
	int trips;                                              // then the chain, on wave 0 of every block
	uint4 *wr; size_t wr_n; uint32_t wr_pat;                // then write
	unsigned *bad; float *sink;
};
__device__ __forceinline__ unsigned check(const uint4 *p, size_t n, uint32_t pat, size_t t, size_t nt)
{
	unsigned bad = 0;
	for (size_t q = t; q < n; q += nt)
	{
		const uint4 v = p[q]; const uint32_t w = pat + (uint32_t)(4 * q);
		bad += (v.x != w) + (v.y != w + 1) + (v.z != w + 2) + (v.w != w + 3);
	}
	return bad;
}
__global__ __launch_bounds__(256) void k_edge(job j)
{
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nt = (size_t)gridDim.x * 256;
	unsigned bad = 0;
	if (j.rd0) bad += check(j.rd0, j.rd0_n, j.rd0_pat, t, nt);
	if (j.rd1) bad += check(j.rd1, j.rd1_n, j.rd1_pat, t, nt);
	if (bad) atomicAdd(j.bad, bad);
	if (threadIdx.x < 64)
	{
		float x = 1.0f + (float)threadIdx.x;
		for (int i = 0; i < j.trips; i++) x = __builtin_fmaf(x, 0.99999994f, 1e-7f);
		if (x == -1.0f) *j.sink = x;      // never: keeps the chain
	}
	__syncthreads();
	if (j.wr) for (size_t q = t; q < j.wr_n; q += nt) { const uint32_t w = j.wr_pat + (uint32_t)(4 * q); j.wr[q] = make_uint4(w, w + 1, w + 2, w + 3); }
}

enum { ONE_STREAM, PLAIN, NOFENCE, TODEVICE, STOP_PLAIN, STOP_NOFENCE, STOP_TODEVICE, NVARIANT };
static const char *const names[NVARIANT] = { "one_stream", "plain", "nofence", "todevice", "stop_plain", "stop_nofence", "stop_todevice" };
static const unsigned ev_flags[NVARIANT] = { 0, hipEventDisableTiming, hipEventDisableTiming | hipEventDisableSystemFence, hipEventDisableTiming | hipEventReleaseToDevice,
                                             hipEventDisableTiming, hipEventDisableTiming | hipEventDisableSystemFence, hipEventDisableTiming | hipEventReleaseToDevice };
enum { REPS = 200, WARM = 5, ROUNDS = 3, GRID_MEM = 256, GRID_K2 = 64 };
static const size_t A_N = (32u << 20) / 16, B_N = (8u << 20) / 16;      // uint4

struct rig { hipStream_t s, u; hipEvent_t t0, t1; uint4 *A, *B; unsigned *bad; float *sink; int trips_long, trips_short; uint32_t rep; };

static void launch(const job &j, int grid, hipStream_t s, hipEvent_t stop)
{
	if (stop) hipExtLaunchKernelGGL(k_edge, dim3(grid), dim3(256), 0, s, nullptr, stop, 0, j);
	else hipLaunchKernelGGL(k_edge, dim3(grid), dim3(256), 0, s, j);
}
// the four kernels of repetition `rep`; long_side: K3 is the long one
static job make_job(const rig &r, int k, bool long_side, uint32_t rep)
{
	const uint32_t pa = rep * 0x9E3779B1u, pb = ~pa;
	job j = {}; j.bad = r.bad; j.sink = r.sink;
	if (k == 1) { j.trips = r.trips_long; j.wr = r.A; j.wr_n = A_N; j.wr_pat = pa; }
	if (k == 2) { j.trips = long_side ? r.trips_short : r.trips_long; }
	if (k == 3) { j.rd0 = r.A; j.rd0_n = A_N; j.rd0_pat = pa; j.trips = long_side ? r.trips_long : r.trips_short; j.wr = r.B; j.wr_n = B_N; j.wr_pat = pb; }
	if (k == 4) { j.rd0 = r.A; j.rd0_n = A_N; j.rd0_pat = pa; j.rd1 = r.B; j.rd1_n = B_N; j.rd1_pat = pb; j.trips = r.trips_short; }
	return j;
}
static void one_rep(rig &r, int v, bool long_side, hipEvent_t ef, hipEvent_t ej)
{
	const uint32_t rep = ++r.rep; const bool stop = v >= STOP_PLAIN, side = v != ONE_STREAM;
	launch(make_job(r, 1, long_side, rep), GRID_MEM, r.s, stop ? ef : nullptr);
	if (side) { if (!stop) CHK(hipEventRecord(ef, r.s)); CHK(hipStreamWaitEvent(r.u, ef, 0)); }
	if (side) launch(make_job(r, 3, long_side, rep), GRID_MEM, r.u, stop ? ej : nullptr);      // the side stream's kernel first, as the library enqueues a fit step
	launch(make_job(r, 2, long_side, rep), GRID_K2, r.s, nullptr);
	if (!side) launch(make_job(r, 3, long_side, rep), GRID_MEM, r.s, nullptr);
	if (side) { if (!stop) CHK(hipEventRecord(ej, r.u)); CHK(hipStreamWaitEvent(r.s, ej, 0)); }
	launch(make_job(r, 4, long_side, rep), GRID_MEM, r.s, nullptr);
}
static float timed(rig &r, int v, bool long_side, hipEvent_t ef, hipEvent_t ej)      // us per repetition
{
	for (int i = 0; i < WARM; i++) one_rep(r, v, long_side, ef, ej);
	CHK(hipEventRecord(r.t0, r.s));
	for (int i = 0; i < REPS; i++) one_rep(r, v, long_side, ef, ej);
	CHK(hipEventRecord(r.t1, r.s)); CHK(hipEventSynchronize(r.t1)); CHK(hipGetLastError()); CHK(hipStreamSynchronize(r.u));
	float ms = 0; CHK(hipEventElapsedTime(&ms, r.t0, r.t1));
	return ms * 1000.0f / REPS;
}
// one kernel of the shape alone, back to back on the main stream (its inputs written once before, so the compare passes); us per launch, one ordinary boundary included
static float alone(rig &r, int k, bool long_side)
{
	const uint32_t rep = ++r.rep;
	launch(make_job(r, 1, long_side, rep), GRID_MEM, r.s, nullptr);
	launch(make_job(r, 3, long_side, rep), GRID_MEM, r.s, nullptr);
	const job j = make_job(r, k, long_side, rep); const int grid = k == 2 ? GRID_K2 : GRID_MEM;
	for (int i = 0; i < WARM; i++) launch(j, grid, r.s, nullptr);
	CHK(hipEventRecord(r.t0, r.s));
	for (int i = 0; i < REPS; i++) launch(j, grid, r.s, nullptr);
	CHK(hipEventRecord(r.t1, r.s)); CHK(hipEventSynchronize(r.t1)); CHK(hipGetLastError());
	float ms = 0; CHK(hipEventElapsedTime(&ms, r.t0, r.t1));
	return ms * 1000.0f / REPS;
}
static unsigned take_bad(rig &r) { unsigned h = 0; CHK(hipMemcpy(&h, r.bad, sizeof h, hipMemcpyDeviceToHost)); CHK(hipMemset(r.bad, 0, sizeof h)); return h; }

int main()
{
	rig r = {};
	CHK(hipStreamCreateWithFlags(&r.s, hipStreamNonBlocking)); CHK(hipStreamCreateWithFlags(&r.u, hipStreamNonBlocking));
	CHK(hipEventCreate(&r.t0)); CHK(hipEventCreate(&r.t1));
	CHK(hipMalloc(&r.A, A_N * 16)); CHK(hipMalloc(&r.B, B_N * 16)); CHK(hipMalloc(&r.bad, 4)); CHK(hipMalloc(&r.sink, 4));
	CHK(hipMemset(r.bad, 0, 4)); CHK(hipMemset(r.A, 0, A_N * 16)); CHK(hipMemset(r.B, 0, B_N * 16));
	hipDeviceProp_t prop; CHK(hipGetDeviceProperties(&prop, 0));
	{      // the trip counts: one timed chain of 200000 trips sets clocks per trip; fixed from here on
		job j = {}; j.bad = r.bad; j.sink = r.sink; j.trips = 200000;
		launch(j, GRID_K2, r.s, nullptr); CHK(hipStreamSynchronize(r.s));
		CHK(hipEventRecord(r.t0, r.s)); launch(j, GRID_K2, r.s, nullptr); CHK(hipEventRecord(r.t1, r.s)); CHK(hipEventSynchronize(r.t1));
		float ms = 0; CHK(hipEventElapsedTime(&ms, r.t0, r.t1));
		const double us_per_trip = ms * 1000.0 / j.trips;
		r.trips_long = (int)(100.0 / us_per_trip); r.trips_short = (int)(20.0 / us_per_trip);
	}
	printf("{\n  \"device\": \"%s\", \"arch\": \"%s\", \"reps\": %d, \"rounds\": %d, \"trips_long\": %d, \"trips_short\": %d, \"buffer_a_mb\": 32, \"buffer_b_mb\": 8,\n", prop.name, prop.gcnArchName, REPS, ROUNDS, r.trips_long, r.trips_short);
	unsigned total_bad = 0;
	float k_us[2][5] = {};
	for (int c = 0; c < 2; c++) for (int k = 1; k <= 4; k++) k_us[c][k] = alone(r, k, c == 1);
	total_bad += take_bad(r);
	printf("  \"kernels_alone_us\": { \"hidden\": [%.2f, %.2f, %.2f, %.2f], \"exposed\": [%.2f, %.2f, %.2f, %.2f], \"mismatches\": %u },\n",
	       k_us[0][1], k_us[0][2], k_us[0][3], k_us[0][4], k_us[1][1], k_us[1][2], k_us[1][3], k_us[1][4], total_bad);
	float ideal[2];
	for (int c = 0; c < 2; c++) ideal[c] = k_us[c][1] + std::max(k_us[c][2], k_us[c][3]) + k_us[c][4];
	printf("  \"ideal_us\": { \"hidden\": %.2f, \"exposed\": %.2f },\n  \"variants\": [\n", ideal[0], ideal[1]);
	hipEvent_t ef[NVARIANT] = {}, ej[NVARIANT] = {};
	for (int v = 1; v < NVARIANT; v++) { CHK(hipEventCreateWithFlags(&ef[v], ev_flags[v])); CHK(hipEventCreateWithFlags(&ej[v], ev_flags[v])); }
	float us[NVARIANT][2][ROUNDS]; unsigned bad[NVARIANT] = {};
	for (int round = 0; round < ROUNDS; round++)      // the variants take turns, so a drift of the clocks touches all of them alike
		for (int v = 0; v < NVARIANT; v++)
		{
			for (int c = 0; c < 2; c++) us[v][c][round] = timed(r, v, c == 1, ef[v], ej[v]);
			bad[v] += take_bad(r);
		}
	for (int v = 0; v < NVARIANT; v++)
	{
		printf("    { \"name\": \"%s\", \"event_flags\": \"0x%x\", \"mismatches\": %u", names[v], ev_flags[v], bad[v]);
		for (int c = 0; c < 2; c++)
		{
			printf(", \"%s_us\": [", c ? "exposed" : "hidden");
			for (int i = 0; i < ROUNDS; i++) printf("%s%.2f", i ? ", " : "", us[v][c][i]);
			printf("], \"%s_over_ideal_us\": [", c ? "exposed" : "hidden");
			for (int i = 0; i < ROUNDS; i++) printf("%s%.2f", i ? ", " : "", us[v][c][i] - ideal[c]);
			printf("]");
		}
		printf(" }%s\n", v + 1 < NVARIANT ? "," : "");
		total_bad += bad[v];
	}
	printf("  ],\n  \"visibility_ok\": %s\n}\n", total_bad ? "false" : "true");
	return total_bad ? 1 : 0;
}
