"""Times the several-views calls on 1024 resident slots with device events, every shape warmed first, each figure the median of --rounds interleaved
series of --steps launches with the series' spread (max - min), the protocol of tools/bench_mirror.py:

 (a) ht_fuse_views_dev on 1024 x 2 views of 320x240 (the bench hands seen by the bench camera and by a second one a quarter turn about the vertical through the palm),
     beside k_prepare_frame on the same 2048 frames as two launches of 1024 (ht_debug_prepare_frames_dev: the yardstick) and a device-to-device copy of the frames'
     bytes for scale.  Stated: whether the fused call stays within the two single-view launches plus twice their spread.
 (b) One ht_fit_views_dev pass on a fused cloud whose every origin is zero (the second camera turned about the origin), beside one pass of ht_fit_rows' own launch
     sequence on the same points (ht_debug_fit_rows_pass_dev), both from the same start state: the only difference is the origin table's look-up.  Bar: inside twice
     the latter's spread.

Exits 1 when (b)'s bar is missed.  Writes profiles/r28_views.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_mirror as BM  # noqa: E402
import views_ref as vr  # noqa: E402
from hand_tracking_samples_amd import build as hb, native  # noqa: E402

B, W, H = BM.B, 320, 240


def second_views(ctx, truth, cam0, cams1):
    """the hands as the posed cameras cams1 [B,12] see them: the rasteriser reads a camera's intrinsics, so the poses go into each camera's space first"""
    local = np.stack([vr.into_camera(truth[i], cams1[i]) for i in range(len(truth))])
    return ctx.raster_mesh_depth(local, np.tile(cam0, (len(truth), 1)), W, H, 4.0, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--fit-steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_views.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    truth = z["gtpose"].astype(np.float32)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev); st = s.cuda_stream
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int
    ctx = native.Context(BM.M17, B)
    res = {"device": torch.cuda.get_device_name(0), "slots": B, "views": 2, "frame": "%dx%d" % (W, H), "steps": a.steps, "fit_steps": a.fit_steps, "rounds": a.rounds,
           "resources": {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "LDS Size", "Occupancy", "SGPRs Spill") if q in v} for k, v in hb.resource_usage().items() if any(n in k for n in ("k_fuse_views", "k_view_rows", "k_cloud_rows", "k_prepare_frame"))}}
    ok = True
    try:
        ctx.set_params(microforce=3.0)
        cam0 = vr.frame_camera(W, H)
        v0 = ctx.raster_mesh_depth(truth, np.tile(cam0, (B, 1)), W, H, 4.0, 0.5)
        # (a) the fused cloud beside the single-view launches
        cams1 = np.stack([vr.orbit(cam0, vr.palm(truth[i]), 90.0) for i in range(B)])
        v1 = second_views(ctx, truth, cam0, cams1)
        depth = np.ascontiguousarray(np.stack([v0, v1], axis=1)); cams = np.ascontiguousarray(np.stack([np.tile(cam0, (B, 1)), cams1], axis=1))
        nbytes = depth.nbytes
        with torch.cuda.stream(s):
            d_depth = torch.from_numpy(depth.view(np.int16)).to(dev); d_cams = torch.from_numpy(cams).to(dev)
            d_single = [torch.from_numpy(np.ascontiguousarray(v).view(np.int16)).to(dev) for v in (v0, v1)]
            d_scams = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in (np.tile(cam0, (B, 1)), cams1)]
            d_copy = torch.empty_like(d_depth)
        s.synchronize()
        opt = ctx.views_default()
        res["fraction"] = int(opt.fraction)

        def single():
            for k in range(2):
                ctx._chk(ctx.L.ht_debug_prepare_frames_dev(ctx.h, d_single[k].data_ptr(), d_scams[k].data_ptr(), W, H, B, st))
        fns = {"ht_fuse_views_dev, 1024 x 2 views": lambda: ctx.fuse_views_dev(d_depth.data_ptr(), d_cams.data_ptr(), W, H, 2, B, options=opt, stream=st),
               "k_prepare_frame, two launches of 1024 frames": single,
               "hipMemcpyAsync of the frames' bytes": lambda: hip.hipMemcpyAsync(d_copy.data_ptr(), d_depth.data_ptr(), nbytes, 3, st)}
        for fn in fns.values():
            fn()
        s.synchronize()
        ms = BM.interleaved(fns, s, a.steps, a.warmup, a.rounds)
        f, p, c = (BM.stat(ms[k]) for k in fns)
        row = {"bytes_read_once": nbytes, "fused": f, "single_view_launches": p, "copy": c, "fused_over_single": round(f["ms"] / p["ms"], 4), "fused_GBps_of_frame_bytes": round(nbytes / f["ms"] / 1e6, 1),
               "within_single_plus_twice_its_spread": bool(f["ms"] <= p["ms"] + 2 * p["spread_ms"]),
               "note": "k_prepare_frame gives every thread one contiguous run of the frame (a cache line a lane and load) and walks it twice; k_fuse_views walks a frame once, lanes on neighbouring pixels, "
                       "plus one counting walk over every earlier view of the slot"}
        res["fuse"] = row; print(json.dumps(row), flush=True)
        # (b) one fit pass, every origin zero, beside ht_fit_rows' sequence on the same points
        cams1 = np.stack([vr.turned(cam0, 3.0) for _ in range(B)])
        v1 = second_views(ctx, truth, cam0, cams1)
        depth = np.ascontiguousarray(np.stack([v0, v1], axis=1)); cams = np.ascontiguousarray(np.stack([np.tile(cam0, (B, 1)), cams1], axis=1))
        with torch.cuda.stream(s):
            d_depth.copy_(torch.from_numpy(depth.view(np.int16))); d_cams.copy_(torch.from_numpy(cams))
            d_org = torch.empty((B, 4, 3), dtype=torch.float32, device=dev); d_n = torch.empty(B, dtype=torch.int32, device=dev)
        ctx.fuse_views_dev(d_depth.data_ptr(), d_cams.data_ptr(), W, H, 2, B, options=opt, d_npoints=d_n.data_ptr(), d_origins=d_org.data_ptr(), stream=st)
        s.synchronize()
        npts = d_n.cpu().numpy()
        start = np.zeros((B, 17, 13), np.float32); start[:, :, :7] = np.roll(truth, -1, axis=0)      # one frame stale
        fns = {"ht_fit_views_dev, one pass": (0, lambda: ctx.fit_views_dev(0, B, 1, stream=st)),
               "ht_fit_rows' sequence, one pass": (1, lambda: ctx._chk(ctx.L.ht_debug_fit_rows_pass_dev(ctx.h, 1, B, st)))}
        out = {k: [] for k in fns}
        for rnd in range(a.rounds + 1):      # round 0 warms both
            for k, (which, fn) in fns.items():
                ctx.set_state(which, start)
                v = BM.series(fn, s, a.fit_steps, 0, 1)
                if rnd:
                    out[k] += v
        same = bool(np.array_equal(ctx.get_state(0, B).view(np.uint32), ctx.get_state(1, B).view(np.uint32)))
        v, r = (BM.stat(out[k]) for k in fns)
        row = {"points_per_slot_mean": round(float(npts.mean()), 1), "origins_all_zero": bool(not d_org.cpu().numpy().any()), "views": v, "rows": r, "difference_ms": round(v["ms"] - r["ms"], 5),
               "same_states_bit_for_bit": same, "within_bar": bool(abs(v["ms"] - r["ms"]) <= 2 * r["spread_ms"]) and same}
        ok = ok and row["within_bar"]
        res["fit_pass"] = row; print(json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out, "within_bars": ok}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
