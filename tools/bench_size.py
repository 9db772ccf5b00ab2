"""Times ht_estimate_scale_dev on 1024 slots at 320x240 and 640x480, fraction 4, with device events, every shape warmed first, each figure the
median of --rounds interleaved series with the series' spread (max - min), the protocol of tools/bench_calib.py.  The frames: the bench hands seen by the frame camera,
drawn by ht_raster_mesh_depth; the model poses are the ground truths, scale0 = 1.1.

 (a) One iteration (k_size_accum + k_size_solve) as the difference of the call with iterations = 1 and with iterations = 0, in each of the four combinations of mode
     and free_pose, taking turns.
 (b) The kernels bracketed by the context's own events (ht_profile_enable): k_size_accum and k_size_solve (SHARED and PER_SLOT, free_pose 1) beside k_calib_accum and
     k_calib_solve of ht_calibrate_view_dev on the same frames and poses in the same session, taking turns.  The bar: k_size_accum forms 37 float64
     sums where k_calib_accum forms 29 over the same closest() walk, so it may take at most 37 / 29 times k_calib_accum plus the larger of the two spreads.  Reported
     with its verdict, not asserted here.

Writes profiles/r30_size.json (or --out)."""
import argparse
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

B = BM.B
COMBOS = [(native.SIZE_SHARED, 0), (native.SIZE_SHARED, 1), (native.SIZE_PER_SLOT, 0), (native.SIZE_PER_SLOT, 1)]


def _name(mode, free_pose):
    return "%s, free_pose = %d" % ("SHARED" if mode == native.SIZE_SHARED else "PER_SLOT", free_pose)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="320x240,640x480")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_size.json"))
    a = ap.parse_args()
    truth = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))["gtpose"].astype(np.float32)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev); st = s.cuda_stream
    ctx = native.Context(BM.M17, B)
    res = {"device": torch.cuda.get_device_name(0), "slots": B, "steps": a.steps, "rounds": a.rounds, "bar": "k_size_accum <= 37 / 29 * k_calib_accum + the larger spread",
           "resources": {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "LDS Size", "Occupancy", "SGPRs Spill") if q in v} for k, v in hb.resource_usage().items() if any(n in k for n in ("k_size_", "k_calib_"))}}
    try:
        for size in a.sizes.split(","):
            w, h = (int(x) for x in size.split("x"))
            cams = np.tile(vr.frame_camera(w, h), (B, 1))
            depth = ctx.raster_mesh_depth(truth, cams, w, h, 4.0, 0.5)
            with torch.cuda.stream(s):
                d_depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(dev); d_cams = torch.from_numpy(cams).to(dev); d_poses = torch.from_numpy(truth).to(dev)
                d_sc = torch.zeros(B, dtype=torch.float32, device=dev); d_T = torch.zeros((B, 7), dtype=torch.float32, device=dev)
                d_stats = torch.zeros((2, native.size_row(B, B)), dtype=torch.float64, device=dev); d_cstats = torch.zeros((2, B, native.CALIB_STATS), dtype=torch.float64, device=dev)
            s.synchronize()
            opts = {(mode, fp, it): ctx.size_default(mode=mode, free_pose=fp, iterations=it, fraction=4, scale0=1.1) for (mode, fp) in COMBOS for it in (0, 1)}
            copt = ctx.calib_default(mode=native.CALIB_PER_SLOT, iterations=1, fraction=4)
            row = {"fraction": 4}

            def est(mode, fp, it):
                return lambda: ctx.estimate_scale_dev(d_depth.data_ptr(), d_cams.data_ptr(), w, h, B, d_sc.data_ptr(), d_T.data_ptr(), d_stats.data_ptr(), d_poses=d_poses.data_ptr(), options=opts[(mode, fp, it)],
                                                      stream=st)

            def calib():
                ctx.calibrate_view_dev(d_depth.data_ptr(), d_cams.data_ptr(), w, h, B, d_T.data_ptr(), d_cstats.data_ptr(), d_poses=d_poses.data_ptr(), options=copt, stream=st)
            est(native.SIZE_SHARED, 1, 0)(); s.synchronize()
            points = int(d_stats.cpu().numpy()[0, 1]); row["points"] = points; row["points_per_slot_mean"] = round(points / B, 1)
            # (a) one iteration as a difference of whole calls
            fns = {"%s, iterations = %d" % (_name(mode, fp), it): est(mode, fp, it) for (mode, fp, it) in opts}
            ms = {k: BM.stat(v) for k, v in BM.interleaved(fns, s, a.steps, a.warmup, a.rounds).items()}
            row["calls"] = ms
            for mode, fp in COMBOS:
                one = ms[_name(mode, fp) + ", iterations = 1"]["ms"] - ms[_name(mode, fp) + ", iterations = 0"]["ms"]
                row["one_iteration_ms, " + _name(mode, fp)] = round(one, 5)
            # (b) the kernels bracketed, taking turns with the calibration's
            ctx.profile_enable(1)
            per = {}
            runs = {"SHARED": est(native.SIZE_SHARED, 1, 1), "PER_SLOT": est(native.SIZE_PER_SLOT, 1, 1), "calib": calib}
            for rnd in range(a.rounds + 1):      # round 0 warms
                for tag, fn in runs.items():
                    ctx.profile_read(reset=True)
                    for _ in range(a.steps):
                        fn()
                    s.synchronize()
                    for k, (t, n) in ctx.profile_read(reset=True).items():
                        if rnd and n and (k.startswith("k_size_") or k.startswith("k_calib_")):
                            per.setdefault(k if tag == "calib" or k.startswith("k_calib_") else "%s (%s)" % (k, tag), []).append(t / n)
            ctx.profile_enable(0)
            row["kernels"] = {k: BM.stat(v) for k, v in per.items()}
            ca = row["kernels"]["k_calib_accum"]
            for tag in ("SHARED", "PER_SLOT"):
                sa = row["kernels"]["k_size_accum (%s)" % tag]
                bar = 37.0 / 29.0 * ca["ms"] + max(ca["spread_ms"], sa["spread_ms"])
                row["k_size_accum over k_calib_accum (%s)" % tag] = {"ratio": round(sa["ms"] / ca["ms"], 4), "bar_ms": round(bar, 5), "met": bool(sa["ms"] <= bar)}
            row["closest_evaluations_per_second, k_size_accum"] = round(points / row["kernels"]["k_size_accum (SHARED)"]["ms"] * 1e3)
            res[size] = row; print(json.dumps({size: row}), flush=True)
            del d_depth
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
