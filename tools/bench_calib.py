"""Times ht_calibrate_view_dev on 1024 slots at 320x240 and 640x480 with device events, every shape warmed first, each figure the median of --rounds
interleaved series with the series' spread (max - min), the protocol of tools/bench_mirror.py.  The frames: the bench hands seen by ONE fixed second camera half way
round the mean palm (a rig), drawn by ht_raster_mesh_depth; the model poses are the ground truths, the guess is 2 degrees and 8 mm off the camera.

 (a) One iteration (k_calib_accum + k_calib_solve) as the difference of the call with iterations = 1 and with iterations = 0, both modes, taking turns.
 (b) The kernels bracketed by the context's own events (ht_profile_enable): k_calib_cloud, k_calib_accum, k_calib_solve, and k_split_model on the same frames and
     poses in the same session (ht_split_hands_model_dev, HT_SPLIT_MODEL_ALWAYS) -- that kernel does the same walk, a lane per (cell, hand).  closest() evaluations a
     second of both and their ratio.  Reported, not asserted.

Writes profiles/r29_calib.json (or --out)."""
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
import calib_ref as cr  # noqa: E402
import views_ref as vr  # noqa: E402
from hand_tracking_samples_amd import build as hb, native  # noqa: E402

B = BM.B


def rig_frames(ctx, truth, w, h, degrees):
    """(the frames [B,h,w] a fixed second camera sees, that camera, the poses in its space)"""
    cam0 = vr.frame_camera(w, h)
    cam1 = vr.orbit(cam0, truth[:, 0, :3].astype(np.float64).mean(0), degrees)
    local = np.stack([vr.into_camera(p, cam1) for p in truth])
    return ctx.raster_mesh_depth(local, np.tile(cam0, (len(truth), 1)), w, h, 4.0, 0.5), cam1, local


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="320x240,640x480")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_calib.json"))
    a = ap.parse_args()
    truth = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))["gtpose"].astype(np.float32)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev); st = s.cuda_stream
    ctx = native.Context(BM.M17, B)
    res = {"device": torch.cuda.get_device_name(0), "slots": B, "steps": a.steps, "rounds": a.rounds,
           "resources": {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "LDS Size", "Occupancy", "SGPRs Spill") if q in v} for k, v in hb.resource_usage().items() if any(n in k for n in ("k_calib_", "k_split_model"))}}
    try:
        for size in a.sizes.split(","):
            w, h = (int(x) for x in size.split("x"))
            depth, cam1, local = rig_frames(ctx, truth, w, h, 180.0)
            guess = np.tile(cr.perturbed(cam1, 2.0, 0.008), (B, 1))
            with torch.cuda.stream(s):
                d_depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(dev); d_cams = torch.from_numpy(guess).to(dev); d_poses = torch.from_numpy(truth).to(dev)
                d_T = torch.zeros((B, 7), dtype=torch.float32, device=dev); d_stats = torch.zeros((2, B, native.CALIB_STATS), dtype=torch.float64, device=dev)
                d_two = torch.from_numpy(np.ascontiguousarray(np.stack([local, local], axis=1))).to(dev)
                d_out = torch.empty((B, 2, h, w), dtype=torch.int16, device=dev); d_info = torch.zeros((B, 2, 8), dtype=torch.int32, device=dev)
            s.synchronize()
            opts = {(mode, it): ctx.calib_default(mode=mode, iterations=it) for mode in (native.CALIB_RIG, native.CALIB_PER_SLOT) for it in (0, 1)}
            row = {"fraction": int(opts[(0, 0)].fraction)}

            def calib(mode, it):
                return lambda: ctx.calibrate_view_dev(d_depth.data_ptr(), d_cams.data_ptr(), w, h, B, d_T.data_ptr(), d_stats.data_ptr(), d_poses=d_poses.data_ptr(), options=opts[(mode, it)], stream=st)

            def split():
                ctx.split_hands_model_dev(d_depth.data_ptr(), d_cams.data_ptr(), d_two.data_ptr(), w, h, B, 100, 700, 65535, 1, 4000, float("inf"), native.SPLIT_MODEL_ALWAYS, 0, d_out.data_ptr(), None, d_info.data_ptr(),
                                          stream=st)
            calib(native.CALIB_PER_SLOT, 0)(); split(); s.synchronize()
            points = int(d_stats.cpu().numpy()[0, :, 1].sum()); cells = int(d_info.cpu().numpy()[:, :, 0].sum())
            row["points"] = points; row["points_per_slot_mean"] = round(points / B, 1); row["split_foreground_cells"] = cells
            # (a) one iteration as a difference of whole calls
            fns = {"%s, iterations = %d" % ("RIG" if mode == native.CALIB_RIG else "PER_SLOT", it): calib(mode, it) for (mode, it) in opts}
            ms = {k: BM.stat(v) for k, v in BM.interleaved(fns, s, a.steps, a.warmup, a.rounds).items()}
            row["calls"] = ms
            for name in ("RIG", "PER_SLOT"):
                one = ms[name + ", iterations = 1"]["ms"] - ms[name + ", iterations = 0"]["ms"]
                row["one_iteration_ms, " + name] = round(one, 5)
                row["closest_evaluations_per_second, " + name] = round(points / one * 1e3) if one > 0 else None
            # (b) the kernels bracketed, taking turns with k_split_model
            ctx.profile_enable(1)
            per = {}
            for rnd in range(a.rounds + 1):      # round 0 warms
                for fn in (calib(native.CALIB_PER_SLOT, 1), split):
                    ctx.profile_read(reset=True)
                    for _ in range(a.steps):
                        fn()
                    s.synchronize()
                    for k, (t, n) in ctx.profile_read(reset=True).items():
                        if rnd and n and (k.startswith("k_calib_") or k == "k_split_model"):
                            per.setdefault(k, []).append(t / n)
            ctx.profile_enable(0)
            row["kernels"] = {k: BM.stat(v) for k, v in per.items()}
            acc, spl = row["kernels"]["k_calib_accum"]["ms"], row["kernels"]["k_split_model"]["ms"]
            row["k_calib_accum_evaluations_per_second"] = round(points / acc * 1e3); row["k_split_model_evaluations_per_second"] = round(2 * cells / spl * 1e3)
            row["rate_ratio_calib_over_split"] = round((points / acc) / (2 * cells / spl), 4)
            row["note"] = "k_split_model's launch also reads every pixel of the frame and labels the cells; k_calib_accum also forms 29 float64 sums a point and reduces them"
            res[size] = row; print(json.dumps({size: row}), flush=True)
            del d_depth, d_out
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
