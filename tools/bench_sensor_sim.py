"""Times ht_sensor_simulate_dev on 1024 resident frames at 320x240 and 640x480, per camera kind, with device events after a warm-up: the median of five interleaved
series, the spread stated.  In the same run, on the same frames:
  (a) a hipMemcpyAsync device-to-device copy of the bytes the call moves (the depth frames; for DS4 also as many bytes as the IR image has) -- the ratio is recorded,
      no bar: the per-pixel hash makes this stage partly arithmetic;
  (b) the update step the frames feed (ht_update_frames_dev at 320x240, ht_update_frames_sized_dev with the 64x64 net at 640x480) -- the bar of DESIGN section 17:
      a stage that feeds the tracker takes at most 0.25 of that step.
Writes profiles/r22_sensor_sim.json (or --out) and prints the table of DESIGN section 29.

Frames: the bench hands rendered at either size (ht_render_depth), the noise sets ht_sensor_noise_default's."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand_tracking_samples_amd import build as hb, native, weights as W  # noqa: E402

M17 = os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand17.htfx")


def time_it(fn, stream, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_sensor_sim.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    B = a.frames
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    ctx = native.Context(M17, B)
    rows = []
    try:
        ctx.load_weights(W.make_cnnb()); ctx.set_params(microforce=3.0, mainthreadpasses=3)
        poses = z["gtpose"][:B].astype(np.float32); start = z["startpose"][:B].astype(np.float32)
        for w, h in ((320, 240), (640, 480)):
            cams = np.zeros((B, 12), np.float32); cams[:, :5] = [305 * w / 320, 305 * w / 320, w / 2, h / 2, 0.001]; cams[:, 11] = 1
            clean = ctx.render_depth(poses, cams, w, h)
            n = B * w * h
            with torch.cuda.stream(s):
                tin = torch.from_numpy(clean.view(np.int16)).to(dev); tc = torch.from_numpy(cams).to(dev); ts = torch.from_numpy(start).to(dev)
                tout = torch.empty((B, h, w), dtype=torch.int16, device=dev); tir = torch.empty((B, h, w), dtype=torch.uint8, device=dev); tir2 = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
                poses_out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev)
            s.synchronize()
            del clean
            if w == 320:
                update = lambda st=None: ctx.update_frames_dev(tin.data_ptr(), tc.data_ptr(), w, h, 0.17, st, B, poses_out.data_ptr(), s.cuda_stream)
                update_name = "ht_update_frames_dev"
            else:
                update = lambda st=None: ctx.update_frames_sized_dev(64, tin.data_ptr(), tc.data_ptr(), w, h, 0.17, st, B, poses_out.data_ptr(), s.cuda_stream)
                update_name = "ht_update_frames_sized_dev, side 64"
            ivy = native.sensor_noise_default(native.SENSOR_IVY, 0.001, 4.0, seed=1)
            ds4 = native.sensor_noise_default(native.SENSOR_DS4, 0.001, 4.0, seed=1)

            def copy(with_ir):
                with torch.cuda.stream(s):      # contiguous tensors of one type on one device: Tensor.copy_ is one hipMemcpyAsync, device to device
                    tout.copy_(tin, non_blocking=True)
                    if with_ir:
                        tir2.copy_(tir, non_blocking=True)
            calls = {
                "simulate Ivy": lambda: ctx.sensor_simulate_dev(native.SENSOR_IVY, tin.data_ptr(), w, h, B, ivy, tout.data_ptr(), None, s.cuda_stream),
                "simulate Ivy with IR": lambda: ctx.sensor_simulate_dev(native.SENSOR_IVY, tin.data_ptr(), w, h, B, ivy, tout.data_ptr(), tir.data_ptr(), s.cuda_stream),
                "simulate DS4": lambda: ctx.sensor_simulate_dev(native.SENSOR_DS4, tin.data_ptr(), w, h, B, ds4, tout.data_ptr(), tir.data_ptr(), s.cuda_stream),
                "copy depth": lambda: copy(False),
                "copy depth and IR": lambda: copy(True),
            }
            update(ts.data_ptr())
            for fn in calls.values():
                for _ in range(a.warmup):
                    fn()
            s.synchronize()
            t = {k: [] for k in list(calls) + ["update"]}
            for _ in range(a.series):      # interleaved: every series times every call once
                for k, fn in calls.items():
                    t[k].append(time_it(fn, s, a.steps))
                t["update"].append(time_it(update, s, 2))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in t.items()}
            for k, against in (("simulate Ivy", "copy depth"), ("simulate Ivy with IR", "copy depth and IR"), ("simulate DS4", "copy depth and IR")):
                moved = n * (4 if k == "simulate Ivy" else 5)
                row = {"call": k, "w": w, "h": h, "B": B, "ms": round(med[k], 4), "spread": round(spread[k], 4), "series_ms": [round(x, 4) for x in t[k]], "bytes_moved": moved,
                       "TBps": round(moved / med[k] / 1e9, 3), "copy": against, "copy_ms": round(med[against], 4), "copy_spread": round(spread[against], 4), "over_copy": round(med[k] / med[against], 3),
                       "update": update_name, "update_ms": round(med["update"], 3), "update_spread": round(spread["update"], 4), "over_update": round(med[k] / med["update"], 5),
                       "bar_0.25_of_update_met": bool(med[k] <= 0.25 * med["update"]), "ns_per_pixel": round(med[k] * 1e6 / n, 4)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del tin, tout, tir, tir2
            torch.cuda.empty_cache()
    finally:
        ctx.close()
    usage = {k: {"VGPRs": v["VGPRs"], "SGPRs": v.get("TotalSGPRs"), "Occupancy": v["Occupancy"], "ScratchSize": v["ScratchSize"]} for k, v in hb.resource_usage().items() if "k_sensor_simulate" in k}
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "series": a.series, "warmup": a.warmup, "bar": "the stage <= 0.25 of the update step on the same frames (DESIGN section 17)",
           "kernel": usage, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("| call | frames | ms (spread) | TB/s moved | copy ms (spread) | over copy | update ms | over update | bar 0.25 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d x %dx%d | %.3f (%.1f %%) | %.2f | %.3f (%.1f %%) | %.2f | %.1f | %.4f | %s |" % (r["call"], r["B"], r["w"], r["h"], r["ms"], 100 * r["spread"], r["TBps"], r["copy_ms"], 100 * r["copy_spread"],
                                                                                                      r["over_copy"], r["update_ms"], r["over_update"], "met" if r["bar_0.25_of_update_met"] else "MISSED"))
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
