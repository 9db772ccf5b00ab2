"""Times the joint-coordinate calls (ht_sample_poses_dev with and without HT_SAMPLE_ENHANCED, ht_joint_pose_dev, ht_joint_coords_dev) beside ht_render_depth_dev
at 320x240 on the same poses in the same run: resident batches of 1024 and 8192 frames of the 17-bone hand, device events, every shape warmed first, each figure the
median of --rounds series of --steps launches with the series' spread (max - min).  The sampler feeds the renderer, so the bar is DESIGN section 17's: a stage that
feeds another takes at most 0.25 of it.  Exits 1 when a stage misses it.

Writes profiles/r18_joints.json (or --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand_tracking_samples_amd import build as hb, native  # noqa: E402

M17 = os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand17.htfx")
QVGA_CAM = np.array([305, 305, 160, 120, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)
BAR = 0.25


def series(fn, stream, steps, warmup, rounds):
    out = []
    for _ in range(rounds):
        for _ in range(warmup):
            fn()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_joints.json"))
    a = ap.parse_args()
    gt = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))["gtpose"].astype(np.float32)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    ctx = native.Context(M17, 4)
    res = {"device": torch.cuda.get_device_name(0), "model": "17 bones, 16 joints", "steps": a.steps, "rounds": a.rounds, "bar": "stage <= %.2f x ht_render_depth_dev 320x240 on the same poses (DESIGN section 17)" % BAR,
           "resources": {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "Occupancy") if q in v} for k, v in hb.resource_usage().items() if any(n in k for n in ("k_joint_coords", "k_joint_pose", "k_sample_poses"))},
           "rows": []}
    ok = True
    try:
        for B in (1024, 8192):
            with torch.cuda.stream(s):
                roots = torch.from_numpy(np.ascontiguousarray(gt[np.arange(B) % len(gt), 0])).to(dev); cams = torch.from_numpy(np.tile(QVGA_CAM, (B, 1))).to(dev)
                poses = torch.empty((B, 17, 7), device=dev); coords = torch.empty((B, 16, 3), device=dev); gaps = torch.empty((B, 16), device=dev)
                depth = torch.empty((B, 240, 320), dtype=torch.int16, device=dev)
            st = s.cuda_stream
            calls = {
                "ht_sample_poses_dev": lambda: ctx.sample_poses_dev(roots.data_ptr(), B, 1, 0, 0.98, poses.data_ptr(), coords.data_ptr(), com_poses=True, stream=st),
                "ht_sample_poses_dev HT_SAMPLE_ENHANCED": lambda: ctx.sample_poses_dev(roots.data_ptr(), B, 1, 0, 0.98, poses.data_ptr(), coords.data_ptr(), com_poses=True, enhanced=True, stream=st),
                "ht_joint_pose_dev": lambda: ctx.joint_pose_dev(roots.data_ptr(), coords.data_ptr(), B, poses.data_ptr(), com_poses=True, stream=st),
                "ht_joint_coords_dev": lambda: ctx.joint_coords_dev(poses.data_ptr(), B, coords.data_ptr(), gaps.data_ptr(), com_poses=True, stream=st),
                "ht_render_depth_dev 320x240": lambda: ctx.render_depth_dev(poses.data_ptr(), cams.data_ptr(), 320, 240, 4.0, B, depth.data_ptr(), None, st),
            }
            for fn in calls.values():      # every shape once before anything is timed; the render last, so that it draws the sampled poses
                fn()
            s.synchronize()
            ms = {k: series(fn, s, a.steps if "render" not in k else max(4, a.steps // 10), a.warmup, a.rounds) for k, fn in calls.items()}
            render = float(np.median(ms["ht_render_depth_dev 320x240"]))
            for k, v in ms.items():
                med = float(np.median(v))
                row = {"call": k, "frames": B, "ms": round(med, 5), "spread_ms": round(max(v) - min(v), 5), "series_ms": [round(x, 5) for x in v], "us_per_frame": round(med * 1e3 / B, 4),
                       "frames_per_s": round(B / med * 1e3)}
                if "render" not in k:
                    row["of_render"] = round(med / render, 5); row["within_bar"] = bool(med <= BAR * render)
                    ok = ok and row["within_bar"]
                res["rows"].append(row); print(json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out, "within_bar": ok}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
