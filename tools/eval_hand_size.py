"""What estimating the hand's size is worth: the bench's 1024 ground truths at 320x240, drawn by ht_raster_mesh_depth_dev from contexts scaled to
0.87, 1.0 and 1.15 (the poses stretched about the wrist as ht_scale stretches a state), seen by the bench camera.  Per size:

 (a) ht_estimate_scale (SHARED, the defaults) from the UNSTRETCHED true poses with each value of free_pose: the estimate where the tracking is perfect
 (b) the loop a user would run with an unscaled tracker and untrained weights: ht_update_frames_dev from poses one frame stale, ht_estimate_scale from the slots'
     state, ht_scale by the result, and again from the poses the update left, three rounds; s (the product of the rounds' factors) after each round and the mean
     SKELETON keypoint error against the scaled hand's own keypoints before the first round and after the last update
 (c) the same loop on the frames through ht_sensor_simulate's default DS4 noise behind RSCam::FilterDS4 (ht_sensor_filter)

Measures and sets no bar.  Writes profiles/r30_size_accuracy.json (or --out)."""
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
import joints_inputs as ji  # noqa: E402
import kpfit_ref as kr  # noqa: E402
import size_ref as sr  # noqa: E402
import views_ref as vr  # noqa: E402
from hand_tracking_samples_amd import native, weights as W  # noqa: E402

B, WD, HT = BM.B, 320, 240
ROUNDS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="0.87,1.0,1.15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_size_accuracy.json"))
    a = ap.parse_args()
    truth = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))["gtpose"].astype(np.float32)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev); st = s.cuda_stream
    m = ji.model("hand17")
    cam0 = vr.frame_camera(WD, HT); cams0 = np.tile(cam0, (B, 1))
    stale = np.zeros((B, m.nb, 13), np.float32); stale[:, :, :7] = np.roll(truth, -1, axis=0)
    start = kr.user_poses(m, stale)
    weights = W.make_cnnb()
    res = {"device": torch.cuda.get_device_name(0), "frames": B, "frame": "%dx%d" % (WD, HT), "rounds": ROUNDS, "weights": "untrained (weights.make_cnnb)",
           "start_pose": "the unscaled model at the ground truth of frame i + 1 (one frame stale)"}
    for size in (float(x) for x in a.sizes.split(",")):
        out = {}
        # the frames and the scaled hand's keypoints, from a context scaled to `size`
        rc = native.Context(BM.M17, 1)
        try:
            if size != 1.0:
                rc.scale(size)
            shown = sr.stretched(truth, size) if size != 1.0 else truth
            clean = rc.raster_mesh_depth(shown, cams0, WD, HT, 4.0, 0.5)
            want = rc.keypoints(shown, native.KP_SKELETON, com_poses=True)["xyz"]
            noise = native.sensor_noise_default(native.SENSOR_DS4)
            raw, ir = rc.sensor_simulate(native.SENSOR_DS4, clean, noise)
            noisy, ncams = rc.sensor_filter(native.SENSOR_DS4, raw, cams0, ir=ir)
        finally:
            rc.close()
        out["filtered_frame"] = "%dx%d" % (noisy.shape[2], noisy.shape[1])
        # (a) from the unstretched true poses
        ctx = native.Context(BM.M17, B)
        try:
            for fp in (0, 1):
                sc, T, stt = ctx.estimate_scale(clean, cams0, truth, 0, ctx.size_default(free_pose=fp))
                out["a: from the true poses, free_pose %d" % fp] = {"s": round(float(sc[0]), 5), "error": round(float(sc[0]) - size, 5), "cost_first": float(stt[0, 2]), "cost_last": float(stt[-1, 2]),
                                                                    "inliers": int(stt[-1, 0]), "points": int(stt[-1, 1]), "flags": [int(f) for f in stt[:, 5]]}
        finally:
            ctx.close()
        # (b), (c) the user's loop on clean and on filtered noisy frames
        for tag, frames, cams in (("b: tracked, clean frames", clean, cams0), ("c: tracked, DS4 noise behind FilterDS4", noisy, ncams)):
            ctx = native.Context(BM.M17, B)
            try:
                ctx.load_weights(weights)
                ctx.set_params(microforce=3.0, mainthreadpasses=3)
                h, w = frames.shape[1:]
                with torch.cuda.stream(s):
                    d_frames = torch.from_numpy(np.ascontiguousarray(frames).view(np.int16)).to(dev); d_cams = torch.from_numpy(np.ascontiguousarray(cams, np.float32)).to(dev)
                    d_start = torch.from_numpy(start).to(dev); d_out = torch.empty((B, m.nb, 7), dtype=torch.float32, device=dev)
                s.synchronize()

                def error(poses):
                    return round(1e3 * float(ctx.keypoint_errors(ctx.keypoints(poses, native.KP_SKELETON)["xyz"], want)["dist"].mean()), 4)

                def update():
                    ctx.update_frames_dev(d_frames.data_ptr(), d_cams.data_ptr(), w, h, 0.17, d_start.data_ptr(), B, d_out.data_ptr(), st); s.synchronize()
                    return d_out.cpu().numpy()
                row = {"keypoint_error_mm, start": error(start), "s_after_round": [], "factor_of_round": [], "flags": []}
                poses = update()
                row["keypoint_error_mm, first update (unscaled model)"] = error(poses)
                total = 1.0
                for rnd in range(ROUNDS):
                    sc, T, stt = ctx.estimate_scale(frames, cams, None, 0, ctx.size_default())
                    f = float(sc[0]); total *= f
                    row["s_after_round"].append(round(total, 5)); row["factor_of_round"].append(round(f, 5)); row["flags"].append(int(stt[:, 5].max()))
                    ctx.scale(f)
                    with torch.cuda.stream(s):
                        d_start.copy_(d_out)
                    s.synchronize()
                    poses = update()
                row["error_of_s"] = round(total - size, 5)
                row["keypoint_error_mm, last update"] = error(poses); row["finite"] = bool(np.isfinite(poses).all())
                out[tag] = row
            finally:
                ctx.close()
        res["hand of size %g" % size] = out
        print(json.dumps({size: out}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
