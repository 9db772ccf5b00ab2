"""What self-calibration from a tracked hand is worth: the bench's 1024 ground truths at 320x240, drawn by ht_raster_mesh_depth_dev from the bench
camera and from ONE fixed second camera (a rig) at 90 and at 180 degrees about the vertical through the mean palm; start poses one frame stale.  ht_update_views_dev
with three fused passes in three legs, each from the same start:

 (a) with the true extrinsics
 (b) with the extrinsics off by 5 degrees about (1,1,0)/sqrt 2 and 20 mm -- the number DESIGN section 37 never had
 (c) with the extrinsics ht_calibrate_view_dev (HT_CALIB_RIG, the defaults) finds from that guess and the poses a single-view update (ht_update_frames_dev) left in
     the slots: what a user has, not the ground truth

Reported: the mean SKELETON keypoint error over all keypoints and over those hidden in view 0 for each leg, and the rigid error of T (the mean distance between where
it and the true transform put the view's points, over the first 32 frames' clouds) for the guess, for (c)'s T, and for the T the same call finds from the ground-truth
poses.  No bar is set.  Writes profiles/r29_calib_accuracy.json (or --out)."""
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
import joints_inputs as ji  # noqa: E402
import kpfit_ref as kr  # noqa: E402
import views_ref as vr  # noqa: E402
from hand_tracking_samples_amd import native, weights as W  # noqa: E402

B, WD, HT = BM.B, 320, 240
PERTURB = (5.0, 0.02)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_calib_accuracy.json"))
    a = ap.parse_args()
    truth = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))["gtpose"].astype(np.float32)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev); st = s.cuda_stream
    m = ji.model("hand17")
    ctx = native.Context(BM.M17, B)
    res = {"device": torch.cuda.get_device_name(0), "frames": B, "frame": "%dx%d" % (WD, HT), "fused_passes": a.passes, "start_pose": "the ground truth of frame i + 1 (one frame stale)",
           "guess": "the true extrinsics turned by %g degrees about (1,1,0)/sqrt 2 through the camera's position and shifted by %g m" % PERTURB,
           "hidden": "keypoints of the ground truth that ht_keypoints does not report visible (0) against view 0's frame"}
    try:
        ctx.load_weights(W.make_cnnb())
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        cam0 = vr.frame_camera(WD, HT); cams0 = np.tile(cam0, (B, 1))
        stale = np.zeros((B, m.nb, 13), np.float32); stale[:, :, :7] = np.roll(truth, -1, axis=0)
        start = kr.user_poses(m, stale)
        with torch.cuda.stream(s):
            d_truth = torch.from_numpy(truth).to(dev); d_cams0 = torch.from_numpy(cams0).to(dev); d_start = torch.from_numpy(start).to(dev)
            d_v0 = torch.empty((B, HT, WD), dtype=torch.int16, device=dev); d_out = torch.empty((B, m.nb, 7), dtype=torch.float32, device=dev)
            d_T = torch.zeros(7, dtype=torch.float32, device=dev)
        ctx.raster_mesh_depth_dev(d_truth.data_ptr(), d_cams0.data_ptr(), WD, HT, 4.0, 0.5, B, d_v0.data_ptr(), stream=st)
        s.synchronize()
        v0 = d_v0.cpu().numpy().view(np.uint16)
        want = ctx.keypoints(truth, native.KP_SKELETON, com_poses=True, cams=cams0, depth=v0)
        hidden = want["vis"] != 0
        res["keypoints"] = int(hidden.shape[1]); res["hidden_share"] = round(float(hidden.mean()), 4)
        vopt = ctx.views_default(); copt = ctx.calib_default()
        d_stats = torch.zeros((copt.iterations + 1, native.CALIB_STATS), dtype=torch.float64, device=dev)

        def errors(poses):
            e = ctx.keypoint_errors(ctx.keypoints(poses, native.KP_SKELETON)["xyz"], want["xyz"])
            return {"mean_all_mm": round(1e3 * float(e["dist"].mean()), 4), "mean_hidden_mm": round(1e3 * float(e["dist"][hidden].mean()), 4), "finite": bool(np.isfinite(poses).all())}

        res["start"] = errors(start)
        for degrees in (90.0, 180.0):
            cam1 = vr.orbit(cam0, truth[:, 0, :3].astype(np.float64).mean(0), degrees)
            guess = cr.perturbed(cam1, *PERTURB)
            local = np.stack([vr.into_camera(p, cam1) for p in truth])
            with torch.cuda.stream(s):
                d_local = torch.from_numpy(local).to(dev); d_v1 = torch.empty_like(d_v0)
            ctx.raster_mesh_depth_dev(d_local.data_ptr(), d_cams0.data_ptr(), WD, HT, 4.0, 0.5, B, d_v1.data_ptr(), stream=st)
            with torch.cuda.stream(s):
                d_depth = torch.stack([d_v0, d_v1], dim=1).contiguous()
                d_guess = torch.from_numpy(np.tile(guess, (B, 1))).to(dev)
            s.synchronize()
            v1 = d_v1.cpu().numpy().view(np.uint16)
            pts = np.concatenate([cr.cloud(v1[b], cam1, dict(range_lo=copt.range_lo, range_hi=copt.range_hi, fraction=copt.fraction)) for b in range(32)])
            true_T = cam1[5:12].astype(np.float64)
            out = {"second_view_points_mean": None}

            def fused(cam):
                with torch.cuda.stream(s):
                    d_cams = torch.from_numpy(np.ascontiguousarray(np.stack([cams0, np.tile(cam.astype(np.float32), (B, 1))], axis=1))).to(dev)
                ctx.update_views_dev(64, d_depth.data_ptr(), d_cams.data_ptr(), WD, HT, 2, 0.17, d_start.data_ptr(), B, d_out.data_ptr(), options=vopt, passes=a.passes, stream=st); s.synchronize()
                return errors(d_out.cpu().numpy())

            def calibrated(d_poses):
                ctx.calibrate_view_dev(d_v1.data_ptr(), d_guess.data_ptr(), WD, HT, B, d_T.data_ptr(), d_stats.data_ptr(), d_poses=d_poses, which=0, options=copt, stream=st); s.synchronize()
                T = d_T.cpu().numpy(); st_ = d_stats.cpu().numpy()
                cam = cam1.copy(); cam[5:12] = T
                return cam, {"rigid_error_mm": round(1e3 * cr.rigid_error(T.astype(np.float64), true_T, pts), 4), "inliers": int(st_[-1, 0]), "points": int(st_[-1, 1]), "cost_first": float(st_[0, 2]),
                             "cost_last": float(st_[-1, 2]), "flags": [int(f) for f in st_[:, 5]]}

            out["a: true extrinsics"] = fused(cam1)
            out["b: extrinsics off by the guess's error"] = dict(fused(guess), rigid_error_mm=round(1e3 * cr.rigid_error(guess[5:12].astype(np.float64), true_T, pts), 4))
            _, from_truth = calibrated(d_truth.data_ptr())
            out["T from the ground-truth poses"] = from_truth
            ctx.update_frames_dev(d_v0.data_ptr(), d_cams0.data_ptr(), WD, HT, 0.17, d_start.data_ptr(), B, d_out.data_ptr(), st); s.synchronize()
            out["single-view update that leaves the poses"] = errors(d_out.cpu().numpy())
            cam_est, from_tracked = calibrated(None)
            out["T from the tracked poses in the slots"] = from_tracked
            out["second_view_points_mean"] = round(from_tracked["points"] / B, 1)
            out["c: extrinsics calibrated from the tracked poses"] = fused(cam_est)
            res["second camera at %d degrees" % degrees] = out
            print(json.dumps({degrees: out}), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
