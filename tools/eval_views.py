"""What a second view is worth: the bench's 1024 ground truths at 320x240, drawn by ht_raster_mesh_depth_dev from the bench camera and from a second
camera at 90 and at 180 degrees about the vertical through the palm, at the same distance; start poses one frame stale.  Three legs in one run, each from the same start:

 (a) ht_update_frames_dev alone
 (b) ht_update_views_dev with both views and three fused passes
 (c) leg (a) plus three more single-view passes (ht_update_views_dev with view 0 alone), so that the extra passes alone are not credited to the second view

Reported: the mean SKELETON keypoint error over all keypoints, and over those ht_keypoints reports hidden in view 0 (anything but "visible" for the ground truth's
keypoint against view 0's frame).  No bar is set.  Writes profiles/r28_views_accuracy.json (or --out)."""
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
import views_ref as vr  # noqa: E402
from hand_tracking_samples_amd import native, weights as W  # noqa: E402

B, WD, HT = BM.B, 320, 240


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_views_accuracy.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    truth = z["gtpose"].astype(np.float32)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev); st = s.cuda_stream
    m = ji.model("hand17")
    ctx = native.Context(BM.M17, B)
    res = {"device": torch.cuda.get_device_name(0), "frames": B, "frame": "%dx%d" % (WD, HT), "fused_passes": a.passes, "start_pose": "the ground truth of frame i + 1 (one frame stale)",
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
        ctx.raster_mesh_depth_dev(d_truth.data_ptr(), d_cams0.data_ptr(), WD, HT, 4.0, 0.5, B, d_v0.data_ptr(), stream=st)
        s.synchronize()
        v0 = d_v0.cpu().numpy().view(np.uint16)
        want = ctx.keypoints(truth, native.KP_SKELETON, com_poses=True, cams=cams0, depth=v0)
        hidden = want["vis"] != 0
        res["keypoints"] = int(hidden.shape[1]); res["hidden_share"] = round(float(hidden.mean()), 4)
        opt = ctx.views_default()

        def errors(poses):
            e = ctx.keypoint_errors(ctx.keypoints(poses, native.KP_SKELETON)["xyz"], want["xyz"])
            return {"mean_all_mm": round(1e3 * float(e["dist"].mean()), 4), "mean_hidden_mm": round(1e3 * float(e["dist"][hidden].mean()), 4), "finite": bool(np.isfinite(poses).all())}

        res["start"] = errors(start)
        ctx.update_frames_dev(d_v0.data_ptr(), d_cams0.data_ptr(), WD, HT, 0.17, d_start.data_ptr(), B, d_out.data_ptr(), st); s.synchronize()
        res["a: ht_update_frames_dev alone"] = errors(d_out.cpu().numpy())
        print(json.dumps(res["a: ht_update_frames_dev alone"]), flush=True)
        ctx.update_views_dev(64, d_v0.data_ptr(), d_cams0.data_ptr(), WD, HT, 1, 0.17, d_start.data_ptr(), B, d_out.data_ptr(), options=opt, passes=a.passes, stream=st); s.synchronize()
        res["c: a plus %d more single-view passes" % a.passes] = errors(d_out.cpu().numpy())
        print(json.dumps(res["c: a plus %d more single-view passes" % a.passes]), flush=True)
        for degrees in (90.0, 180.0):
            cams1 = np.stack([vr.orbit(cam0, vr.palm(truth[i]), degrees) for i in range(B)])
            local = np.stack([vr.into_camera(truth[i], cams1[i]) for i in range(B)])
            with torch.cuda.stream(s):
                d_local = torch.from_numpy(local).to(dev); d_v1 = torch.empty_like(d_v0)
            ctx.raster_mesh_depth_dev(d_local.data_ptr(), d_cams0.data_ptr(), WD, HT, 4.0, 0.5, B, d_v1.data_ptr(), stream=st)
            with torch.cuda.stream(s):
                d_depth = torch.stack([d_v0, d_v1], dim=1).contiguous(); d_cams = torch.from_numpy(np.ascontiguousarray(np.stack([cams0, cams1], axis=1))).to(dev)
            ctx.update_views_dev(64, d_depth.data_ptr(), d_cams.data_ptr(), WD, HT, 2, 0.17, d_start.data_ptr(), B, d_out.data_ptr(), options=opt, passes=a.passes, stream=st); s.synchronize()
            key = "b: ht_update_views_dev, second camera at %d degrees, %d fused passes" % (degrees, a.passes)
            res[key] = errors(d_out.cpu().numpy())
            print(json.dumps({key: res[key]}), flush=True)
        c = res["c: a plus %d more single-view passes" % a.passes]
        res["b_beats_c_on_hidden_keypoints"] = {k: bool(v["mean_hidden_mm"] < c["mean_hidden_mm"]) for k, v in res.items() if k.startswith("b: ")}
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out, "b_beats_c_on_hidden_keypoints": res["b_beats_c_on_hidden_keypoints"]}))


if __name__ == "__main__":
    main()
