"""Times the accuracy layer on 1024 resident frames with device events, every shape warmed first, each figure the median of --rounds series with
the series' spread (max - min), the compared calls' series taking turns (the protocol of tools/bench_mirror.py, whose helpers this uses):

 (a) ht_depth_compare_dev on 1024 frame pairs of 320x240 and of 640x480 (the bench hands rendered at their ground truths and at their start poses), beside a
     device-to-device hipMemcpyAsync of one batch's n bytes: the copy reads n and writes n, the kernel reads 2 n.  Bar: 1.5 times the copy.  The fraction of the
     HBM peak is stated as measured.
 (b) ht_keypoints_dev with visibility followed by ht_keypoint_errors_dev on 1024 frames, beside ht_update_dev of the same 1024 bench tiles in the same run.
     Bar: DESIGN section 17's for a stage beside another, at most 0.25 of it.  ht_joint_coords_dev is printed next to it for scale.
 (c) ht_pose_depth_residual_dev on 1024 frames of 320x240 beside ht_render_depth_dev alone plus ht_depth_compare_dev alone.  Bar: their sum plus twice the larger spread.
 (d) bench.py's default run of this commit against the parent's is two processes taking turns (python bench.py ..., and HT_LIB_PATH=<the parent's library> python bench.py ...)
     and not part of this tool.

Exits 1 when a bar is missed.  Writes profiles/r21_quality.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_mirror as BM  # noqa: E402
from hand_tracking_samples_amd import build as hb, native, weights as W  # noqa: E402

B = BM.B
LO, HI, TOL = 1, 650, 10
THR = np.array([0.005, 0.01, 0.02, 0.04], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--update-steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_quality.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    st = s.cuda_stream
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int
    ctx = native.Context(BM.M17, B)
    names = ("k_keypoints", "k_kp_errors", "k_depth_compare", "k_pose_to_render")
    res = {"device": torch.cuda.get_device_name(0), "frames": B, "steps": a.steps, "update_steps": a.update_steps, "rounds": a.rounds,
           "resources": {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "LDS Size", "Occupancy") if q in v} for k, v in hb.resource_usage().items() if any(n in k for n in names)}}
    ok = True
    try:
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        gt, start = z["gtpose"].astype(np.float32), z["startpose"].astype(np.float32)
        cam = {(640, 480): np.zeros((B, 12), np.float32)}
        cam[(640, 480)][:, :5] = [610, 610, 320, 240, 0.001]; cam[(640, 480)][:, 11] = 1
        cam[(320, 240)] = cam[(640, 480)].copy(); cam[(320, 240)][:, :4] /= 2
        with torch.cuda.stream(s):
            ta = {wh: torch.from_numpy(ctx.render_depth(gt, cam[wh], wh[0], wh[1]).view(np.int16)).to(dev) for wh in cam}
            tb = {wh: torch.from_numpy(ctx.render_depth(start, cam[wh], wh[0], wh[1]).view(np.int16)).to(dev) for wh in cam}
            tc = {wh: torch.from_numpy(cam[wh]).to(dev) for wh in cam}
            info = torch.empty((B, 8), dtype=torch.int64, device=dev)
        s.synchronize()
        # (a) the comparison kernel beside a device-to-device copy of one batch's bytes
        res["depth_compare"] = []
        for wh in ((320, 240), (640, 480)):
            nbytes = B * wh[0] * wh[1] * 2
            to = torch.empty_like(ta[wh])
            fns = {"ht_depth_compare_dev": lambda wh=wh: ctx.depth_compare_dev(ta[wh].data_ptr(), tb[wh].data_ptr(), wh[0], wh[1], B, LO, HI, TOL, info.data_ptr(), st),
                   "hipMemcpyAsync": lambda wh=wh, nbytes=nbytes, to=to: hip.hipMemcpyAsync(to.data_ptr(), ta[wh].data_ptr(), nbytes, 3, st)}
            for fn in fns.values():
                fn()
            s.synchronize()
            i0 = info.cpu().numpy()
            ms = BM.interleaved(fns, s, a.steps, a.warmup, a.rounds)
            k, c = BM.stat(ms["ht_depth_compare_dev"]), BM.stat(ms["hipMemcpyAsync"])
            row = {"frame": "%dx%d" % wh, "bytes_read": 2 * nbytes, "kernel": k, "copy_of_n_bytes": c, "kernel_TBps": round(2 * nbytes / k["ms"] / 1e9, 3), "copy_TBps_both_ways": round(2 * nbytes / c["ms"] / 1e9, 3),
                   "kernel_of_hbm_peak": round(2 * nbytes / (k["ms"] * 1e-3) / BM.HBM_PEAK, 4), "kernel_over_copy": round(k["ms"] / c["ms"], 4), "within_bar": bool(k["ms"] <= 1.5 * c["ms"]),
                   "mean_iou_start_against_gt": round(float(np.mean(i0[:, 2] / np.maximum(i0[:, 0] + i0[:, 1] - i0[:, 2], 1))), 4)}
            ok = ok and row["within_bar"]
            res["depth_compare"].append(row); print(json.dumps(row), flush=True)
            del to
        # (b) keypoints with visibility, then errors, beside the update of the same frames
        w64 = W.make_cnnb()
        ctx.load_weights(w64)
        K = len(ctx.keypoint_table(native.KP_FEATURE8)[0])
        with torch.cuda.stream(s):
            tiles = torch.from_numpy(z["depth"].view(np.int16)).to(dev); tcam = torch.from_numpy(z["cam"].astype(np.float32)).to(dev)
            ts = torch.from_numpy(start).to(dev); tg = torch.from_numpy(gt).to(dev); out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev)
            xyz = torch.empty((B, K, 3), dtype=torch.float32, device=dev); xyz_gt = torch.empty_like(xyz); pix = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
            zc = torch.empty((B, K), dtype=torch.float32, device=dev); vis = torch.empty((B, K), dtype=torch.uint8, device=dev)
            dist = torch.empty((B, K), dtype=torch.float32, device=dev); frame = torch.empty((B, 2), dtype=torch.float32, device=dev)
            sum_kp = torch.empty(K, dtype=torch.float64, device=dev); hk = torch.empty(len(THR), dtype=torch.int64, device=dev); hf = torch.empty(len(THR), dtype=torch.int64, device=dev)
            coords = torch.empty((B, ctx.nj, 3), dtype=torch.float32, device=dev)
        s.synchronize()
        ctx.keypoints_dev(tg.data_ptr(), B, native.KP_FEATURE8, xyz_gt.data_ptr(), com_poses=True, stream=st)

        def measure():
            ctx.keypoints_dev(out.data_ptr(), B, native.KP_FEATURE8, xyz.data_ptr(), pix.data_ptr(), zc.data_ptr(), vis.data_ptr(), d_cams=tcam.data_ptr(), d_depth=tiles.data_ptr(), w=64, h=64, stream=st)
            ctx.keypoint_errors_dev(xyz.data_ptr(), xyz_gt.data_ptr(), B, K, THR, dist.data_ptr(), frame.data_ptr(), sum_kp.data_ptr(), hk.data_ptr(), hf.data_ptr(), st)

        fns = {"update": lambda: ctx.update_dev(tiles.data_ptr(), tcam.data_ptr(), ts.data_ptr(), B, out.data_ptr(), st), "keypoints + errors": measure,
               "joint_coords": lambda: ctx.joint_coords_dev(out.data_ptr(), B, coords.data_ptr(), stream=st)}
        for fn in fns.values():
            fn()
        s.synchronize()
        ms = BM.interleaved({"update": fns["update"]}, s, a.update_steps, 1, a.rounds)
        ms.update(BM.interleaved({k: fns[k] for k in ("keypoints + errors", "joint_coords")}, s, a.steps, a.warmup, a.rounds))
        u, q, j = BM.stat(ms["update"]), BM.stat(ms["keypoints + errors"]), BM.stat(ms["joint_coords"])
        row = {"ht_update_dev, 1024 bench tiles, re-seeded every call": u, "ht_keypoints_dev with visibility + ht_keypoint_errors_dev": q, "ht_joint_coords_dev": j,
               "measure_of_update": round(q["ms"] / u["ms"], 5), "within_bar": bool(q["ms"] <= 0.25 * u["ms"]), "mean_keypoint_error_m": float(sum_kp.cpu().numpy().sum() / (B * K)),
               "frames_under_thr": dict(zip(("5mm", "10mm", "20mm", "40mm"), hf.cpu().numpy().tolist()))}
        ok = ok and row["within_bar"]
        res["keypoints_and_errors"] = row; print(json.dumps(row), flush=True)
        # (c) the composite beside its two parts
        wh = (320, 240)
        with torch.cuda.stream(s):
            rend = torch.empty_like(ta[wh])
        fns = {"ht_pose_depth_residual_dev": lambda: ctx.pose_depth_residual_dev(ts.data_ptr(), tc[wh].data_ptr(), ta[wh].data_ptr(), wh[0], wh[1], B, LO, HI, TOL, info.data_ptr(), None, com_poses=True, stream=st),
               "ht_render_depth_dev": lambda: ctx.render_depth_dev(ts.data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], 4.0, B, rend.data_ptr(), None, st),
               "ht_depth_compare_dev": lambda: ctx.depth_compare_dev(ta[wh].data_ptr(), rend.data_ptr(), wh[0], wh[1], B, LO, HI, TOL, info.data_ptr(), st)}
        for fn in fns.values():
            fn()
        s.synchronize()
        i_parts = info.cpu().numpy().copy()
        fns["ht_pose_depth_residual_dev"](); s.synchronize()
        same = bool(np.array_equal(info.cpu().numpy(), i_parts))
        ms = BM.interleaved(fns, s, a.steps, a.warmup, a.rounds)
        p, r, c = BM.stat(ms["ht_pose_depth_residual_dev"]), BM.stat(ms["ht_render_depth_dev"]), BM.stat(ms["ht_depth_compare_dev"])
        row = {"frame": "320x240", "composite": p, "render": r, "compare": c, "sum_of_parts_ms": round(r["ms"] + c["ms"], 5), "over_ms": round(p["ms"] - r["ms"] - c["ms"], 5), "same_info_as_the_parts": same,
               "within_bar": bool(p["ms"] <= r["ms"] + c["ms"] + 2 * max(r["spread_ms"], c["spread_ms"])) and same}
        ok = ok and row["within_bar"]
        res["pose_depth_residual"] = row; print(json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out, "within_bars": ok}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
