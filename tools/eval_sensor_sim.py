"""The accuracy table under sensor noise: the bench ground-truth poses rendered at 640x480 for an SR300 (Ivy) and at 320x240 for an R200 (DS4),
made raw by ht_sensor_simulate_dev under ht_sensor_noise_default's figures, filtered by the camera's own filter (ht_sensor_filter_dev) and tracked from the bench
start poses (ht_update_frames_sized_dev with the 64x64 net at 640x480, ht_update_frames_dev at 320x240), all on one stream; then measured on the device against the
ground truths as tools/eval_tracking.py measures (ht_keypoints, ht_keypoint_errors, ht_pose_depth_residual against the CLEAN frame).  Beside each row the same
pipeline on the clean frames: every front-end stage is the same call, only the simulation is left out (the clean R200 path gets a uniformly bright IR image).

For the R200 it also records how many of the simulator's flying pixels FilterDS4 removes.  A flying pixel is known on the device without a mask: it is a pixel
whose output changes when p_edge_fly alone is set to 0 (same seed, so every other decision is the same).

The noise figures were never measured against a camera; these are recorded figures of a model, not bars.  Writes profiles/r22_sensor_accuracy.json (or --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand_tracking_samples_amd import native, weights as W  # noqa: E402
import eval_tracking as E  # noqa: E402

M17 = os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand17.htfx")


def run(ctx, kind, clean, cams, start, noise, stream):
    """simulate (or not: noise None) -> filter -> update on one stream -> (tracked poses, raw frames on the device or None, filtered frames on the device)"""
    B, h, w = clean.shape
    dev = torch.device("cuda:0")
    with torch.cuda.stream(stream):
        tclean = torch.from_numpy(clean.view(np.int16)).to(dev); tc = torch.from_numpy(cams).to(dev); ts = torch.from_numpy(start).to(dev)
        traw = torch.empty((B, h, w), dtype=torch.int16, device=dev); tir = torch.full((B, h, w), 120, dtype=torch.uint8, device=dev)
        tf = torch.empty((B, h, w), dtype=torch.int16, device=dev); tco = torch.empty((B, 12), dtype=torch.float32, device=dev); out = torch.empty((B, ctx.nb, 7), dtype=torch.float32, device=dev)
    stream.synchronize()
    src = tclean
    if noise is not None:
        ctx.sensor_simulate_dev(kind, tclean.data_ptr(), w, h, B, noise, traw.data_ptr(), tir.data_ptr() if kind == native.SENSOR_DS4 else None, stream.cuda_stream)
        src = traw
    ctx.sensor_filter_dev(kind, src.data_ptr(), tir.data_ptr() if kind == native.SENSOR_DS4 else None, tc.data_ptr(), w, h, B, w, None, tf.data_ptr(), tco.data_ptr(), stream.cuda_stream)
    if kind == native.SENSOR_IVY:
        ctx.update_frames_sized_dev(64, tf.data_ptr(), tco.data_ptr(), w, h, 0.17, ts.data_ptr(), B, out.data_ptr(), stream.cuda_stream)
    else:
        ctx.update_frames_dev(tf.data_ptr(), tco.data_ptr(), w, h, 0.17, ts.data_ptr(), B, out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy(), (traw if noise is not None else None), tf, tclean, tir


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_sensor_accuracy.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    B = a.frames
    gt, start = z["gtpose"][:B].astype(np.float32), z["startpose"][:B].astype(np.float32)
    if a.weights and os.path.exists(a.weights):
        w64, which = W.load_cnnb(a.weights), "trained weights from " + os.path.basename(a.weights)
    else:
        w64, which = W.make_cnnb(), "the generator's seeded weights (untrained: the CNN-driven branch proposes noise)"
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    res = {"frames": B, "weights": which, "seed": a.seed, "note": "noise figures: ht_sensor_noise_default, reasoned from data sheets, never measured against a camera", "kinds": {}}
    ctx = native.Context(M17, B)
    try:
        ctx.load_weights(w64); ctx.set_params(microforce=3.0, mainthreadpasses=3)
        for name, kind, w, h in (("ivy", native.SENSOR_IVY, 640, 480), ("ds4", native.SENSOR_DS4, 320, 240)):
            cams = np.zeros((B, 12), np.float32); cams[:, :5] = [305 * w / 320, 305 * w / 320, w / 2, h / 2, 0.001]; cams[:, 11] = 1
            clean = ctx.render_depth(gt, cams, w, h)
            noise = native.sensor_noise_default(kind, 0.001, 4.0, seed=a.seed)
            entry = {"frame": [w, h], "noise": {k: getattr(noise, k) for k, _ in noise._fields_}, "start_poses": E.measure(ctx, start, True, gt, cams, clean)}
            for label, nz in (("clean", None), ("simulated", noise)):
                tracked, traw, tf, tclean, tir = run(ctx, kind, clean, cams, start, nz, stream)
                entry[label] = E.measure(ctx, tracked, False, gt, cams, clean)
                if nz is not None:
                    raw = traw.cpu().numpy().view(np.uint16)
                    fg = clean < noise.far_count
                    entry["raw_frames"] = {"foreground_pixels": int(fg.sum()), "dropped_share_of_foreground": round(float((raw[fg] == 0).mean()), 5),
                                           "mean_abs_change_of_kept_pixels_counts": round(float(np.abs(raw[fg & (raw != 0)].astype(np.int64) - clean[fg & (raw != 0)].astype(np.int64)).mean()), 4)}
                    if kind == native.SENSOR_DS4:      # the flying pixels: what changes when p_edge_fly alone is 0
                        tnofly = torch.empty_like(traw); tir2 = torch.empty_like(tir)
                        ctx.sensor_simulate_dev(kind, tclean.data_ptr(), w, h, B, noise.but(p_edge_fly=0), tnofly.data_ptr(), tir2.data_ptr(), stream.cuda_stream)
                        stream.synchronize()
                        with torch.cuda.stream(stream):
                            flying = (traw != tnofly) & (traw != 0)
                            kept = tf != 4096
                            n_fly = int(flying.sum()); gone = int((flying & ~kept).sum())
                            others = (traw != 0) & ~flying & torch.from_numpy(fg).to(traw.device)
                            n_other = int(others.sum()); other_gone = int((others & ~kept).sum())
                        entry["filter_ds4"] = {"flying_pixels": n_fly, "flying_removed": gone, "flying_removed_share": round(gone / max(n_fly, 1), 5),
                                               "other_hand_pixels": n_other, "other_removed_share": round(other_gone / max(n_other, 1), 5)}
                del traw, tf, tclean, tir
            res["kinds"][name] = entry
            del clean
            torch.cuda.empty_cache()
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("| camera | frames | table | mean error mm | frames within 5 / 10 / 20 / 40 mm | IoU | mean residual mm |")
    print("|---|---|---|---|---|---|---|")
    for name, e in res["kinds"].items():
        for label in ("start_poses", "clean", "simulated"):
            for table, _ in E.TABLES:
                r, d = e[label][table], e[label]["depth"]
                print("| %s %dx%d | %s | %s | %.3f | %s | %.3f | %.2f |" % (name, e["frame"][0], e["frame"][1], label.replace("_", " "), table, r["mean_error_mm"],
                                                                      " / ".join("%.1f %%" % (100 * v) for v in r["frames_within"].values()), d["mean_iou"], d["mean_abs_residual_mm"]))
    if "filter_ds4" in res["kinds"].get("ds4", {}):
        print(json.dumps(res["kinds"]["ds4"]["filter_ds4"]))
    print(json.dumps({"out": a.out, "weights": which}))


if __name__ == "__main__":
    main()
