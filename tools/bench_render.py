"""Device renderer (ht_render_depth_dev, csrc/ht_render.hip): frames/s by size, model and batch, the empty-frame floor, and the closed loop
render -> ht_update_frames_dev at 1024 frames with a new batch of poses every step.  Writes profiles/r07_render.json (or --out).

    python tools/bench_render.py [--steps 20] [--warmup 3] [--out profiles/r07_render.json] [--quick]
    python tools/bench_render.py --mesh      the mesh ray cast beside the hulls (profiles/r08_render_mesh.json)
    python tools/bench_render.py --raster    the mesh rasteriser beside the ray cast, the hulls and the tracking step (profiles/r26_raster_mesh.json)
    python tools/bench_render.py --scene     the scene call beside its composition from tested calls, the two-hand update and the one-hand rasteriser (profiles/r27_raster_scene.json)

Hands: the bench recording's ground truths (bench_data/frames1024.npz, 17 bones) and the 26-bone start poses of bench_data/frames5_256.npz, seen
through the application's 320x240 camera (focal 305) or a 128x128 one (focal 163).  Empty frames: the same hands moved 10 m behind the camera."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand_tracking_samples_amd import build as hb, native, weights as W  # noqa: E402

M17 = os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand17.htfx")
M26 = os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand26.htfx")
CAMS = {(320, 240): [305, 305, 160, 120], (128, 128): [163, 163, 64, 64], (640, 480): [610, 610, 320, 240]}


def cam_of(w, h, B):
    c = np.zeros((B, 12), np.float32); c[:, :4] = CAMS[(w, h)]; c[:, 4] = 0.001; c[:, 11] = 1
    return c


def time_it(fn, stream, steps, warmup):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def slerp(a, b, t):
    """[..., 4] quaternions, float64"""
    d = (a * b).sum(-1, keepdims=True)
    b = np.where(d < 0, -b, b); d = np.abs(d)
    th = np.arccos(np.clip(d, -1.0, 1.0))
    sn = np.sin(th)
    lin = d > 0.9995
    q = np.where(lin, a + (b - a) * t, (np.sin((1 - t) * th) * a + np.sin(t * th) * b) / np.where(lin, 1.0, sn))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def user_pos(poses, com):
    """RigidBody::PositionUser (physics.h:142): pose * -com, for comparing body poses with the tracker's GetPoseUser output"""
    x, y, z, w = (poses[..., 3 + i].astype(np.float64) for i in range(4))
    v = -com[None].astype(np.float64)
    m = [[w * w + x * x - y * y - z * z, 2 * (x * y - z * w), 2 * (z * x + y * w)], [2 * (x * y + z * w), w * w - x * x + y * y - z * z, 2 * (y * z - x * w)],
         [2 * (z * x - y * w), 2 * (y * z + x * w), w * w - x * x - y * y + z * z]]
    return poses[..., :3] + np.stack([m[r][0] * v[..., 0] + m[r][1] * v[..., 1] + m[r][2] * v[..., 2] for r in range(3)], -1)


def main_mesh(a):
    """--mesh: ht_render_mesh_depth_dev beside ht_render_depth_dev on the same poses in the same run, the no-body-in-view floor, and the same batch's tracking step"""
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s = torch.cuda.Stream(device=dev)
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    z5 = np.load(os.path.join(ROOT, "bench_data", "frames5_256.npz"))
    hands = {17: z["gtpose"], 26: z5["startpose"]}
    w, h = 320, 240
    res = {"device": torch.cuda.get_device_name(dev), "steps": a.steps, "warmup": a.warmup, "w": w, "h": h, "render": [], "usage": {}}
    for k, v in hb.resource_usage().items():
        if "render" in k:
            res["usage"][k] = {x: v.get(x) for x in ("VGPRs", "SGPRs", "AGPRs", "ScratchSize", "LDS Size", "Occupancy")}
    for nb, model in ((17, M17), (26, M26)):
        ctx = native.Context(model, 1024 if nb == 17 else 1)
        try:
            if nb == 17:
                ctx.load_weights(W.make_cnnb()); ctx.set_params(microforce=3.0, mainthreadpasses=3); ctx.reserve_points(w * h // 4)
            for B in ((1024,) if a.quick else (1024, 8192)):
                p = hands[nb][np.arange(B) % len(hands[nb])].copy()
                away = p.copy(); away[:, :, 2] -= 10.0
                tp = torch.from_numpy(p).to(dev); ta = torch.from_numpy(away).to(dev); tc = torch.from_numpy(cam_of(w, h, B)).to(dev)
                td = torch.empty((B, h, w), dtype=torch.int16, device=dev)
                row = {"bones": nb, "B": B}
                for name, off, far in (("mesh_off0_far4", 0.0, 4.0), ("mesh_off05_far085", 0.5, 0.85)):
                    row[name + "_ms"] = round(time_it(lambda: ctx.render_mesh_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, far, off, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup), 4)
                    row[name + "_hand_pixel_fraction"] = round(float((td[:64].cpu().numpy().view(np.uint16) < int(far * 1000) - 1).mean()), 4)
                row["mesh_empty_ms"] = round(time_it(lambda: ctx.render_mesh_depth_dev(ta.data_ptr(), tc.data_ptr(), w, h, 4.0, 0.0, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup), 4)
                row["hull_empty_ms"] = round(time_it(lambda: ctx.render_depth_dev(ta.data_ptr(), tc.data_ptr(), w, h, 4.0, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup), 4)
                row["hull_ms"] = round(time_it(lambda: ctx.render_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, 4.0, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup), 4)
                if nb == 17 and B == 1024:      # the tracking step these frames feed (hull frames, as section 17 measured it)
                    ts = torch.from_numpy(z["startpose"]).to(dev); out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev)
                    ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), w, h, 0.17, ts.data_ptr(), B, out.data_ptr(), s.cuda_stream)
                    s.synchronize()
                    row["update_frames_dev_ms"] = round(time_it(lambda: ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), w, h, 0.17, None, B, out.data_ptr(), s.cuda_stream), s, max(4, a.steps // 4), 1), 3)
                    row["mesh_over_update"] = round(row["mesh_off0_far4_ms"] / row["update_frames_dev_ms"], 4)
                row["mesh_over_hull"] = round(row["mesh_off0_far4_ms"] / row["hull_ms"], 3)
                print(json.dumps(row), flush=True)
                res["render"].append(row)
                del tp, ta, tc, td
        finally:
            ctx.close()
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "r08_render_mesh.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main_raster(a):
    """--raster: ht_raster_mesh_depth_dev beside ht_render_mesh_depth_dev and ht_render_depth_dev on the same poses in the same run, the none-in-view floor of each,
    and the same batch's tracking step (17 bones, 1024 frames of 320x240)"""
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s = torch.cuda.Stream(device=dev)
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    z5 = np.load(os.path.join(ROOT, "bench_data", "frames5_256.npz"))
    hands = {17: z["gtpose"], 26: z5["startpose"]}
    res = {"device": torch.cuda.get_device_name(dev), "steps": a.steps, "warmup": a.warmup, "render": [], "usage": {}}
    for k, v in hb.resource_usage().items():
        if "render" in k or "raster" in k:
            res["usage"][k] = {x: v.get(x) for x in ("VGPRs", "SGPRs", "AGPRs", "ScratchSize", "LDS Size", "Occupancy")}
    cases = ((320, 240, 1024),) if a.quick else ((320, 240, 1024), (320, 240, 8192), (640, 480, 1024))
    few = max(3, a.steps // 4)      # the ray cast and the tracking step take tens of milliseconds a call
    for nb, model in ((17, M17), (26, M26)):
        ctx = native.Context(model, 1024 if nb == 17 else 1)
        try:
            if nb == 17:
                ctx.load_weights(W.make_cnnb()); ctx.set_params(microforce=3.0, mainthreadpasses=3); ctx.reserve_points(320 * 240 // 4)
            for w, h, B in cases:
                p = hands[nb][np.arange(B) % len(hands[nb])].copy()
                away = p.copy(); away[:, :, 2] -= 10.0
                tp = torch.from_numpy(p).to(dev); ta = torch.from_numpy(away).to(dev); tc = torch.from_numpy(cam_of(w, h, B)).to(dev)
                td = torch.empty((B, h, w), dtype=torch.int16, device=dev)
                row = {"bones": nb, "w": w, "h": h, "B": B}
                for name, off, far in (("raster_off0_far4", 0.0, 4.0), ("raster_off05_far085", 0.5, 0.85)):
                    row[name + "_ms"] = round(time_it(lambda: ctx.raster_mesh_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, far, off, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup), 4)
                    row[name + "_hand_pixel_fraction"] = round(float((td[:64].cpu().numpy().view(np.uint16) < int(far * 1000) - 1).mean()), 4)
                row["raster_frames_per_s"] = round(B / row["raster_off0_far4_ms"] * 1e3, 1)
                row["raster_empty_ms"] = round(time_it(lambda: ctx.raster_mesh_depth_dev(ta.data_ptr(), tc.data_ptr(), w, h, 4.0, 0.0, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup), 4)
                row["mesh_ms"] = round(time_it(lambda: ctx.render_mesh_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, 4.0, 0.0, B, td.data_ptr(), None, s.cuda_stream), s, few, 1), 4)
                row["mesh_empty_ms"] = round(time_it(lambda: ctx.render_mesh_depth_dev(ta.data_ptr(), tc.data_ptr(), w, h, 4.0, 0.0, B, td.data_ptr(), None, s.cuda_stream), s, few, 1), 4)
                row["hull_empty_ms"] = round(time_it(lambda: ctx.render_depth_dev(ta.data_ptr(), tc.data_ptr(), w, h, 4.0, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup), 4)
                row["hull_ms"] = round(time_it(lambda: ctx.render_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, 4.0, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup), 4)
                if nb == 17 and B == 1024 and (w, h) == (320, 240):      # the tracking step these frames feed (hull frames, as section 17 measured it)
                    ts = torch.from_numpy(z["startpose"]).to(dev); out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev)
                    ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), w, h, 0.17, ts.data_ptr(), B, out.data_ptr(), s.cuda_stream)
                    s.synchronize()
                    row["update_frames_dev_ms"] = round(time_it(lambda: ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), w, h, 0.17, None, B, out.data_ptr(), s.cuda_stream), s, few, 1), 3)
                    row["raster_over_update"] = round(row["raster_off0_far4_ms"] / row["update_frames_dev_ms"], 4)
                row["raster_over_mesh"] = round(row["raster_off0_far4_ms"] / row["mesh_ms"], 4)
                row["raster_over_hull"] = round(row["raster_off0_far4_ms"] / row["hull_ms"], 3)
                print(json.dumps(row), flush=True)
                res["render"].append(row)
                del tp, ta, tc, td
        finally:
            ctx.close()
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "r26_raster_mesh.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")

def main_scene(a):
    """--scene: ht_raster_scene_depth_dev on scenes of one right and one left hand beside the same frames composed on the device from two ht_raster_mesh_depth_dev, the three
    mirror calls and a torch.minimum, on one stream; beside ht_update_two_hands_dev on the same scenes; and with one right hand beside ht_raster_mesh_depth_dev.  Resident
    batches, device events, every shape warmed, five series of each leg taken in turn within one run: the median and the spread (largest minus smallest) are reported."""
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s = torch.cuda.Stream(device=dev)
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    gt = z["gtpose"].astype(np.float32)
    res = {"device": torch.cuda.get_device_name(dev), "steps": a.steps, "warmup": a.warmup, "series": 5, "scenes": [], "usage": {}}
    for k, v in hb.resource_usage().items():
        if "raster" in k:
            res["usage"][k] = {x: v.get(x) for x in ("VGPRs", "SGPRs", "AGPRs", "ScratchSize", "LDS Size", "Occupancy")}

    def series(legs):
        """{name: (median, spread)} of five series, the legs in turn"""
        t = {n: [] for n in legs}
        for _ in range(5):
            for n, (fn, steps) in legs.items():
                t[n].append(time_it(fn, s, steps, 1))
        return {n: (float(np.median(v)), float(max(v) - min(v))) for n, v in t.items()}

    ctx = native.Context(M17, 1024)
    try:
        ctx.load_weights(W.make_cnnb()); ctx.set_params(microforce=3.0, mainthreadpasses=3); ctx.reserve_points(320 * 240 // 4)
        for w, h, B in (((320, 240, 512),) if a.quick else ((320, 240, 512), (320, 240, 1024), (640, 480, 512))):
            right = gt[np.arange(B) % len(gt)].copy(); right[:, :, 0] += 0.06
            left = gt[(np.arange(B) + 300) % len(gt)].copy(); left[:, :, 0] *= -1; left[:, :, 4:6] *= -1; left[:, :, 0] -= 0.06      # the mirror image of another hand, on the other side
            poses = np.stack([right, left], 1)
            tp = torch.from_numpy(poses).to(dev); tr = torch.from_numpy(right).to(dev); tl = torch.from_numpy(left).to(dev); tc = torch.from_numpy(cam_of(w, h, B)).to(dev)
            th = torch.from_numpy(np.tile(np.array([0, 1], np.uint8), (B, 1))).to(dev)
            td = torch.empty((B, h, w), dtype=torch.int16, device=dev); tha = torch.empty((B, h, w), dtype=torch.int8, device=dev); tb = torch.empty_like(tha); tv = torch.empty((B, 2), dtype=torch.int32, device=dev)
            ta, tm, tf, tout = (torch.empty_like(td) for _ in range(4)); tcan = torch.empty_like(tl); tmc = torch.empty_like(tc)

            def scene():
                ctx.raster_scene_depth_dev(tp.data_ptr(), th.data_ptr(), 2, tc.data_ptr(), w, h, 4.0, 0.0, B, None, td.data_ptr(), tha.data_ptr(), tb.data_ptr(), tv.data_ptr(), s.cuda_stream)

            def scene_depth_only():
                ctx.raster_scene_depth_dev(tp.data_ptr(), th.data_ptr(), 2, tc.data_ptr(), w, h, 4.0, 0.0, B, None, td.data_ptr(), None, None, None, s.cuda_stream)

            def composed():
                ctx.raster_mesh_depth_dev(tr.data_ptr(), tc.data_ptr(), w, h, 4.0, 0.0, B, ta.data_ptr(), None, s.cuda_stream)
                ctx.mirror_poses_dev(tl.data_ptr(), 17, B, None, tcan.data_ptr(), s.cuda_stream)
                ctx.mirror_cams_dev(tc.data_ptr(), w, B, None, tmc.data_ptr(), s.cuda_stream)
                ctx.raster_mesh_depth_dev(tcan.data_ptr(), tmc.data_ptr(), w, h, 4.0, 0.0, B, tm.data_ptr(), None, s.cuda_stream)
                ctx.mirror_frames_dev(tm.data_ptr(), w, h, B, None, tf.data_ptr(), s.cuda_stream)
                with torch.cuda.stream(s):
                    torch.minimum(ta, tf, out=tout)      # counts stay below 32768 here, so the signed minimum is the unsigned one

            def one_scene():
                ctx.raster_scene_depth_dev(tr.data_ptr(), None, 1, tc.data_ptr(), w, h, 4.0, 0.0, B, None, td.data_ptr(), None, None, None, s.cuda_stream)

            def one_mesh():
                ctx.raster_mesh_depth_dev(tr.data_ptr(), tc.data_ptr(), w, h, 4.0, 0.0, B, ta.data_ptr(), None, s.cuda_stream)

            s.wait_stream(torch.cuda.current_stream(dev))
            for fn in (scene, scene_depth_only, composed, one_scene, one_mesh):
                for _ in range(a.warmup):
                    fn()
            s.synchronize()
            scene(); composed(); s.synchronize()
            same = bool(torch.equal(td, tout))
            t = series({"scene": (scene, a.steps), "composed": (composed, a.steps), "scene_depth_only": (scene_depth_only, a.steps)})
            row = {"w": w, "h": h, "B": B, "hands": "one right, one left", "scene_equals_composition": same, "hand_pixel_fraction": round(float((tha[:64] >= 0).float().mean()), 4)}
            for n, (med, spread) in t.items():
                row[n + "_ms"] = round(med, 4); row[n + "_spread_ms"] = round(spread, 4)
            row["scene_minus_composed_ms"] = round(t["scene"][0] - t["composed"][0], 4)
            row["bar_not_slower_by_more_than_ms"] = round(2 * t["composed"][1], 4)
            row["bar_met"] = bool(t["scene"][0] - t["composed"][0] <= 2 * t["composed"][1])
            t1 = series({"one_scene": (one_scene, a.steps), "one_mesh": (one_mesh, a.steps)})
            row["one_right_hand_scene_ms"] = round(t1["one_scene"][0], 4); row["one_right_hand_scene_spread_ms"] = round(t1["one_scene"][1], 4)
            row["raster_mesh_ms"] = round(t1["one_mesh"][0], 4); row["raster_mesh_spread_ms"] = round(t1["one_mesh"][1], 4)
            row["one_hand_scene_over_raster_mesh"] = round(t1["one_scene"][0] / t1["one_mesh"][0], 4)
            if (w, h, B) == (320, 240, 512):      # the step these frames feed: the two-hand update of the same scenes, in the same run
                seeds = poses.reshape(2 * B, 17, 7).copy(); odd = np.arange(2 * B) % 2 == 1
                seeds[odd, :, 0] *= -1; seeds[odd, :, 4:6] *= -1      # a left slot is seeded with the canonical pose
                ctx.tracker_reset(seeds)
                out = torch.empty((2 * B, 17, 7), dtype=torch.float32, device=dev); info = torch.empty((B, 2, 8), dtype=torch.int32, device=dev)
                scene(); s.synchronize()

                def update():
                    ctx.update_two_hands_dev(64, td.data_ptr(), tc.data_ptr(), w, h, 0.17, 0, 650, 65535, 50, 3999, 0, None, B, out.data_ptr(), info.data_ptr(), s.cuda_stream)
                update(); s.synchronize()
                tu = series({"update": (update, max(3, a.steps // 4)), "scene": (scene, a.steps)})
                row["update_two_hands_dev_ms"] = round(tu["update"][0], 3); row["update_two_hands_dev_spread_ms"] = round(tu["update"][1], 3)
                row["both_hands_found_share"] = round(float((info[:, :, 0] > 0).float().mean()), 4)
                row["scene_over_update"] = round(tu["scene"][0] / tu["update"][0], 4); row["bar_scene_over_update"] = 0.25
            print(json.dumps(row), flush=True)
            res["scenes"].append(row)
            del tp, tr, tl, tc, th, td, tha, tb, tv, ta, tm, tf, tout, tcan, tmc
    finally:
        ctx.close()
    res["k_raster_mesh"] = "its instructions are the parent's (only the headers its definitions sit in were rearranged), so no parent comparison was run"
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "r27_raster_scene.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07_render.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", action="store_true", help="measure ht_render_mesh_depth_dev (the subdivision surface) beside the hull renderer and the tracking step")
    ap.add_argument("--raster", action="store_true", help="measure ht_raster_mesh_depth_dev (the z-buffer rasteriser) beside the mesh ray cast, the hull renderer and the tracking step")
    ap.add_argument("--scene", action="store_true", help="measure ht_raster_scene_depth_dev (several hands in one z-buffer pass) beside its composition from single-hand calls and the two-hand update")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--quick", action="store_true", help="one batch size per case (a check that everything runs)")
    ap.add_argument("--loop-steps", type=int, default=32)
    a = ap.parse_args()
    if a.mesh:
        return main_mesh(a)
    if a.raster:
        return main_raster(a)
    if a.scene:
        return main_scene(a)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s = torch.cuda.Stream(device=dev)
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    z5 = np.load(os.path.join(ROOT, "bench_data", "frames5_256.npz"))
    hands = {17: z["gtpose"], 26: z5["startpose"]}
    res = {"device": torch.cuda.get_device_name(dev), "steps": a.steps, "warmup": a.warmup, "render": [], "usage": {}}
    for k, v in hb.resource_usage().items():
        if "render" in k:
            res["usage"][k] = {x: v.get(x) for x in ("VGPRs", "SGPRs", "AGPRs", "ScratchSize", "LDS Size", "Occupancy")}
    batches = (1024,) if a.quick else (1, 64, 1024, 8192)
    for nb, model in ((17, M17), (26, M26)):
        ctx = native.Context(model, 1)
        try:
            for (w, h) in ((320, 240), (128, 128)):
                for B in batches:
                    for empty in (False, True):
                        p = hands[nb][np.arange(B) % len(hands[nb])].copy()
                        if empty:
                            p[:, :, 2] -= 10.0
                        tp = torch.from_numpy(p).to(dev); tc = torch.from_numpy(cam_of(w, h, B)).to(dev)
                        td = torch.empty((B, h, w), dtype=torch.int16, device=dev)
                        ms = time_it(lambda: ctx.render_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, 4.0, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup)
                        hand_px = float((td.cpu().numpy().view(np.uint16) < 3999).mean())
                        row = {"bones": nb, "w": w, "h": h, "B": B, "empty": empty, "ms": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1), "hand_pixel_fraction": round(hand_px, 4)}
                        print(json.dumps(row), flush=True)
                        res["render"].append(row)
                        del tp, tc, td
        finally:
            ctx.close()
    # ---- closed loop at 1024 frames, 320x240: every step renders a new batch of poses (interpolated between consecutive ground truths) and tracks it ----
    B, w, h, sub = 1024, 320, 240, 4
    gt = z["gtpose"]
    seq = []
    nerr = 8
    for st in range(a.loop_steps + a.warmup + nerr):
        k, t = divmod(st, sub); t = t / sub
        p0 = gt[(np.arange(B) + k) % len(gt)]; p1 = gt[(np.arange(B) + k + 1) % len(gt)]
        p = np.empty_like(p0)
        p[:, :, :3] = p0[:, :, :3] * (1 - t) + p1[:, :, :3] * t
        p[:, :, 3:] = slerp(p0[:, :, 3:].astype(np.float64), p1[:, :, 3:].astype(np.float64), t)
        seq.append(p.astype(np.float32))
    ctx = native.Context(M17, B)
    L = native.load()
    try:
        ctx.load_weights(W.make_cnnb())
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        ctx.reserve_points(w * h // 4)
        com = np.zeros((17, 3), np.float32)
        import ctypes as C
        m = C.c_void_p(); assert L.ht_model_open(M17.encode(), 1, C.byref(m)) == 0
        for b in range(17):
            c3 = np.zeros(3, np.float32); L.ht_model_body(m, b, None, None, None, c3.ctypes.data_as(C.POINTER(C.c_float)), None); com[b] = c3
        L.ht_model_close(m)
        tseq = torch.from_numpy(np.stack(seq)).to(dev)
        tc = torch.from_numpy(cam_of(w, h, B)).to(dev)
        ts = torch.from_numpy(z["startpose"]).to(dev)
        td = torch.empty((B, h, w), dtype=torch.int16, device=dev); out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev)
        ctx.render_depth_dev(tseq[0].data_ptr(), tc.data_ptr(), w, h, 4.0, B, td.data_ptr(), None, s.cuda_stream)
        ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), w, h, 0.17, ts.data_ptr(), B, out.data_ptr(), s.cuda_stream)      # seeds every slot, grows the point arrays
        s.synchronize()
        errs = []
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        step = {"i": 1}

        def loop_step():
            i = step["i"]; step["i"] += 1
            ctx.render_depth_dev(tseq[i].data_ptr(), tc.data_ptr(), w, h, 4.0, B, td.data_ptr(), None, s.cuda_stream)
            ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), w, h, 0.17, None, B, out.data_ptr(), s.cuda_stream)
        for _ in range(a.warmup - 1):
            loop_step()
        s.synchronize()
        e[0].record(s)
        for _ in range(a.loop_steps):
            loop_step()
        e[1].record(s); e[1].synchronize()
        loop_ms = e[0].elapsed_time(e[1]) / a.loop_steps
        for _ in range(nerr):      # then the error against the truth after every step (untimed)
            loop_step()
            s.synchronize()
            got = out.cpu().numpy(); want = user_pos(seq[step["i"] - 1], com)
            errs.append(float(np.linalg.norm(got[:, :, :3] - want, axis=2).mean()))
        # the two halves apart, same batch: the render alone and the tracker step alone
        r_ms = time_it(lambda: ctx.render_depth_dev(tseq[-1].data_ptr(), tc.data_ptr(), w, h, 4.0, B, td.data_ptr(), None, s.cuda_stream), s, a.steps, a.warmup)
        u_ms = time_it(lambda: ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), w, h, 0.17, None, B, out.data_ptr(), s.cuda_stream), s, max(4, a.steps // 4), 1)
        got = out.cpu().numpy()
    finally:
        ctx.close()
    res["closed_loop"] = {"B": B, "w": w, "h": h, "steps": a.loop_steps, "substeps_between_truths": sub, "ms_per_step": round(loop_ms, 3), "frames_per_s": round(B / loop_ms * 1e3, 1),
                          "render_ms": round(r_ms, 3), "update_frames_dev_ms": round(u_ms, 3), "render_over_update": round(r_ms / u_ms, 4),
                          "tracked_vs_truth_mean_body_position_error_m": [round(x, 5) for x in errs],
                          "note": "poses interpolated between consecutive frames1024.npz ground truths (positions lerped, quaternions slerped); error = mean over frames and bodies of |GetPoseUser position - truth|"}
    print(json.dumps(res["closed_loop"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
