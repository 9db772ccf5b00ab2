"""Times the segmentation kernel (ht_segment_vr_sized_dev) on 1024 resident frames with device events, after a warm-up of every shape: 320x240 and 640x480 frames
to 64x64 and 128x128 tiles, useful bytes per second (frame read plus tile written); the worst-case block (640x480 with every pixel in range: 19200 dependent steps
of the raster-order sums) alone and as a batch; and ht_update_frames_sized_dev at 640x480 -> 128 beside ht_update_frames_dev at 320x240 for the 17-bone hand.

--parent-lib PATH: a library built from the parent commit (HT_LIB_PATH=PATH python -m hand_tracking_samples_amd.build in a checkout of it).  The 320x240 -> 64 launch
through the OLD entry point (ht_segment_vr_dev) is then timed through both libraries in this process, alternating the two; the new build may be slower by at most
twice the parent's own run-to-run spread (max - min of its series).  Both series go to the JSON.

Writes profiles/r17_segment.json (or --out).  Frames: the bench hands rendered on the device at both sizes."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand_tracking_samples_amd import build as hb, native, weights as W  # noqa: E402

M17 = os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand17.htfx")
HBM_PEAK = 8.0e12
B = 1024


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


def old_entry(path):
    """ht_segment_vr_dev of the library at `path`, on a context of its own (plain ctypes: the parent's library does not have the symbols native.py binds)"""
    L = C.CDLL(path)
    vp = C.c_void_p
    L.ht_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]; L.ht_destroy.argtypes = [vp]
    L.ht_segment_vr_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp, vp, vp]
    h = vp()
    if L.ht_create(os.fsencode(M17), 1, 0, C.byref(h)) != 0:
        raise RuntimeError("ht_create failed for " + path)

    def call(d_depth, d_cams, w, hgt, n, d_tiles, d_cams_out, stream):
        if L.ht_segment_vr_dev(h, d_depth, d_cams, w, hgt, n, 0xF, 0.1, 0.65, 0.17, d_tiles, d_cams_out, stream) != 0:
            raise RuntimeError("ht_segment_vr_dev failed for " + path)
    return call, (lambda: L.ht_destroy(h))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=9, help="alternations of the A/B against --parent-lib")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-update", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_segment.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    ctx = native.Context(M17, B)
    rows, res = [], {"device": torch.cuda.get_device_name(0), "frames": B}
    try:
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        cam = {(640, 480): np.zeros((B, 12), np.float32)}
        cam[(640, 480)][:, :5] = [610, 610, 320, 240, 0.001]; cam[(640, 480)][:, 11] = 1
        cam[(320, 240)] = cam[(640, 480)].copy(); cam[(320, 240)][:, :4] /= 2
        poses = z["gtpose"].astype(np.float32)
        frames = {wh: ctx.render_depth(poses, cam[wh], wh[0], wh[1]) for wh in cam}
        with torch.cuda.stream(s):
            td = {wh: torch.from_numpy(frames[wh].view(np.int16)).to(dev) for wh in cam}
            tc = {wh: torch.from_numpy(cam[wh]).to(dev) for wh in cam}
            tt = torch.empty((B, 128 * 128), dtype=torch.int16, device=dev); tco = torch.empty((B, 12), dtype=torch.float32, device=dev)
            rng = np.random.default_rng(0)
            full = torch.from_numpy((450 + rng.integers(0, 60, size=(1, 480, 640))).astype(np.uint16).view(np.int16)).to(dev).repeat(B, 1, 1)
        s.synchronize()

        def seg(side, wh, src, n=B):
            return lambda: ctx.segment_vr_sized_dev(side, src.data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], n, tt.data_ptr(), tco.data_ptr(), s.cuda_stream)
        shapes = [(wh, side) for wh in ((320, 240), (640, 480)) for side in (64, 128)]
        for wh, side in shapes:      # every shape once before anything is timed
            seg(side, wh, td[wh])()
        s.synchronize()
        usage = {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "LDS Size", "Occupancy") if q in v} for k, v in hb.resource_usage().items() if "k_segment" in k}
        for wh, side in shapes:
            ms = time_it(seg(side, wh, td[wh]), s, a.steps, a.warmup)
            useful = B * (wh[0] * wh[1] + side * side) * 2
            lds = (wh[0] // 4) * (wh[1] // 4) * 5
            row = {"call": "ht_segment_vr_sized_dev %dx%d -> %d" % (wh[0], wh[1], side), "ms": round(ms, 4), "us_per_frame": round(ms * 1e3 / B, 3), "useful_bytes": useful,
                   "useful_TBps": round(useful / ms / 1e9, 3), "of_hbm_peak": round(useful / (ms * 1e-3) / HBM_PEAK, 4), "dynamic_lds_bytes": lds, "blocks_per_cu_by_lds": min(8, (160 * 1024) // (lds + 128))}
            rows.append(row); print(json.dumps(row), flush=True)
        # the worst-case block: every quarter-size pixel in the blob, so the four raster-order sums run 19200 dependent steps each on four lanes
        for side in (64, 128):
            one = time_it(seg(side, (640, 480), full, 1), s, a.steps, a.warmup)
            typ = time_it(seg(side, (640, 480), td[(640, 480)], 1), s, a.steps, a.warmup)
            allb = time_it(seg(side, (640, 480), full), s, max(4, a.steps // 4), 1)
            row = {"call": "640x480 -> %d, every pixel in range" % side, "one_frame_ms": round(one, 4), "one_frame_ms_rendered_hand": round(typ, 4), "ms_1024_frames": round(allb, 4),
                   "ns_per_dependent_step": round((one - typ) * 1e6 / 19200, 2)}
            rows.append(row); print(json.dumps(row), flush=True)
        res["k_segment_resources"] = usage
        if not a.no_update:
            ctx.load_weights(W.make_cnnb()); ctx.load_weights128(W.make_cnnb128())
            with torch.cuda.stream(s):
                ts = torch.from_numpy(z["startpose"].astype(np.float32)).to(dev); out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev)
            s.synchronize()
            upd = {"ht_update_frames_dev 320x240 (64x64 net)": lambda st: ctx.update_frames_dev(td[(320, 240)].data_ptr(), tc[(320, 240)].data_ptr(), 320, 240, 0.17, st, B, out.data_ptr(), s.cuda_stream),
                   "ht_update_frames_sized_dev 640x480 -> 128 (128x128 net)": lambda st: ctx.update_frames_sized_dev(128, td[(640, 480)].data_ptr(), tc[(640, 480)].data_ptr(), 640, 480, 0.17, st, B, out.data_ptr(), s.cuda_stream),
                   "ht_update_frames_sized_dev 640x480 -> 64 (64x64 net)": lambda st: ctx.update_frames_sized_dev(64, td[(640, 480)].data_ptr(), tc[(640, 480)].data_ptr(), 640, 480, 0.17, st, B, out.data_ptr(), s.cuda_stream)}
            for name, fn in upd.items():
                fn(ts.data_ptr()); s.synchronize()
                ms = time_it(lambda: fn(None), s, max(4, a.steps // 4), 1)
                row = {"call": name, "ms": round(ms, 3), "frames_per_s": round(B / ms * 1e3), "points_per_frame_capacity": ctx.point_capacity(), "frames_overflow": ctx.frames_overflow()}
                rows.append(row); print(json.dumps(row), flush=True)
        res["rows"] = rows
        if a.parent_lib:
            new_call, new_close = old_entry(native.lib_path()); par_call, par_close = old_entry(os.path.abspath(a.parent_lib))
            wh = (320, 240)
            args = (td[wh].data_ptr(), tc[wh].data_ptr(), 320, 240, B, tt.data_ptr(), tco.data_ptr(), s.cuda_stream)
            new_call(*args); par_call(*args); s.synchronize()
            series = {"new": [], "parent": []}
            for _ in range(a.rounds):
                series["parent"].append(round(time_it(lambda: par_call(*args), s, a.steps, a.warmup), 5))
                series["new"].append(round(time_it(lambda: new_call(*args), s, a.steps, a.warmup), 5))
            new_close(); par_close()
            spread = max(series["parent"]) - min(series["parent"])
            med = {k: float(np.median(v)) for k, v in series.items()}
            res["old_entry_320x240_to_64"] = {"call": "ht_segment_vr_dev, 1024 frames, ms per launch, the two libraries alternating", "series_ms": series, "median_ms": med,
                                              "parent_spread_ms": round(spread, 5), "allowed_ms": round(med["parent"] + 2 * spread, 5), "not_slower": bool(med["new"] <= med["parent"] + 2 * spread)}
            print(json.dumps(res["old_entry_320x240_to_64"]), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out}))
    if a.parent_lib and not res["old_entry_320x240_to_64"]["not_slower"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
