"""Times the left-hand path on 1024 resident frames with device events, every shape warmed first, each figure the median of --rounds series of
--steps launches with the series' spread (max - min), the protocol of tools/bench_joints.py:

 (a) ht_mirror_frames_dev, every flag set, at 320x240 and 640x480, beside a device-to-device hipMemcpyAsync of the same bytes in the same run.  The kernel moves the
     same bytes; the bar is 1.5 times the copy.
 (b) ht_update_hands_dev, every flag set, against ht_update_frames_sized_dev on the same frames already mirrored (side 64, 320x240), the two calls' series
     interleaved.  The mirroring feeds the update, so the bar is DESIGN section 17's: at most 0.25 of it.
 (c) --parent-lib PATH (a library built from the parent commit: HT_LIB_PATH=PATH python -m hand_tracking_samples_amd.build in a checkout of it): ht_update_hands_dev
     without flags against the parent's ht_update_frames_sized_dev, alternating; the difference must be inside twice the parent's spread.

Exits 1 when a bar is missed.  Writes profiles/r19_mirror.json (or --out).  Frames: the bench hands rendered on the device."""
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
B = 1024
HBM_PEAK = 8.0e12


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


def interleaved(fns, stream, steps, warmup, rounds):
    """the calls' series taking turns, so that what else the machine does falls on all alike"""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k] += series(fn, stream, steps, warmup, 1)
    return out


def stat(v):
    return {"ms": round(float(np.median(v)), 5), "spread_ms": round(max(v) - min(v), 5), "series_ms": [round(x, 5) for x in v]}


def parent_update(path, weights):
    """ht_update_frames_sized_dev of the library at `path` on a context of its own (plain ctypes: the parent's library lacks the symbols native.py binds)"""
    L = C.CDLL(path)
    vp = C.c_void_p
    L.ht_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]; L.ht_destroy.argtypes = [vp]
    L.ht_cnn_load_weights.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]; L.ht_get_params.argtypes = [vp, C.POINTER(native.Params)]; L.ht_set_params.argtypes = [vp, C.POINTER(native.Params)]
    L.ht_update_frames_sized_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, vp, C.c_int, vp, vp]
    h = vp()
    if L.ht_create(os.fsencode(M17), B, 0, C.byref(h)) != 0 or L.ht_cnn_load_weights(h, weights.ctypes.data_as(C.POINTER(C.c_float)), weights.size) != 0:
        raise RuntimeError("cannot set up a context of " + path)
    p = native.Params(); L.ht_get_params(h, C.byref(p)); p.microforce = 3.0; p.mainthreadpasses = 3; L.ht_set_params(h, C.byref(p))

    def call(d_depth, d_cams, w, hgt, d_start, d_out, stream):
        if L.ht_update_frames_sized_dev(h, 64, d_depth, d_cams, w, hgt, 0.17, d_start, B, d_out, stream) != 0:
            raise RuntimeError("ht_update_frames_sized_dev failed for " + path)
    return call, (lambda: L.ht_destroy(h))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--update-steps", type=int, default=4, help="launches per series of the update calls (an update of 1024 frames takes tens of milliseconds)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_mirror.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    st = s.cuda_stream
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int
    ctx = native.Context(M17, B)
    res = {"device": torch.cuda.get_device_name(0), "frames": B, "steps": a.steps, "update_steps": a.update_steps, "rounds": a.rounds,
           "resources": {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "Occupancy") if q in v} for k, v in hb.resource_usage().items() if "k_mirror" in k}}
    ok = True
    try:
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        cam = {(640, 480): np.zeros((B, 12), np.float32)}
        cam[(640, 480)][:, :5] = [610, 610, 320, 240, 0.001]; cam[(640, 480)][:, 11] = 1
        cam[(320, 240)] = cam[(640, 480)].copy(); cam[(320, 240)][:, :4] /= 2
        frames = {wh: ctx.render_depth(z["gtpose"].astype(np.float32), cam[wh], wh[0], wh[1]) for wh in cam}
        with torch.cuda.stream(s):
            td = {wh: torch.from_numpy(frames[wh].view(np.int16)).to(dev) for wh in cam}
            to = {wh: torch.empty_like(td[wh]) for wh in cam}
            ones = torch.ones(B, dtype=torch.uint8, device=dev)
        s.synchronize()
        # (a) the frame kernel beside a device-to-device copy of the same bytes
        res["mirror_frames"] = []
        for wh in ((320, 240), (640, 480)):
            nbytes = B * wh[0] * wh[1] * 2
            fns = {"ht_mirror_frames_dev": lambda wh=wh: ctx.mirror_frames_dev(td[wh].data_ptr(), wh[0], wh[1], B, ones.data_ptr(), to[wh].data_ptr(), st),
                   "hipMemcpyAsync": lambda wh=wh, nbytes=nbytes: hip.hipMemcpyAsync(to[wh].data_ptr(), td[wh].data_ptr(), nbytes, 3, st)}
            for fn in fns.values():
                fn()
            s.synchronize()
            ms = interleaved(fns, s, a.steps, a.warmup, a.rounds)
            k, c = stat(ms["ht_mirror_frames_dev"]), stat(ms["hipMemcpyAsync"])
            row = {"frame": "%dx%d" % wh, "bytes_each_way": nbytes, "kernel": k, "copy": c, "kernel_TBps_both_ways": round(2 * nbytes / k["ms"] / 1e9, 3), "copy_TBps_both_ways": round(2 * nbytes / c["ms"] / 1e9, 3),
                   "kernel_of_hbm_peak": round(2 * nbytes / (k["ms"] * 1e-3) / HBM_PEAK, 4), "kernel_over_copy": round(k["ms"] / c["ms"], 4), "within_bar": bool(k["ms"] <= 1.5 * c["ms"])}
            ok = ok and row["within_bar"]
            res["mirror_frames"].append(row); print(json.dumps(row), flush=True)
        # (b) the flagged update against the existing call on the frames already mirrored
        w64 = W.make_cnnb()
        ctx.load_weights(w64)
        wh = (320, 240)
        hands = np.ones(B, np.uint8)
        mirrored = ctx.mirror_frames(frames[wh], hands); mcams = ctx.mirror_cams(cam[wh], wh[0], hands); start = z["startpose"].astype(np.float32)
        with torch.cuda.stream(s):
            tc = torch.from_numpy(cam[wh]).to(dev); tm = torch.from_numpy(mirrored.view(np.int16)).to(dev); tmc = torch.from_numpy(mcams).to(dev)
            ts = torch.from_numpy(start).to(dev); tms = torch.from_numpy(ctx.mirror_poses(start, hands)).to(dev)
            out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev); out2 = torch.empty_like(out)
        s.synchronize()
        ctx.reserve_hands(*wh)
        # the left hands are the rendered frames flipped, with their cameras and start poses mirrored; what the tracker then works on is the frames as rendered
        fns = {"ht_update_hands_dev, every flag set": lambda: ctx.update_hands_dev(64, tm.data_ptr(), tmc.data_ptr(), wh[0], wh[1], 0.17, ones.data_ptr(), tms.data_ptr(), B, out.data_ptr(), st),
               "ht_update_frames_sized_dev, frames already mirrored": lambda: ctx.update_frames_sized_dev(64, td[wh].data_ptr(), tc.data_ptr(), wh[0], wh[1], 0.17, ts.data_ptr(), B, out2.data_ptr(), st)}
        for fn in fns.values():
            fn()
        s.synchronize()
        same = bool(torch.equal(out, torch.from_numpy(ctx.mirror_poses(out2.cpu().numpy(), hands)).to(dev)))
        ms = interleaved(fns, s, a.update_steps, 1, a.rounds)
        h, u = stat(ms["ht_update_hands_dev, every flag set"]), stat(ms["ht_update_frames_sized_dev, frames already mirrored"])
        row = {"frame": "320x240, side 64, re-seeded every call", "hands": h, "update": u, "added_ms": round(h["ms"] - u["ms"], 5), "added_of_update": round((h["ms"] - u["ms"]) / u["ms"], 5),
               "poses_equal_the_mirrored_update": same, "frames_overflow": ctx.frames_overflow(), "within_bar": bool(h["ms"] - u["ms"] <= 0.25 * u["ms"]) and same}
        ok = ok and row["within_bar"]
        res["update_hands"] = row; print(json.dumps(row), flush=True)
        # (c) without flags, against the parent commit's library
        if a.parent_lib:
            par, par_close = parent_update(os.path.abspath(a.parent_lib), w64)
            fns = {"this library, ht_update_hands_dev without flags": lambda: ctx.update_hands_dev(64, td[wh].data_ptr(), tc.data_ptr(), wh[0], wh[1], 0.17, None, ts.data_ptr(), B, out.data_ptr(), st),
                   "parent library, ht_update_frames_sized_dev": lambda: par(td[wh].data_ptr(), tc.data_ptr(), wh[0], wh[1], ts.data_ptr(), out2.data_ptr(), st)}
            for fn in fns.values():
                fn()
            s.synchronize()
            same = bool(torch.equal(out, out2))
            ms = interleaved(fns, s, a.update_steps, 1, a.rounds)
            n, p = stat(ms["this library, ht_update_hands_dev without flags"]), stat(ms["parent library, ht_update_frames_sized_dev"])
            row = {"frame": "320x240, side 64, re-seeded every call", "this": n, "parent": p, "difference_ms": round(n["ms"] - p["ms"], 5), "same_poses": same,
                   "within_bar": bool(abs(n["ms"] - p["ms"]) <= 2 * p["spread_ms"]) and same}
            ok = ok and row["within_bar"]
            res["no_flags_against_parent"] = row; print(json.dumps(row), flush=True)
            par_close()
        else:
            res["no_flags_against_parent"] = "not measured (no --parent-lib)"
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
