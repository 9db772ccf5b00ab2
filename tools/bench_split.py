"""Times the two-hand front end on 1024 resident frames with device events, every shape warmed first, each figure the median of --rounds series
with the series' spread (max - min), the compared calls' series taking turns (the protocol of tools/bench_mirror.py, whose helpers this uses):

 (a) k_split_write alone (the context's own event pair around the launch, ht_profile_enable) at 320x240 and 640x480, beside a device-to-device hipMemcpyAsync that
     moves the same bytes: the kernel reads one frame and writes two, 3 n bytes through the memory system, so the copy is of 1.5 n bytes.  Bar: 1.5 times the copy.
 (b) k_split_label alone, the same way, beside ht_segment_vr_sized_dev (side 64) on the same frames: that kernel also builds the quarter image and scans it in LDS.
     The ratio is recorded; no bar.
 (c) ht_update_two_hands_dev on 512 scenes against ht_split_hands_dev followed by ht_update_hands_dev (flags 0, 1, 0, 1, ...) on the same 1024 hand frames, which
     writes the hand frames twice.  Bar: not slower than the composed path by more than twice its spread; the poses must be the same bytes.
 (d) --parent-lib PATH (a library built from the parent commit: HT_LIB_PATH=PATH python -m hand_tracking_samples_amd.build in a checkout of it):
     ht_update_frames_sized_dev, no two-hand call made, against the parent's, alternating.  Bar: the same poses, the difference inside twice the parent's spread.

--model measures the model split in place of (a)-(d) and writes profiles/r24_split_model.json (or --out): the hands 0.05 m either side of the axis, where
they touch and the blob split sees one component.
 (e) k_split_model (HT_SPLIT_MODEL_ALWAYS: every frame evaluated) at 320x240 and 640x480 beside k_split_label on the same frames, with the foreground cells per frame
     and the closest() evaluations per second that follow.  No bar.
 (f) ht_update_two_hands_model_dev in both modes on 512 touching scenes beside ht_update_two_hands_dev on the same frames, interleaved: the difference is the feature's
     cost, stated as a share of the update.  No bar.
 (g) with --parent-lib: ht_update_two_hands_dev and ht_update_frames_sized_dev on a context no model-split call was made on against the parent commit's library,
     alternating.  Bar: the same poses, the difference inside twice the parent's spread.

Exits 1 when a bar is missed.  Writes profiles/r20_split.json (or --out).  Scenes: two of the bench hands rendered on the device, one of them mirrored, 0.09 m either
side of the optical axis."""
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
LO, HI, FAR, MINPX = 0, 650, 3999, 50


def mirror_poses(p):
    out = p.copy()
    out[..., 0] = -out[..., 0]; out[..., 4] = -out[..., 4]; out[..., 5] = -out[..., 5]
    return out


def kernel_series(ctx, fn, stream, names, steps, warmup):
    """ms per launch of the named kernels over `steps` calls of fn, from the context's event pairs"""
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ctx.profile_read()
    for _ in range(steps):
        fn()
    stream.synchronize()
    prof = ctx.profile_read()
    return {k: prof[k][0] / prof[k][1] for k in names}


def parent_two_hands(path, weights):
    """ht_update_two_hands_dev and ht_update_frames_sized_dev of the library at `path` on a context of its own (plain ctypes, as bench_mirror.parent_update)"""
    L = C.CDLL(path)
    vp = C.c_void_p; u16 = C.c_uint16
    L.ht_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]; L.ht_destroy.argtypes = [vp]
    L.ht_cnn_load_weights.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]; L.ht_get_params.argtypes = [vp, C.POINTER(native.Params)]; L.ht_set_params.argtypes = [vp, C.POINTER(native.Params)]
    L.ht_update_frames_sized_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, vp, C.c_int, vp, vp]
    L.ht_update_two_hands_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, u16, u16, u16, C.c_int, u16, C.c_int, vp, C.c_int, vp, vp, vp]
    h = vp()
    if L.ht_create(os.fsencode(BM.M17), B, 0, C.byref(h)) != 0 or L.ht_cnn_load_weights(h, weights.ctypes.data_as(C.POINTER(C.c_float)), weights.size) != 0:
        raise RuntimeError("cannot set up a context of " + path)
    p = native.Params(); L.ht_get_params(h, C.byref(p)); p.microforce = 3.0; p.mainthreadpasses = 3; L.ht_set_params(h, C.byref(p))

    def two(d_depth, d_cams, w, hgt, d_start, n, d_out, d_info, stream):
        if L.ht_update_two_hands_dev(h, 64, d_depth, d_cams, w, hgt, 0.17, LO, HI, 65535, MINPX, FAR, 0, d_start, n, d_out, d_info, stream) != 0:
            raise RuntimeError("ht_update_two_hands_dev failed for " + path)

    def frames(d_depth, d_cams, w, hgt, d_start, d_out, stream):
        if L.ht_update_frames_sized_dev(h, 64, d_depth, d_cams, w, hgt, 0.17, d_start, B, d_out, stream) != 0:
            raise RuntimeError("ht_update_frames_sized_dev failed for " + path)
    return two, frames, (lambda: L.ht_destroy(h))


def model_rows(a):
    """(e), (f), (g) of the module's text"""
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    st = s.cuda_stream
    inf = float("inf")
    ctx = native.Context(BM.M17, B)
    res = {"device": torch.cuda.get_device_name(0), "frames": B, "steps": a.steps, "update_steps": a.update_steps, "rounds": a.rounds, "lateral_offset_m": 0.05,
           "resources": {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "LDS Size", "Occupancy") if q in v} for k, v in hb.resource_usage().items() if "k_split" in k}}
    ok = True
    try:
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        cam = {(640, 480): np.zeros((B, 12), np.float32)}
        cam[(640, 480)][:, :5] = [610, 610, 320, 240, 0.001]; cam[(640, 480)][:, 11] = 1
        cam[(320, 240)] = cam[(640, 480)].copy(); cam[(320, 240)][:, :4] /= 2
        gt = z["gtpose"].astype(np.float32)
        right = gt.copy(); right[..., 0] += 0.05
        lcanon = np.roll(gt, 341, axis=0).copy(); lcanon[..., 0] += 0.05      # the left hands in canonical space; their frames are rendered through the mirrored camera and flipped
        left = mirror_poses(lcanon)
        frames = {}
        for wh in cam:
            mcam = cam[wh].copy(); mcam[:, 2] = np.float32(wh[0] - 1) - mcam[:, 2]
            frames[wh] = np.minimum(ctx.render_depth(right, cam[wh], wh[0], wh[1]).reshape(B, wh[1], wh[0]), ctx.render_depth(lcanon, mcam, wh[0], wh[1]).reshape(B, wh[1], wh[0])[:, :, ::-1])
        priors = np.ascontiguousarray(np.stack([right, left], axis=1).astype(np.float32))      # [B][2][nb][7], the camera's space
        with torch.cuda.stream(s):
            td = {wh: torch.from_numpy(np.ascontiguousarray(frames[wh]).view(np.int16)).to(dev) for wh in cam}
            tc = {wh: torch.from_numpy(cam[wh]).to(dev) for wh in cam}
            to = {wh: torch.empty((B, 2) + td[wh].shape[1:], dtype=torch.int16, device=dev) for wh in cam}
            tp = torch.from_numpy(priors).to(dev)
            tco = torch.empty((B, 2, 12), dtype=torch.float32, device=dev); info = torch.empty((B, 2, 8), dtype=torch.int32, device=dev); ncomp = torch.empty(B, dtype=torch.int32, device=dev)
            src = torch.empty(B, dtype=torch.int32, device=dev)
        s.synchronize()
        ctx.profile_enable(1)
        res["split_model"] = []
        for wh in ((320, 240), (640, 480)):
            blob = lambda wh=wh: ctx.split_hands_dev(td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], B, LO, HI, 65535, MINPX, FAR, native.SPLIT_MIRROR_LEFT, to[wh].data_ptr(), tco.data_ptr(), info.data_ptr(),
                                                     ncomp.data_ptr(), None, st)
            model = lambda wh=wh: ctx.split_hands_model_dev(td[wh].data_ptr(), tc[wh].data_ptr(), tp.data_ptr(), wh[0], wh[1], B, LO, HI, 65535, 1, FAR, inf, native.SPLIT_MODEL_ALWAYS, native.SPLIT_MIRROR_LEFT,
                                                            to[wh].data_ptr(), tco.data_ptr(), info.data_ptr(), None, src.data_ptr(), None, None, st)
            blob(); s.synchronize()
            merged = int((ncomp < 2).sum().item())
            model(); s.synchronize()
            cells = float(info[:, :, 0].sum().item()) / B      # min_pixels 1, no max_dist: every foreground cell is counted for one hand
            km, kl = [], []
            for _ in range(a.rounds):
                km.append(kernel_series(ctx, model, s, ("k_split_model",), a.steps, a.warmup)["k_split_model"])
                kl.append(kernel_series(ctx, blob, s, ("k_split_label",), a.steps, a.warmup)["k_split_label"])
            km, kl = BM.stat(km), BM.stat(kl)
            row = {"frame": "%dx%d" % wh, "frames_whose_blobs_merged": merged, "foreground_cells_per_frame": round(cells, 1), "k_split_model": km, "k_split_label": kl, "model_over_label": round(km["ms"] / kl["ms"], 4),
                   "closest_evaluations_per_s": round(2 * cells * B / (km["ms"] * 1e-3), 0)}
            res["split_model"].append(row); print(json.dumps(row), flush=True)
        ctx.profile_enable(0)
        # (f) the model update beside the blob update on the same touching scenes
        w64 = W.make_cnnb()
        ctx.load_weights(w64)
        wh = (320, 240); S = B // 2
        with torch.cuda.stream(s):
            out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev); out2 = torch.empty_like(out)
        s.synchronize()
        ctx.reserve_hands(*wh)
        two = lambda: ctx.update_two_hands_dev(64, td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], 0.17, LO, HI, 65535, MINPX, FAR, 0, tp.data_ptr(), S, out.data_ptr(), info.data_ptr(), st)
        mod = lambda mode: (lambda: ctx.update_two_hands_model_dev(64, td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], 0.17, LO, HI, 65535, MINPX, FAR, inf, mode, 0, tp.data_ptr(), S, out2.data_ptr(), info.data_ptr(),
                                                                   src.data_ptr(), st))
        fns = {"ht_update_two_hands_dev": two, "model, merged": mod(native.SPLIT_MODEL_MERGED), "model, always": mod(native.SPLIT_MODEL_ALWAYS)}
        present = {}
        for k, fn in fns.items():
            fn(); s.synchronize()
            present[k] = int((info[:S, :, 0] > 0).all(dim=1).sum().item())
        ms = {k: BM.stat(v) for k, v in BM.interleaved(fns, s, a.update_steps, 1, a.rounds).items()}
        base = ms["ht_update_two_hands_dev"]["ms"]
        row = {"scenes": S, "frame": "320x240, side 64, re-seeded every call", "scenes_with_both_hands_present": present, "ms": ms,
               "cost_ms": {k: round(ms[k]["ms"] - base, 5) for k in ms if k != "ht_update_two_hands_dev"}, "cost_share_of_the_update": {k: round((ms[k]["ms"] - base) / base, 5) for k in ms if k != "ht_update_two_hands_dev"},
               "frames_overflow": ctx.frames_overflow()}
        res["update_two_hands_model"] = row; print(json.dumps(row), flush=True)
        # (g) the existing calls against the parent commit's library
        if a.parent_lib:
            ctx2 = native.Context(BM.M17, B)      # a context no model-split call was made on
            try:
                ctx2.set_params(microforce=3.0, mainthreadpasses=3); ctx2.load_weights(w64)
                ptwo, pframes, pclose = parent_two_hands(os.path.abspath(a.parent_lib), w64)
                with torch.cuda.stream(s):
                    ts1 = torch.from_numpy(z["startpose"].astype(np.float32)).to(dev); info2 = torch.empty_like(info)
                s.synchronize()
                res["existing_calls_against_parent"] = []
                pairs = {"ht_update_two_hands_dev, 512 scenes of 320x240, side 64":
                         (lambda: ctx2.update_two_hands_dev(64, td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], 0.17, LO, HI, 65535, MINPX, FAR, 0, tp.data_ptr(), S, out.data_ptr(), info.data_ptr(), st),
                          lambda: ptwo(td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], tp.data_ptr(), S, out2.data_ptr(), info2.data_ptr(), st)),
                         "ht_update_frames_sized_dev, 1024 frames of 320x240, side 64":
                         (lambda: ctx2.update_frames_sized_dev(64, td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], 0.17, ts1.data_ptr(), B, out.data_ptr(), st),
                          lambda: pframes(td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], ts1.data_ptr(), out2.data_ptr(), st))}
                for name, (this, parent) in pairs.items():
                    fns = {"this library": this, "parent library": parent}
                    for fn in fns.values():
                        fn()
                    s.synchronize()
                    same = bool(torch.equal(out, out2))
                    ms = BM.interleaved(fns, s, a.update_steps, 1, a.rounds)
                    n, p = BM.stat(ms["this library"]), BM.stat(ms["parent library"])
                    row = {"call": name, "this": n, "parent": p, "difference_ms": round(n["ms"] - p["ms"], 5), "same_poses": same, "within_bar": bool(abs(n["ms"] - p["ms"]) <= 2 * p["spread_ms"]) and same}
                    ok = ok and row["within_bar"]
                    res["existing_calls_against_parent"].append(row); print(json.dumps(row), flush=True)
                pclose()
            finally:
                ctx2.close()
        else:
            res["existing_calls_against_parent"] = "not measured (no --parent-lib)"
    finally:
        ctx.close()
    return res, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--update-steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", action="store_true", help="the model split's rows (e)-(g) in place of (a)-(d)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.model:
        res, ok = model_rows(a)
        a.out = a.out or os.path.join(ROOT, "profiles", "r24_split_model.json")
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({"out": a.out, "within_bars": ok}))
        sys.exit(0 if ok else 1)
    a.out = a.out or os.path.join(ROOT, "profiles", "r20_split.json")
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    st = s.cuda_stream
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int
    ctx = native.Context(BM.M17, B)
    res = {"device": torch.cuda.get_device_name(0), "frames": B, "steps": a.steps, "update_steps": a.update_steps, "rounds": a.rounds,
           "resources": {k: {q: v[q] for q in ("VGPRs", "ScratchSize", "LDS Size", "Occupancy") if q in v} for k, v in hb.resource_usage().items() if "k_split" in k}}
    ok = True
    try:
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        cam = {(640, 480): np.zeros((B, 12), np.float32)}
        cam[(640, 480)][:, :5] = [610, 610, 320, 240, 0.001]; cam[(640, 480)][:, 11] = 1
        cam[(320, 240)] = cam[(640, 480)].copy(); cam[(320, 240)][:, :4] /= 2
        gt = z["gtpose"].astype(np.float32)
        right = gt.copy(); right[..., 0] += 0.09
        left = mirror_poses(np.roll(gt, 341, axis=0)); left[..., 0] -= 0.09
        frames = {wh: np.minimum(ctx.render_depth(right, cam[wh], wh[0], wh[1]), ctx.render_depth(left, cam[wh], wh[0], wh[1])) for wh in cam}
        with torch.cuda.stream(s):
            td = {wh: torch.from_numpy(frames[wh].view(np.int16)).to(dev) for wh in cam}
            tc = {wh: torch.from_numpy(cam[wh]).to(dev) for wh in cam}
            to = {wh: torch.empty((B, 2) + td[wh].shape[1:], dtype=torch.int16, device=dev) for wh in cam}
            tco = torch.empty((B, 2, 12), dtype=torch.float32, device=dev); info = torch.empty((B, 2, 8), dtype=torch.int32, device=dev); ncomp = torch.empty(B, dtype=torch.int32, device=dev)
            tiles = torch.empty((B, 64, 64), dtype=torch.int16, device=dev); tcs = torch.empty((B, 12), dtype=torch.float32, device=dev)
        s.synchronize()
        # (a), (b): the two kernels of the split, each beside its yardstick
        ctx.profile_enable(1)
        res["split"] = []
        for wh in ((320, 240), (640, 480)):
            nbytes = B * wh[0] * wh[1] * 2
            split = lambda wh=wh: ctx.split_hands_dev(td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], B, LO, HI, 65535, MINPX, FAR, native.SPLIT_MIRROR_LEFT, to[wh].data_ptr(), tco.data_ptr(), info.data_ptr(),
                                                      ncomp.data_ptr(), None, st)
            seg = lambda wh=wh: ctx.segment_vr_sized_dev(64, td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], B, tiles.data_ptr(), tcs.data_ptr(), st)
            src15 = torch.empty(nbytes * 3 // 2, dtype=torch.uint8, device=dev)
            copy = lambda wh=wh, nbytes=nbytes, src15=src15: hip.hipMemcpyAsync(to[wh].data_ptr(), src15.data_ptr(), nbytes * 3 // 2, 3, st)
            for fn in (split, copy, seg):
                fn()
            s.synchronize()
            both = int((info[:, :, 0] > 0).all(dim=1).sum().item())
            kw, kl, cp, sg = [], [], [], []
            for _ in range(a.rounds):
                k = kernel_series(ctx, split, s, ("k_split_write", "k_split_label"), a.steps, a.warmup)
                kw.append(k["k_split_write"]); kl.append(k["k_split_label"])
                cp += BM.series(copy, s, a.steps, a.warmup, 1)
                sg += BM.series(seg, s, a.steps, a.warmup, 1)
            kw, kl, cp, sg = BM.stat(kw), BM.stat(kl), BM.stat(cp), BM.stat(sg)
            row = {"frame": "%dx%d" % wh, "frames_with_both_hands": both, "bytes_in": nbytes, "bytes_out": 2 * nbytes, "k_split_write": kw, "copy_of_1.5n_bytes": cp,
                   "write_TBps_in_and_out": round(3 * nbytes / kw["ms"] / 1e9, 3), "copy_TBps_in_and_out": round(3 * nbytes / cp["ms"] / 1e9, 3), "write_of_hbm_peak": round(3 * nbytes / (kw["ms"] * 1e-3) / BM.HBM_PEAK, 4),
                   "write_over_copy": round(kw["ms"] / cp["ms"], 4), "within_bar": bool(kw["ms"] <= 1.5 * cp["ms"]), "k_split_label": kl, "ht_segment_vr_sized_dev": sg, "label_over_segment": round(kl["ms"] / sg["ms"], 4)}
            ok = ok and row["within_bar"]
            res["split"].append(row); print(json.dumps(row), flush=True)
        ctx.profile_enable(0)
        # (c) the fused update against split + flagged update
        w64 = W.make_cnnb()
        ctx.load_weights(w64)
        wh = (320, 240); S = B // 2
        start = np.stack([right[:S], left[:S]], axis=1).astype(np.float32)      # [S][2][nb][7], the camera's space
        odd = (np.arange(B) % 2).astype(np.uint8)
        with torch.cuda.stream(s):
            ts = torch.from_numpy(np.ascontiguousarray(start)).to(dev); todd = torch.from_numpy(odd).to(dev)
            out = torch.empty((B, 17, 7), dtype=torch.float32, device=dev); out2 = torch.empty_like(out)
        s.synchronize()
        ctx.reserve_hands(*wh)

        def fused():
            ctx.update_two_hands_dev(64, td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], 0.17, LO, HI, 65535, MINPX, FAR, 0, ts.data_ptr(), S, out.data_ptr(), info.data_ptr(), st)

        def composed():
            ctx.split_hands_dev(td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], S, LO, HI, 65535, MINPX, FAR, 0, to[wh].data_ptr(), tco.data_ptr(), info.data_ptr(), None, None, st)
            ctx.update_hands_dev(64, to[wh].data_ptr(), tco.data_ptr(), wh[0], wh[1], 0.17, todd.data_ptr(), ts.data_ptr(), B, out2.data_ptr(), st)

        fns = {"ht_update_two_hands_dev": fused, "ht_split_hands_dev + ht_update_hands_dev": composed}
        for fn in fns.values():
            fn()
        s.synchronize()
        same = bool(torch.equal(out, out2))
        ms = BM.interleaved(fns, s, a.update_steps, 1, a.rounds)
        f, c = BM.stat(ms["ht_update_two_hands_dev"]), BM.stat(ms["ht_split_hands_dev + ht_update_hands_dev"])
        row = {"scenes": S, "frame": "320x240, side 64, re-seeded every call", "fused": f, "composed": c, "difference_ms": round(f["ms"] - c["ms"], 5), "same_poses": same, "frames_overflow": ctx.frames_overflow(),
               "within_bar": bool(f["ms"] - c["ms"] <= 2 * c["spread_ms"]) and same}
        ok = ok and row["within_bar"]
        res["update_two_hands"] = row; print(json.dumps(row), flush=True)
        # (d) the existing update against the parent commit's library
        if a.parent_lib:
            ctx2 = native.Context(BM.M17, B)      # a context no two-hand call was made on
            try:
                ctx2.set_params(microforce=3.0, mainthreadpasses=3); ctx2.load_weights(w64)
                par, par_close = BM.parent_update(os.path.abspath(a.parent_lib), w64)
                with torch.cuda.stream(s):
                    ts1 = torch.from_numpy(z["startpose"].astype(np.float32)).to(dev)
                s.synchronize()
                fns = {"this library": lambda: ctx2.update_frames_sized_dev(64, td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], 0.17, ts1.data_ptr(), B, out.data_ptr(), st),
                       "parent library": lambda: par(td[wh].data_ptr(), tc[wh].data_ptr(), wh[0], wh[1], ts1.data_ptr(), out2.data_ptr(), st)}
                for fn in fns.values():
                    fn()
                s.synchronize()
                same = bool(torch.equal(out, out2))
                ms = BM.interleaved(fns, s, a.update_steps, 1, a.rounds)
                n, p = BM.stat(ms["this library"]), BM.stat(ms["parent library"])
                row = {"call": "ht_update_frames_sized_dev, 1024 frames of 320x240, side 64", "this": n, "parent": p, "difference_ms": round(n["ms"] - p["ms"], 5), "same_poses": same,
                       "within_bar": bool(abs(n["ms"] - p["ms"]) <= 2 * p["spread_ms"]) and same}
                ok = ok and row["within_bar"]
                res["existing_update_against_parent"] = row; print(json.dumps(row), flush=True)
                par_close()
            finally:
                ctx2.close()
        else:
            res["existing_update_against_parent"] = "not measured (no --parent-lib)"
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
