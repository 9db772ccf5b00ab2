"""Times the sensor filters (ht_sensor_filter_dev, ht_sensor_background_dev) on resident batches with device events after a warm-up, beside the
ht_update_frames_dev step of the same 1024 frames in the same run (the bar of DESIGN section 17: a stage that feeds the tracker takes at most 0.25 of
that step).  Writes profiles/r15_sensor.json (or --out).

Frames: the bench hands rendered at 640x480 with the background reported as 0 (FilterIvy) and at 320x240 with bright IR and 5 % dark pixels (FilterDS4)."""
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
HBM_PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_sensor.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    ctx = native.Context(M17, 1024)
    rows = []
    try:
        ctx.load_weights(W.make_cnnb()); ctx.set_params(microforce=3.0, mainthreadpasses=3)
        cam640 = np.zeros((1024, 12), np.float32); cam640[:, :5] = [610, 610, 320, 240, 0.001]; cam640[:, 11] = 1
        cam320 = cam640.copy(); cam320[:, :4] /= 2
        poses = z["gtpose"].astype(np.float32)
        raw = ctx.render_depth(poses, cam640, 640, 480); raw[raw == raw.max()] = 0
        qv = ctx.render_depth(poses, cam320, 320, 240)
        rng = np.random.default_rng(0)
        ir = np.where(rng.random(qv.shape) < 0.05, 0, 120).astype(np.uint8)
        usage = {k: v for k, v in hb.resource_usage().items() if "k_sensor_ds4" in k}
        # the tracker's step on the same 1024 frames
        with torch.cuda.stream(s):
            tq = torch.from_numpy(qv.view(np.int16)).to(dev); tc = torch.from_numpy(cam320).to(dev); ts = torch.from_numpy(z["startpose"].astype(np.float32)).to(dev)
            out = torch.empty((1024, 17, 7), dtype=torch.float32, device=dev)
        s.synchronize()
        ctx.update_frames_dev(tq.data_ptr(), tc.data_ptr(), 320, 240, 0.17, ts.data_ptr(), 1024, out.data_ptr(), s.cuda_stream)
        u_ms = time_it(lambda: ctx.update_frames_dev(tq.data_ptr(), tc.data_ptr(), 320, 240, 0.17, None, 1024, out.data_ptr(), s.cuda_stream), s, max(4, a.steps // 4), 1)
        for B in a.batches:
            rep = (B + 1023) // 1024
            with torch.cuda.stream(s):
                tr = torch.from_numpy(np.tile(raw, (rep, 1, 1))[:B].view(np.int16)).to(dev); tc6 = torch.from_numpy(np.tile(cam640, (rep, 1))[:B]).to(dev)
                td = torch.from_numpy(np.tile(qv, (rep, 1, 1))[:B].view(np.int16)).to(dev); ti = torch.from_numpy(np.tile(ir, (rep, 1, 1))[:B]).to(dev)
                tc3 = torch.from_numpy(np.tile(cam320, (rep, 1))[:B]).to(dev)
                to = torch.empty((B, 240, 320), dtype=torch.int16, device=dev); tco = torch.empty((B, 12), dtype=torch.float32, device=dev)
                tb = torch.full((B, 240, 320), 4096, dtype=torch.int16, device=dev)
            s.synchronize()
            px = B * 320 * 240
            calls = {
                "FilterIvy 640x480 -> 320x240": (lambda: ctx.sensor_filter_dev(native.SENSOR_IVY, tr.data_ptr(), None, tc6.data_ptr(), 640, 480, B, 320, None, to.data_ptr(), tco.data_ptr(), s.cuda_stream),
                                                 px * 4, B * 240 * 640 * 2 + px * 2),      # useful: a quarter of the input and the output; fetched: every line of every other row
                "ht_sensor_background_dev 320x240": (lambda: ctx.sensor_background_dev(td.data_ptr(), 320, 240, B, 3, False, tb.data_ptr(), s.cuda_stream), px * 6, None),
                "FilterDS4 320x240": (lambda: ctx.sensor_filter_dev(native.SENSOR_DS4, td.data_ptr(), ti.data_ptr(), tc3.data_ptr(), 320, 240, B, 320, None, to.data_ptr(), tco.data_ptr(), s.cuda_stream), px * 5, None),
                "FilterDS4 320x240 with background": (lambda: ctx.sensor_filter_dev(native.SENSOR_DS4, td.data_ptr(), ti.data_ptr(), tc3.data_ptr(), 320, 240, B, 320, tb.data_ptr(), to.data_ptr(), tco.data_ptr(), s.cuda_stream), px * 7, None),
            }
            for name, (fn, useful, fetched) in calls.items():
                ms = time_it(fn, s, a.steps, a.warmup)
                row = {"call": name, "B": B, "ms": round(ms, 4), "useful_bytes": useful, "useful_TBps": round(useful / ms / 1e9, 3), "of_hbm_peak": round(useful / (ms * 1e-3) / HBM_PEAK, 4),
                       "over_update_step_1024": round(ms / u_ms, 4) if B == 1024 else None}
                if fetched:
                    row["fetched_line_bytes"] = fetched; row["fetched_TBps"] = round(fetched / ms / 1e9, 3)
                if "DS4" in name:      # one wave per frame: rounds of frames per SIMD (4 SIMDs x n_cu), 236 interior rows each
                    n_simd = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
                    rounds = -(-B // n_simd)
                    lds = 5 * 320 * 2 + 320
                    row.update(us_per_row_and_block=round(ms * 1e3 / 240, 3), frames_per_simd=rounds, lds_bytes_per_block=lds, blocks_per_cu_by_lds=min(32, (160 * 1024) // lds),
                               blocks_resident_per_cu=min(32, -(-B // (n_simd // 4))), vgprs=[v["VGPRs"] for v in usage.values()])
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        ctx.close()
    res = {"device": torch.cuda.get_device_name(0), "update_frames_dev_ms_1024": round(u_ms, 3), "bar": "each filter <= 0.25 of the update step at 1024 frames", "rows": rows,
           "note": "us_per_row_and_block is the kernel's time over 240 rows: what a row costs a block while the other resident blocks share its CU, loads and stores included"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"update_frames_dev_ms_1024": res["update_frames_dev_ms_1024"], "out": a.out}))


if __name__ == "__main__":
    main()
