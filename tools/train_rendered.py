"""train-cnn's loop on the device (train-hand-pose-cnn/train-cnn.cpp: render, compress, label, Train), on one stream, from a seed.  Every round:

  1. B poses interpolated between consecutive bench_data/frames1024.npz ground truths (positions lerped, rotations slerped, as tools/bench_render.py);
  2. ht_render_depth_dev at 320x240 with the application's camera (synthetic-tracker.cpp:98);
  3. ht_segment_vr_dev(0xF, {0.1, 0.70});
  4. ht_cnn_input_dev (handtrack.h:700);
  5. ht_expected_cnn_dev(..., HT_LABELS_SEGMENT_FRAME): train-cnn's compress + GatherHandExpectedCNN;
  6. ht_cnn_train_dev over a seeded permutation of the round's samples (batch-1 SGD, lr 0.001, CNN::Train); with --minibatch N the permutation is cut
     into steps of N samples for ht_cnn_train_batch_dev (w' = w - lr * SUM_b g_b(w): a sum, so --lr keeps its per-sample meaning).  --optimizer / --weight-decay /
     --clip-norm / --accum (with --minibatch > 1) step through ht_cnn_train_opt_sized_dev instead: sgd at grad_scale 1 (the same --lr), momentum / nesterov / adam on the
     mean gradient (grad_scale = 1 / (minibatch * accum)); the defaults are the fused step, unchanged.

Held out: the frames tools/train_synthetic.py holds out (every 16th bench frame) and every interpolation that touches one of them.  Reported: the held-out
MSE of the net on those 64 bench tiles, and on how many of them the unit of work takes the CNN-driven pose (the measure of tests/test_gpu_trained_net.py).
Rates: closed-loop samples/s against ht_cnn_train_dev steps/s on a resident pool, and the label and tile-input stages timed with device events.

    python tools/train_rendered.py [--rounds 280] [--batch 1024] [--minibatch 1] [--lr 0.001] [--seed N] [--json profiles/r07_labels.json]

--side 128 trains the 128x128-input net instead (BASELINE configs[4]): the 26-bone hand rendered straight at 128x128 by the camera of that configuration's frames (focal 163,
principal 64, depth scale 0.001, identity pose), no segmentation step; poses interpolated between consecutive start poses of bench_data/frames5_256.npz, every 16th held out;
inputs from ht_cnn_input_sized_dev, labels with HT_LABELS_SIDE128, steps of --minibatch samples through ht_cnn_train_batch_sized_dev.  Reported: the held-out MSE (the
16 held-out poses, rendered the same way) before and after, and the closed-loop samples/s against the training call alone.

--side 128 --frame 640x480 trains that net on what a segmenter hands it: the 17-bone hand of bench_data/frames1024.npz rendered at 640x480 by the SR300's camera (focal 610,
principal (320, 240)), ht_segment_vr_sized_dev(128, 0xF, {0.1, 0.70}), ht_cnn_input_sized_dev, labels with HT_LABELS_SEGMENT_FRAME | HT_LABELS_SIDE128,
ht_cnn_train_batch_sized_dev.  Held out: every 16th ground truth, rendered and segmented the same way.

--sampled (64x64 net) replaces step 1: only the wrist pose of each interpolated ground truth is uploaded (B x 7 floats) and ht_sample_poses_dev(HT_SAMPLE_ENHANCED, --spread)
draws the hand on the device inside the model's joint limits, sample i of round r from (--seed, r * B + i).  Off by default: the other modes compute what they did.

--sensor-noise {ivy,ds4} (64x64 net; off by default, and then nothing below runs) puts the camera between the renderer and the segmenter: every rendered 320x240 frame is made
raw by ht_sensor_simulate_dev under ht_sensor_noise_default's figures (frame f of round r is stream r * B + f of --seed) and filtered by ht_sensor_filter_dev before step 3.  The
tool then trains TWO nets from the same weights on the same poses and permutations for the same number of frames -- one on clean frames (the same filter call, no simulation; a
uniformly bright IR image for ds4), one on simulated frames -- and reports each net's held-out MSE on simulated and on clean renderings of the held-out ground truths (every 16th,
rendered, filtered and segmented the same way; the simulated ones from streams 2^48 onwards).  The noise figures were never measured against a camera: recorded figures, no bar.
--json writes profiles/r22_sensor_train.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hand_tracking_samples_amd import native, weights as W  # noqa: E402
from bench_render import slerp  # noqa: E402

SEED = 0x5EED0001
HOLD = 16
M17 = os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand17.htfx")
M26 = os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand26.htfx")
CAM128 = np.array([163, 163, 64, 64, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)
VGA_CAM = np.array([610, 610, 320, 240, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)
QVGA_CAM = np.array([305, 305, 160, 120, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)


def train_pairs(n):
    """consecutive ground-truth pairs (k, k + 1) that touch no held-out frame"""
    held = set(range(0, n, HOLD))
    return np.array([k for k in range(n - 1) if k not in held and k + 1 not in held])


def draw(gt, pairs, B, rng):
    k = pairs[rng.integers(len(pairs), size=B)]
    t = rng.uniform(0, 1, size=(B, 1, 1))
    p0, p1 = gt[k], gt[k + 1]
    p = np.empty_like(p0)
    p[:, :, :3] = p0[:, :, :3] * (1 - t) + p1[:, :, :3] * t
    p[:, :, 3:] = slerp(p0[:, :, 3:].astype(np.float64), p1[:, :, 3:].astype(np.float64), t)
    return p.astype(np.float32)


def held_out(ctx, d):
    """held-out MSE on the 64 bench tiles train_synthetic.py holds out (host labels of their ground truths), and the CNN-driven pose count"""
    fr = np.arange(0, len(d["gtpose"]), HOLD)
    depth, cams, start = d["depth"][fr].reshape(len(fr), -1), d["cam"][fr], d["startpose"][fr]
    x = ctx.stage_prepare(depth, cams)[0]
    t = np.stack([native.expected_cnn(d["gtpose"][i], d["cam"][i]) for i in fr])
    y = ctx.cnn_eval(x)
    ctx.set_params(microforce=3.0, mainthreadpasses=3)
    ctx.tracker_reset(start)
    _, acc = ctx.update_cnn_model_sync(depth.reshape(len(fr), 64, 64), cams)
    return float(((y - t) ** 2).mean()), int(np.asarray(acc).astype(bool).sum())


def main128(a):
    """the loop for the 128x128-input net: render at 128x128, tile inputs, labels at camsub(cam, 8), mini-batch steps"""
    dev = torch.device("cuda:0")
    seg = a.frame is not None      # full-size frames, segmented to the 128x128 tile
    fw, fh = a.frame if seg else (128, 128)
    d = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz" if seg else "frames5_256.npz"))
    gt = d["gtpose" if seg else "startpose"].astype(np.float32); pairs = train_pairs(len(gt)); nb = gt.shape[1]
    fcam = VGA_CAM.copy() if seg else CAM128
    if seg:
        fcam[:4] *= fw / 640.0
    B = a.batch
    rng = np.random.default_rng(a.seed)
    ctx = native.Context(M17 if seg else M26, 64)
    ctx.load_weights128(W.make_cnnb128(a.seed, 1.0))
    s = torch.cuda.Stream(device=dev)
    cams = torch.from_numpy(np.tile(fcam, (B, 1))).to(dev)
    tp = torch.empty((B, nb, 7), device=dev)
    depth = torch.empty((B, fh, fw), dtype=torch.int16, device=dev)
    tiles = torch.empty((B, 128, 128), dtype=torch.int16, device=dev) if seg else depth
    tcams = torch.empty((B, 12), device=dev) if seg else cams
    x = torch.empty((B, 16384), device=dev); lab = torch.empty((B, 2304), device=dev); mse = torch.empty(B, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]

    def train(order, d_mse=None):
        if a.opt is not None:
            ctx.cnn_train_opt_dev(x.data_ptr(), lab.data_ptr(), B, a.minibatch, a.opt, accum=a.accum, order=order, d_mse=d_mse, stream=s.cuda_stream, side=128)
        else:
            ctx.cnn_train_batch_dev(x.data_ptr(), lab.data_ptr(), B, a.minibatch, order=order, alpha=a.lr, d_mse=d_mse, stream=s.cuda_stream, side=128)

    def round_(poses, order, timed=False):
        with torch.cuda.stream(s):
            tp.copy_(torch.from_numpy(poses))
            if timed: ev[0].record(s)
            ctx.render_depth_dev(tp.data_ptr(), cams.data_ptr(), fw, fh, 4.0, B, depth.data_ptr(), None, s.cuda_stream)
            if timed: ev[1].record(s)
            if seg:
                ctx.segment_vr_sized_dev(128, depth.data_ptr(), cams.data_ptr(), fw, fh, B, tiles.data_ptr(), tcams.data_ptr(), s.cuda_stream, 0xF, (0.1, 0.70), 0.17)
            if timed: ev[2].record(s)
            ctx.cnn_input_dev(tiles.data_ptr(), tcams.data_ptr(), B, x.data_ptr(), s.cuda_stream, side=128)
            if timed: ev[3].record(s)
            ctx.expected_cnn_dev(tp.data_ptr(), tcams.data_ptr(), B, lab.data_ptr(), segment_frame=seg, stream=s.cuda_stream, side=128)
            if timed: ev[4].record(s)
            train(order, mse.data_ptr())
            if timed: ev[5].record(s)

    # held out: every 16th start pose, rendered by the same camera (host forms), labels from the host's GatherHandExpectedCNN on the halved camera
    fr = np.arange(0, len(gt), HOLD)
    hd = ctx.render_depth(gt[fr], np.tile(fcam, (len(fr), 1)), fw, fh, 4.0)
    hd = hd[0] if isinstance(hd, tuple) else hd
    if seg:      # the held-out frames go the same way: the device's segment and its camera, the labels of train-cnn's compress in that camera
        hd, hcams = ctx.segment_vr_sized(hd.reshape(len(fr), fh, fw), np.tile(fcam, (len(fr), 1)), 128, 0xF, (0.1, 0.70), 0.17)
        ht = ctx.expected_cnn_batch(gt[fr], hcams, segment_frame=True, side=128)[0]
    else:
        half = CAM128.copy(); half[:4] *= 0.5
        ht = np.stack([native.expected_cnn(gt[i], half) for i in fr])
    hd = hd.reshape(len(fr), -1)
    hx = np.clip(1.0 - (hd.astype(np.float32) * np.float32(fcam[4]) - np.float32(0.1)) / (np.float32(ctx.params.drangey) - np.float32(0.1)), 0.0, 1.0).astype(np.float32)

    def held_out():
        return float(((ctx.cnn128_eval(hx) - ht) ** 2).mean())

    mse0 = held_out()
    print("before: held-out mse %.3e on %d rendered poses" % (mse0, len(fr)), flush=True)
    curve = []
    stage_ms = np.zeros(5)
    t0 = time.perf_counter()
    for r in range(a.rounds):
        poses = draw(gt, pairs, B, rng); order = rng.permutation(B).astype(np.int32)
        round_(poses, order, timed=True)
        s.synchronize()
        stage_ms += [ev[i].elapsed_time(ev[i + 1]) for i in range(5)]
        if (r + 1) % 10 == 0 or r + 1 == a.rounds:
            rec = {"round": r + 1, "samples": (r + 1) * B, "train_mse": float(mse.mean().item()), "held_out_mse": held_out()}
            curve.append(rec)
            print(rec, "%.0f s" % (time.perf_counter() - t0), flush=True)
    seconds = time.perf_counter() - t0
    stage_ms /= a.rounds
    poses = draw(gt, pairs, B, rng); order = rng.permutation(B).astype(np.int32)
    round_(poses, order); s.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nloop = 4
    with torch.cuda.stream(s):
        e0.record(s)
    for _ in range(nloop):
        round_(poses, order)
    with torch.cuda.stream(s):
        e1.record(s)
    s.synchronize()
    loop_sps = nloop * B / (e0.elapsed_time(e1) / 1e3)
    with torch.cuda.stream(s):
        e0.record(s)
        train(order)
        e1.record(s)
    s.synchronize()
    bare_sps = B / (e0.elapsed_time(e1) / 1e3)
    mse1 = held_out()
    ctx.close()
    what = "the 17-bone hand rendered at %dx%d (render, ht_segment_vr_sized_dev(128), input, HT_LABELS_SEGMENT_FRAME | HT_LABELS_SIDE128 labels" % (fw, fh) if seg else \
        "the 26-bone hand rendered at 128x128 (render, input, HT_LABELS_SIDE128 labels"
    out = {"what": "tools/train_rendered.py --side 128%s: %d rounds of %d frames of %s, steps of %d lr %g over a "
                   "seeded permutation), seed 0x%X" % (" --frame %dx%d" % (fw, fh) if seg else "", a.rounds, B, what, a.minibatch, a.lr, a.seed),
           "side": 128, "rounds": a.rounds, "batch": B, "minibatch": a.minibatch, "lr": a.lr, "optimizer": None if a.opt is None else {k: getattr(a.opt, k) for k, _ in a.opt._fields_}, "accum": a.accum, "samples": a.rounds * B, "seconds": seconds,
           "stage_ms_per_round": {"render": stage_ms[0], "segment": stage_ms[1], "cnn_input": stage_ms[2], "labels": stage_ms[3], "train": stage_ms[4]},
           "closed_loop_samples_per_s": loop_sps, "bare_train_samples_per_s": bare_sps,
           "held_out": {"frames": int(len(fr)), "mse_before": mse0, "mse_after": mse1}, "curve": curve}
    print(json.dumps({k: v for k, v in out.items() if k != "curve"}, indent=1))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


def main_sensor(a):
    """--sensor-noise: the 64x64 net trained on clean and on simulated frames, both judged on held-out simulated and clean frames"""
    dev = torch.device("cuda:0")
    kind = native.SENSOR_IVY if a.sensor_noise == "ivy" else native.SENSOR_DS4
    noise = native.sensor_noise_default(kind, float(QVGA_CAM[4]), 4.0, seed=a.seed)
    d = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    gt = d["gtpose"].astype(np.float32); pairs = train_pairs(len(gt))
    B = a.batch
    fr = np.arange(0, len(gt), HOLD)
    results, held = {}, None
    for trained_on in ("clean", "simulated"):
        rng = np.random.default_rng(a.seed)
        ctx = native.Context(M17, 64)
        ctx.load_weights(W.make_cnnb(a.seed, 1.0))
        if held is None:      # the held-out inputs and labels, once: (x, labels) per kind of frame
            hcams = np.tile(QVGA_CAM, (len(fr), 1))
            clean = ctx.render_depth(gt[fr], hcams, 320, 240)
            raw, ir = ctx.sensor_simulate(kind, clean, noise.but(first_index=1 << 48), want_ir=True)
            held = {}
            for name, frames, irs in (("clean", clean, np.full(clean.shape, 120, np.uint8)), ("simulated", raw, ir)):
                filtered, fc = ctx.sensor_filter(kind, frames, hcams, ir=irs if kind == native.SENSOR_DS4 else None, max_width=320)
                tiles, tc = ctx.segment_vr(filtered, fc, 0xF, (0.1, 0.70), 0.17)
                held[name] = (ctx.stage_prepare(tiles.reshape(len(fr), -1), tc)[0], ctx.expected_cnn_batch(gt[fr], tc, segment_frame=True)[0])
        s = torch.cuda.Stream(device=dev)
        cams = torch.from_numpy(np.tile(QVGA_CAM, (B, 1))).to(dev); fcams = torch.empty((B, 12), device=dev); tcams = torch.empty((B, 12), device=dev)
        tp = torch.empty((B, 17, 7), device=dev)
        depth = torch.empty((B, 240, 320), dtype=torch.int16, device=dev); raw_d = torch.empty_like(depth); filtered_d = torch.empty_like(depth)
        ir_d = torch.full((B, 240, 320), 120, dtype=torch.uint8, device=dev)
        tiles = torch.empty((B, 64, 64), dtype=torch.int16, device=dev)
        x = torch.empty((B, 4096), device=dev); lab = torch.empty((B, 2304), device=dev); mse = torch.empty(B, device=dev)
        d_ir = ir_d.data_ptr() if kind == native.SENSOR_DS4 else None

        def score():
            return {name: float(((ctx.cnn_eval(hx) - ht) ** 2).mean()) for name, (hx, ht) in held.items()}
        before = score()
        print("%s frames: held-out mse before %s" % (trained_on, before), flush=True)
        curve = []
        t0 = time.perf_counter()
        for r in range(a.rounds):
            poses = draw(gt, pairs, B, rng); order = rng.permutation(B).astype(np.int32)
            with torch.cuda.stream(s):
                tp.copy_(torch.from_numpy(poses))
                ctx.render_depth_dev(tp.data_ptr(), cams.data_ptr(), 320, 240, 4.0, B, depth.data_ptr(), None, s.cuda_stream)
                src = depth
                if trained_on == "simulated":
                    ctx.sensor_simulate_dev(kind, depth.data_ptr(), 320, 240, B, noise.but(first_index=r * B), raw_d.data_ptr(), d_ir, s.cuda_stream)
                    src = raw_d
                ctx.sensor_filter_dev(kind, src.data_ptr(), d_ir, cams.data_ptr(), 320, 240, B, 320, None, filtered_d.data_ptr(), fcams.data_ptr(), s.cuda_stream)
                assert ctx.L.ht_segment_vr_dev(ctx.h, filtered_d.data_ptr(), fcams.data_ptr(), 320, 240, B, 0xF, 0.1, 0.70, 0.17, tiles.data_ptr(), tcams.data_ptr(), s.cuda_stream) == 0
                ctx.cnn_input_dev(tiles.data_ptr(), tcams.data_ptr(), B, x.data_ptr(), s.cuda_stream)
                ctx.expected_cnn_dev(tp.data_ptr(), tcams.data_ptr(), B, lab.data_ptr(), segment_frame=True, stream=s.cuda_stream)
                if a.minibatch == 1:
                    ctx.cnn_train_dev(x.data_ptr(), lab.data_ptr(), B, order=order, alpha=a.lr, d_mse=mse.data_ptr(), stream=s.cuda_stream)
                else:
                    ctx.cnn_train_batch_dev(x.data_ptr(), lab.data_ptr(), B, a.minibatch, order=order, alpha=a.lr, d_mse=mse.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            if (r + 1) % 10 == 0 or r + 1 == a.rounds:
                rec = {"round": r + 1, "samples": (r + 1) * B, "train_mse": float(mse.mean().item()), "held_out_mse": score()}
                curve.append(rec)
                print(trained_on, rec, "%.0f s" % (time.perf_counter() - t0), flush=True)
        results[trained_on] = {"held_out_mse_before": before, "held_out_mse_after": curve[-1]["held_out_mse"], "seconds": time.perf_counter() - t0, "curve": curve}
        ctx.close()
    out = {"what": "tools/train_rendered.py --sensor-noise %s: two nets from the same seeded weights, %d rounds of %d rendered 320x240 frames each (render, [ht_sensor_simulate_dev,] "
                   "ht_sensor_filter_dev, segment, input, segment-frame labels, SGD in steps of %d lr %g over a seeded permutation), seed 0x%X; held-out MSE on %d held-out ground "
                   "truths rendered clean and simulated" % (a.sensor_noise, a.rounds, B, a.minibatch, a.lr, a.seed, len(fr)),
           "note": "noise figures: ht_sensor_noise_default, reasoned from data sheets, never measured against a camera; recorded figures, no bar",
           "kind": a.sensor_noise, "noise": {k: getattr(noise, k) for k, _ in noise._fields_}, "rounds": a.rounds, "batch": B, "minibatch": a.minibatch, "lr": a.lr, "optimizer": None if a.opt is None else {k: getattr(a.opt, k) for k, _ in a.opt._fields_}, "accum": a.accum, "samples": a.rounds * B,
           "trained_on": results}
    print(json.dumps({"trained_on": {k: {"held_out_mse_before": v["held_out_mse_before"], "held_out_mse_after": v["held_out_mse_after"]} for k, v in results.items()}}, indent=1))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=64, choices=(64, 128), help="128: train the 128x128-input net on frames rendered at 128x128 (see the module's text)")
    ap.add_argument("--rounds", type=int, default=280)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--minibatch", type=int, default=1, help="samples per SGD step: 1 = ht_cnn_train_dev (CNN::Train sample by sample), N > 1 = ht_cnn_train_batch_dev on steps of N of the round's permutation")
    ap.add_argument("--lr", type=float, default=0.001, help="alpha of every step; a mini-batch step subtracts lr times the SUM of its samples' gradients")
    ap.add_argument("--optimizer", default="sgd", choices=("sgd", "momentum", "nesterov", "adam"), help="with --minibatch > 1: the optimiser of every step (ht_cnn_train_opt_sized_dev).  sgd without "
                    "--weight-decay, --clip-norm or --accum is the fused step above, unchanged.  sgd keeps --lr's per-sample meaning (grad_scale 1); the other kinds step on the MEAN "
                    "gradient, grad_scale = 1 / (minibatch * accum), with ht_opt_default's momentum and betas")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="coupled weight decay on W1..W4 (decoupled for adam)")
    ap.add_argument("--clip-norm", type=float, default=0.0, help="clip the scaled gradient to this global norm (0 = off)")
    ap.add_argument("--accum", type=int, default=1, help="gradient calls of --minibatch samples per optimiser step")
    ap.add_argument("--json", default=None)
    ap.add_argument("--rate-steps", type=int, default=2048)
    ap.add_argument("--frame", default=None, type=lambda v: tuple(int(x) for x in v.lower().split("x")), help="with --side 128: render full-size frames of this size (640x480) and segment them to the 128x128 tile")
    ap.add_argument("--mesh", action="store_true", help="render the training frames from the subdivision surface (ht_render_mesh_depth_dev, pixel offset 0, far 4) instead of the hulls")
    ap.add_argument("--mesh-raster", action="store_true", help="render the training frames from the subdivision surface with the z-buffer rasteriser (ht_raster_mesh_depth_dev, pixel offset 0, far 4); "
                                                                "the JSON then also holds the closed loop's samples/s with the mesh ray cast and with the hulls, measured in the same run")
    ap.add_argument("--sampled", action="store_true", help="draw the hands with ht_sample_poses_dev (HT_SAMPLE_ENHANCED, seed --seed) inside the model's joint limits; only the wrists come from the "
                                                            "interpolated ground truths.  64x64 net only")
    ap.add_argument("--spread", type=float, default=0.98, help="with --sampled: the share of every joint range the sampler uses")
    ap.add_argument("--sensor-noise", default=None, choices=("ivy", "ds4"), help="64x64 net: train one net on clean and one on simulated raw frames of this camera (ht_sensor_simulate_dev, "
                                                                                 "ht_sensor_filter_dev) and report both on held-out simulated frames (see the module's text).  Off by default")
    a = ap.parse_args()
    if a.mesh and a.mesh_raster:
        ap.error("--mesh and --mesh-raster name two renderers of the same surface: choose one")
    if a.mesh_raster and a.side != 64:
        ap.error("--mesh-raster trains the 64x64-input net")
    a.renderer = "raster" if a.mesh_raster else "mesh" if a.mesh else "hull"
    if a.sensor_noise and (a.side != 64 or a.sampled or a.mesh or a.mesh_raster):
        ap.error("--sensor-noise trains the 64x64-input net on hull renderings of the interpolated poses")
    if a.sampled and a.side != 64:
        ap.error("--sampled trains the 64x64-input net")
    if a.minibatch < 1 or a.batch % a.minibatch:
        ap.error("--minibatch must divide --batch")
    a.opt = None      # the optimiser of the steps, or None for the fused SGD step
    if a.optimizer != "sgd" or a.weight_decay or a.clip_norm or a.accum != 1:
        if a.minibatch < 2 or a.accum < 1 or a.batch % (a.minibatch * a.accum) or a.sensor_noise:
            ap.error("--optimizer, --weight-decay, --clip-norm and --accum need --minibatch > 1 with minibatch * accum dividing --batch, and no --sensor-noise")
        a.opt = native.Opt.default(a.optimizer, lr=a.lr, weight_decay=a.weight_decay, clip_norm=a.clip_norm, decoupled_decay=int(a.optimizer == "adam"),
                                   grad_scale=1.0 if a.optimizer == "sgd" else 1.0 / (a.minibatch * a.accum))
    if a.frame is not None and (a.side != 128 or len(a.frame) != 2 or not native.segment_vr_supported(a.frame[0], a.frame[1], 128)):
        ap.error("--frame needs --side 128 and a size ht_segment_vr_supported takes")
    if a.side == 128:
        return main128(a)
    if a.sensor_noise:
        return main_sensor(a)
    dev = torch.device("cuda:0")
    d = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    gt = d["gtpose"]; pairs = train_pairs(len(gt))
    B = a.batch
    rng = np.random.default_rng(a.seed)
    ctx = native.Context(M17, 64)
    ctx.load_weights(W.make_cnnb(a.seed, 1.0))
    s = torch.cuda.Stream(device=dev)
    cams = torch.from_numpy(np.tile(QVGA_CAM, (B, 1))).to(dev)
    tp = torch.empty((B, 17, 7), device=dev)
    depth = torch.empty((B, 240, 320), dtype=torch.int16, device=dev)
    tiles = torch.empty((B, 64, 64), dtype=torch.int16, device=dev); tcams = torch.empty((B, 12), device=dev)
    x = torch.empty((B, 4096), device=dev); lab = torch.empty((B, 2304), device=dev); mse = torch.empty(B, device=dev)
    L = ctx.L

    def train(order, d_mse=None):
        if a.opt is not None:
            ctx.cnn_train_opt_dev(x.data_ptr(), lab.data_ptr(), B, a.minibatch, a.opt, accum=a.accum, order=order, d_mse=d_mse, stream=s.cuda_stream)
        elif a.minibatch == 1:
            ctx.cnn_train_dev(x.data_ptr(), lab.data_ptr(), B, order=order, alpha=a.lr, d_mse=d_mse, stream=s.cuda_stream)
        else:
            ctx.cnn_train_batch_dev(x.data_ptr(), lab.data_ptr(), B, a.minibatch, order=order, alpha=a.lr, d_mse=d_mse, stream=s.cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]

    nsampled = [0]      # samples drawn so far: the next round's first_index
    troots = torch.empty((B, 7), device=dev)

    def round_(poses, order, timed=False, renderer=a.renderer):
        with torch.cuda.stream(s):
            if a.sampled:      # `poses` gives the wrists only; the hands are drawn on the device, inside the model's joint limits
                troots.copy_(torch.from_numpy(np.ascontiguousarray(poses[:, 0])))
                ctx.sample_poses_dev(troots.data_ptr(), B, a.seed, nsampled[0], a.spread, tp.data_ptr(), None, com_poses=True, enhanced=True, stream=s.cuda_stream)
                nsampled[0] += B
            else:
                tp.copy_(torch.from_numpy(poses))      # in the stream's order: the previous round may still read the poses
            if timed: ev[0].record(s)
            if renderer == "raster":
                ctx.raster_mesh_depth_dev(tp.data_ptr(), cams.data_ptr(), 320, 240, 4.0, 0.0, B, depth.data_ptr(), None, s.cuda_stream)
            elif renderer == "mesh":
                ctx.render_mesh_depth_dev(tp.data_ptr(), cams.data_ptr(), 320, 240, 4.0, 0.0, B, depth.data_ptr(), None, s.cuda_stream)
            else:
                ctx.render_depth_dev(tp.data_ptr(), cams.data_ptr(), 320, 240, 4.0, B, depth.data_ptr(), None, s.cuda_stream)
            if timed: ev[1].record(s)
            assert L.ht_segment_vr_dev(ctx.h, depth.data_ptr(), cams.data_ptr(), 320, 240, B, 0xF, 0.1, 0.70, 0.17, tiles.data_ptr(), tcams.data_ptr(), s.cuda_stream) == 0
            if timed: ev[2].record(s)
            ctx.cnn_input_dev(tiles.data_ptr(), tcams.data_ptr(), B, x.data_ptr(), s.cuda_stream)
            if timed: ev[3].record(s)
            ctx.expected_cnn_dev(tp.data_ptr(), tcams.data_ptr(), B, lab.data_ptr(), segment_frame=True, stream=s.cuda_stream)
            if timed: ev[4].record(s)
            train(order, mse.data_ptr())
            if timed: ev[5].record(s)

    mse0, acc0 = held_out(ctx, d)
    print("before: held-out mse %.3e, CNN-driven pose on %d of 64" % (mse0, acc0), flush=True)
    curve = []
    t0 = time.perf_counter()
    stage_ms = np.zeros(5)
    for r in range(a.rounds):
        poses = draw(gt, pairs, B, rng)
        order = rng.permutation(B).astype(np.int32)
        round_(poses, order, timed=True)
        s.synchronize()
        stage_ms += [ev[i].elapsed_time(ev[i + 1]) for i in range(5)]
        if (r + 1) % 20 == 0 or r + 1 == a.rounds:
            rec = {"round": r + 1, "samples": (r + 1) * B, "train_mse": float(mse.mean().item())}
            if (r + 1) % 70 == 0 or r + 1 == a.rounds:
                rec["held_out_mse"], rec["cnn_pose_frames"] = held_out(ctx, d)
            curve.append(rec)
            print(rec, "%.0f s" % (time.perf_counter() - t0), flush=True)
    seconds = time.perf_counter() - t0
    stage_ms /= a.rounds
    # rates: the closed loop (one untimed-stage round per step of the measurement) against bare training steps on a resident pool
    poses = draw(gt, pairs, B, rng); order = rng.permutation(B).astype(np.int32)
    round_(poses, order); s.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nloop = 4
    by_renderer = {}
    for renderer in ((a.renderer, "mesh", "hull") if a.mesh_raster else (a.renderer,)):      # --mesh-raster: the same loop on the other two renderers' frames, in the same run
        round_(poses, order, renderer=renderer); s.synchronize()
        with torch.cuda.stream(s):
            e0.record(s)
        for _ in range(nloop):
            round_(poses, order, renderer=renderer)
        with torch.cuda.stream(s):
            e1.record(s)
        s.synchronize()
        by_renderer[renderer] = nloop * B / (e0.elapsed_time(e1) / 1e3)
    loop_sps = by_renderer[a.renderer]
    nbare =a.rate_steps // a.minibatch * a.minibatch
    bare_order = rng.integers(B, size=nbare).astype(np.int32)
    with torch.cuda.stream(s):
        e0.record(s)
        train(bare_order)
        e1.record(s)
    s.synchronize()
    bare_sps = nbare / (e0.elapsed_time(e1) / 1e3)
    # the label kernel alone (B = 1024 and 8192, labels + key angles written) and the tile inputs, device events over repeated launches
    kern = {}
    for nB in (1024, 8192):
        reps = 50
        P = torch.from_numpy(draw(gt, pairs, nB, rng)).to(dev); Cq = torch.from_numpy(np.tile(QVGA_CAM, (nB, 1))).to(dev)
        E = torch.empty((nB, 2304), device=dev); V = torch.empty((nB, 16), device=dev)
        with torch.cuda.stream(s):
            ctx.expected_cnn_dev(P.data_ptr(), Cq.data_ptr(), nB, E.data_ptr(), None, V.data_ptr(), segment_frame=True, stream=s.cuda_stream)
            e0.record(s)
            for _ in range(reps):
                ctx.expected_cnn_dev(P.data_ptr(), Cq.data_ptr(), nB, E.data_ptr(), None, V.data_ptr(), segment_frame=True, stream=s.cuda_stream)
            e1.record(s)
        s.synchronize()
        ms = e0.elapsed_time(e1) / reps
        stored = nB * (2304 + 16) * 4
        kern["labels_B%d" % nB] = {"ms": ms, "frames_per_s": nB / (ms / 1e3), "stored_bytes": stored, "store_GBps": stored / (ms / 1e3) / 1e9, "of_hbm_peak_8TBps": stored / (ms / 1e3) / 8e12}
        del P, Cq, E, V
    with torch.cuda.stream(s):
        ctx.cnn_input_dev(tiles.data_ptr(), tcams.data_ptr(), B, x.data_ptr(), s.cuda_stream)
        e0.record(s)
        for _ in range(50):
            ctx.cnn_input_dev(tiles.data_ptr(), tcams.data_ptr(), B, x.data_ptr(), s.cuda_stream)
        e1.record(s)
    s.synchronize()
    ms = e0.elapsed_time(e1) / 50
    kern["cnn_input_B%d" % B] = {"ms": ms, "bytes_moved": B * 4096 * 6, "GBps": B * 4096 * 6 / (ms / 1e3) / 1e9}
    mse1, acc1 = curve[-1]["held_out_mse"], curve[-1]["cnn_pose_frames"]
    ctx.close()
    out = {"what": "tools/train_rendered.py%s: train-cnn's loop on the device, one stream: %d rounds of %d rendered 320x240 frames (%srender, segment, input, segment-frame labels, "
                   "SGD in steps of %d lr %g over a seeded permutation), seed 0x%X" % (" --sampled" if a.sampled else "", a.rounds, B,
                                                                                        "ht_sample_poses_dev HT_SAMPLE_ENHANCED spread %g at the interpolated wrists, " % a.spread if a.sampled else "", a.minibatch, a.lr, a.seed),
           "pose_source": "sampled" if a.sampled else "interpolated",
           "rounds": a.rounds, "batch": B, "minibatch": a.minibatch, "lr": a.lr, "optimizer": None if a.opt is None else {k: getattr(a.opt, k) for k, _ in a.opt._fields_}, "accum": a.accum, "samples": a.rounds * B, "seconds": seconds,
           "stage_ms_per_round": {"render": stage_ms[0], "segment": stage_ms[1], "cnn_input": stage_ms[2], "labels": stage_ms[3], "train": stage_ms[4]},
           "kernels": kern, "renderer": a.renderer, "closed_loop_samples_per_s": loop_sps, "closed_loop_samples_per_s_by_renderer": by_renderer, "bare_train_steps_per_s": bare_sps,      # samples/s of the training call alone on the resident pool "loop_over_bare": loop_sps / bare_sps,
           "held_out": {"frames": 64, "mse_before": mse0, "mse_after": mse1, "cnn_pose_frames_before": acc0, "cnn_pose_frames_after": acc1,
                        "train_synthetic_reference": "50 of 64 after 300 epochs of the 960 fixed tiles"},
           "curve": curve}
    print(json.dumps({k: v for k, v in out.items() if k != "curve"}, indent=1))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
