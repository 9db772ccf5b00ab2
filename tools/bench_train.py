"""Time the device training step on seeded inputs.

bench_train.py [n]                         ht_cnn_train: ms per SGD step and the implied weight traffic (as before)
bench_train.py --batch N [N ...] [--out F] samples/s of the mini-batch step (ht_cnn_train_batch_dev) per batch size on a pool resident on the device,
                                           timed with device events after a warm-up, at least 20 steps per size, beside the batch-1 path
                                           (ht_cnn_train_dev, one sample a step) in the same run; --out writes the figures as JSON.
bench_train.py --side 128 --batch N [...]  the same sizes for the 128x128-input net as well (ht_cnn_train_batch_sized_dev on a pool of 16384-float inputs), after the
                                           64x64-input path of the same run, with the ratio of the two steps per size (no stage's work grows by more than 5.44 x); profiles/r14_train128.json is its --out.
bench_train.py --batch N [...] --optimizer K [K ...]  after the above, in the same run: the gradient call alone (ht_cnn_grad_batch_sized_dev), each optimiser's step alone
                                           (ht_cnn_opt_step_sized_dev, with and without the global-norm clip) beside a device-to-device copy of the bytes it moves, and
                                           the one-call loop of both (ht_cnn_train_opt_sized_dev) against the fused step; profiles/r23_optim.json is its --out."""
import argparse, json, sys, time, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hand_tracking_samples_amd import native, weights

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=256)
ap.add_argument("--batch", nargs="+", type=int, default=None)
ap.add_argument("--steps", type=int, default=40, help="timed steps per batch size (at least 20)")
ap.add_argument("--side", type=int, default=64, choices=(64, 128), help="128: time the 128x128-input net's step too, beside the 64x64-input one")
ap.add_argument("--optimizer", nargs="+", choices=("sgd", "momentum", "nesterov", "adam"), default=None, help="with --batch: also time the gradient call, these optimisers' steps and the loop of both")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.optimizer and args.batch is None:
    ap.error("--optimizer times steps over mini-batch gradients: give --batch N [N ...]")
if args.side == 128 and args.batch is None:
    ap.error("--side 128 times the mini-batch step: give --batch N [N ...]")
n = args.n
if args.batch is not None:
    import torch      # before the library opens the device
ctx = native.Context(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "model_hand17.htfx"), 1)
W0 = weights.make_cnnb()
ctx.load_weights(W0)
rng = np.random.default_rng(3)
if args.batch is None:
    xs = rng.random((n, 4096), dtype=np.float32)
    ts = np.zeros((n, 2304), np.float32)
    for m in range(24):
        ts[np.arange(n), (256 * m if m < 8 else 2048 + 16 * (m - 8)) + rng.integers(0, 16, n)] = 1.0
    ctx.cnn_train(xs[:8], ts[:8], 0.001)
    t0 = time.perf_counter(); mse = ctx.cnn_train(xs, ts, 0.001); dt = time.perf_counter() - t0
    print("steps %d  %.3f ms/step  %.1f GB/s weight traffic (75.7 MB/step)  mse first %.5f last %.5f" % (n, dt / n * 1e3, 75.7e-3 / (dt / n), mse[0], mse[-1]))
    sys.exit(0)

steps = max(20, args.steps)
pool = max(1024, max(args.batch))
xs = rng.random((pool, 4096), dtype=np.float32)
ts = np.zeros((pool, 2304), np.float32)
for m in range(24):
    ts[np.arange(pool), (256 * m if m < 8 else 2048 + 16 * (m - 8)) + rng.integers(0, 16, pool)] = 1.0
dev = torch.device("cuda:0")
tx = torch.from_numpy(xs).to(dev); tt = torch.from_numpy(ts).to(dev)
stream = torch.cuda.Stream(device=dev)


def timed(call, reps=3, reload=lambda: ctx.load_weights(W0)):
    """the best of `reps` timings of call() between two device events on the tool's stream, each from the seeded weights, after one warm-up"""
    best = None
    for r in range(reps + 1):
        reload()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); call(); e1.record(stream); e1.synchronize()
        if r:
            best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
    return best


out = {"steps": steps, "pool": pool, "batch": {}}
n1 = max(256, steps)
order1 = rng.integers(0, pool, n1).astype(np.int32)
ms = timed(lambda: ctx.cnn_train_dev(tx.data_ptr(), tt.data_ptr(), pool, order=order1, alpha=0.001, stream=stream.cuda_stream))
base = n1 / ms * 1e3
out["batch1_path"] = {"samples": n1, "ms_per_step": ms / n1, "samples_per_s": base}
print("batch-1 path (ht_cnn_train_dev)  %d steps  %.4f ms/step  %.0f samples/s" % (n1, ms / n1, base))
for b in args.batch:
    order = rng.integers(0, pool, steps * b).astype(np.int32)
    ms = timed(lambda: ctx.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), pool, b, order=order, alpha=0.001 / b, stream=stream.cuda_stream))
    rate = steps * b / ms * 1e3
    out["batch"][str(b)] = {"steps": steps, "ms_per_step": ms / steps, "samples_per_s": rate, "ratio_to_batch1_path": rate / base}
    print("batch %-4d %d steps  %.4f ms/step  %.0f samples/s  %.2f x the batch-1 path" % (b, steps, ms / steps, rate, rate / base))
if args.side == 128:
    W128 = weights.make_cnnb128()
    tx128 = torch.from_numpy(rng.random((pool, 16384), dtype=np.float32)).to(dev)
    out["side128"] = {"pool": pool, "batch": {}}
    for b in args.batch:
        order = rng.integers(0, pool, steps * b).astype(np.int32)
        ms = timed(lambda: ctx.cnn_train_batch_dev(tx128.data_ptr(), tt.data_ptr(), pool, b, order=order, alpha=0.001 / b, stream=stream.cuda_stream, side=128), reload=lambda: ctx.load_weights128(W128))
        rate = steps * b / ms * 1e3
        small = out["batch"][str(b)]["ms_per_step"]
        out["side128"]["batch"][str(b)] = {"steps": steps, "ms_per_step": ms / steps, "samples_per_s": rate, "step_over_side64_step": ms / steps / small}
        print("side 128 batch %-4d %d steps  %.4f ms/step  %.0f samples/s  %.2f x the 64x64-input net's step (work grows by at most 5.44 x)" % (b, steps, ms / steps, rate, ms / steps / small))
if args.optimizer:
    # The gradient call alone, the optimiser step alone and the one-call loop of both (ht_cnn_train_opt_sized_dev, accum = 1), beside the fused step timed above in this run;
    # and the step kernel against a device-to-device copy that moves the same bytes (SGD reads w, G and writes w: 3 arrays of the weight count; momentum 5; Adam 7).
    ARRAYS = {"sgd": 3, "momentum": 5, "nesterov": 5, "adam": 7}
    out["optimizer"] = {}
    for side in ((64, 128) if args.side == 128 else (64,)):
        px = tx if side == 64 else tx128
        reload = (lambda: ctx.load_weights(W0)) if side == 64 else (lambda: ctx.load_weights128(W128))
        count = native.CNNB_COUNT if side == 64 else native.CNNB128_COUNT
        fused = out["batch"] if side == 64 else out["side128"]["batch"]
        rec = out["optimizer"][str(side)] = {"grad": {}, "step": {}, "loop": {}}
        for b in args.batch:
            order = rng.integers(0, pool, steps * b).astype(np.int32)

            def grads():
                for k in range(steps):
                    ctx.cnn_grad_batch_dev(px.data_ptr(), tt.data_ptr(), pool, b, order=order[k * b:(k + 1) * b], stream=stream.cuda_stream, side=side)
            ms = timed(grads, reload=reload) / steps
            rec["grad"][str(b)] = {"ms_per_call": ms, "fused_step_ms": fused[str(b)]["ms_per_step"]}
            print("side %d batch %-4d gradient call %.4f ms (the fused step: %.4f ms)" % (side, b, ms, fused[str(b)]["ms_per_step"]))
        for kind in args.optimizer:
            opt = native.Opt.default(kind, lr=1e-6)

            def opt_steps():
                for k in range(steps):
                    ctx.cnn_opt_step(opt, stream=stream.cuda_stream, side=side)
            ms = timed(opt_steps, reload=reload) / steps      # the step with the refresh of the packed copies
            nbytes = ARRAYS[kind] * count * 4
            src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev); dst = torch.empty_like(src)

            def copies():
                with torch.cuda.stream(stream):
                    for k in range(steps):
                        dst.copy_(src)
            cp = timed(copies, reload=lambda: None) / steps
            clip = native.Opt.default(kind, lr=1e-6, clip_norm=1.0)

            def clip_steps():
                for k in range(steps):
                    ctx.cnn_opt_step(clip, stream=stream.cuda_stream, side=side)
            msc = timed(clip_steps, reload=reload) / steps
            rec["step"][kind] = {"ms_per_step": ms, "ms_per_step_with_clip": msc, "bytes_moved": nbytes, "copy_of_the_same_bytes_ms": cp, "GBps": nbytes / ms * 1e-6, "copy_GBps": nbytes / cp * 1e-6}
            print("side %d %-8s step %.4f ms (with clip %.4f), a copy of its %d MB %.4f ms" % (side, kind, ms, msc, nbytes >> 20, cp))
            del src, dst
            for b in args.batch:
                order = rng.integers(0, pool, steps * b).astype(np.int32)
                ms = timed(lambda: ctx.cnn_train_opt_dev(px.data_ptr(), tt.data_ptr(), pool, b, native.Opt.default(kind, lr=1e-6, grad_scale=1.0 / b), order=order, stream=stream.cuda_stream, side=side), reload=reload) / steps
                rec["loop"]["%s/%d" % (kind, b)] = {"ms_per_step": ms, "fused_step_ms": fused[str(b)]["ms_per_step"]}
                print("side %d %-8s batch %-4d gradient + step %.4f ms  (%.2f x the fused step)" % (side, kind, b, ms, ms / fused[str(b)]["ms_per_step"]))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
