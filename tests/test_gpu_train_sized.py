"""The mini-batch training step of the 128x128-input net (ht_cnn_train_batch_sized / _sized_dev, csrc/ht_train_batch.hip at side 128) against the references of
tests/train_ref_sized.py, on every weight and on every per-sample tensor of the step, and the calls that go with it (ht_cnn_get_weights_sized,
ht_debug_train_batch_buffers_sized, ht_cnn_input_sized_dev, HT_LABELS_SIDE128).

Per weight tensor T of W1 B1 W2 B2 W3 B3 W4 B4 (all 30 429 920 weights), per sample of the latest step for a3 a6 a8 e9 e7 e6 e3, and for every sample's loss:
    max|T_dev - T_64| <= 4 d32(T) + 4 * 2^-24 max|T_64|,   d32(T) = the float32 mode's own distance from the float64 mode on the same batch
(DESIGN.md section 18.1's rule; tests/test_train_sized_ref.py pins the two modes and shows what the rule tells from rounding).
Every batch runs once per module; the references and the results are shared by the tests and left unchanged."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_lib as ol
import pose_frame as pf
import train_batch_ref as tb
import train_ref_sized as ts
from hand_tracking_samples_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
MODEL26 = os.path.join(HERE, "golden", "model_hand26.htfx")


@pytest.fixture(scope="module")
def w128():
    return W.make_cnnb128()


def _run(name, w128, ctx=None):
    """the batch through ht_cnn_train_batch_sized (the pool form when it has an order): weights after, losses, the latest step's tensors"""
    from hand_tracking_samples_amd import native
    B = ts.BATCHES[name]
    x, t = ts.pool_arrays(name)
    own = ctx is None
    if own:
        ctx = native.Context(None, 8)      # a context that serves the nets only
    try:
        ctx.load_weights128(ts.start_weights(B["w"], w128))
        seq, steps = ts.sequence(name)
        if B["order"] is None:
            mse = ctx.cnn_train_batch(x, t, B["batch"], B["alpha"], side=128)
        else:
            tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV); tm = torch.full((len(seq),), -1.0, device=DEV)
            ctx.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), len(x), B["batch"], order=B["order"], alpha=B["alpha"], d_mse=tm.data_ptr(), side=128)
            torch.cuda.synchronize()
            mse = tm.cpu().numpy()
        return dict(w=ctx.cnn_get_weights(side=128), mse=mse, buf=ctx.cnn_train_batch_buffers(steps[-1][1] - steps[-1][0], side=128))
    finally:
        if own:
            ctx.close()


@pytest.fixture(scope="module")
def refs(w128):
    return ts.references(ts.GPU_BATCHES, w128)


@pytest.fixture(scope="module")
def runs(w128):
    return {name: _run(name, w128) for name in ts.GPU_BATCHES}


@pytest.mark.parametrize("name", ts.GPU_BATCHES)
def test_every_weight_and_every_sample_tensor_matches_float64(name, runs, refs):
    dev, steps = runs[name], refs[name]
    last = steps[-1]
    bad = []
    print("batch %s: tensor d_dev bound d_dev/bound" % name)
    assert dev["w"].size == 30429920 and np.isfinite(dev["w"]).all()
    P, Q = ts.split(dev["w"], 128), ts.split(last["w64"], 128)
    for T in ts.TENSORS:
        d, b = ts.dist(P[T], Q[T]), last["bound"][T]
        print("  %s %-4s %.3e %.3e %.3f" % (name, T, d, b, d / b))
        if not d <= b:
            bad.append((T, d, b))
    worst = {}
    for p, rec in enumerate(last["samples"]):      # the latest step's per-sample tensors
        for T in ts.PER_SAMPLE[:-1]:
            d, b = ts.dist(dev["buf"][T][p], rec["tensors"][T].reshape(dev["buf"][T][p].shape)), rec["bound"][T]
            worst[T] = max(worst.get(T, 0.0), d / b)
            if not d <= b:
                print("  %s sample %d (%s) %-3s %.3e %.3e %.3f" % (name, p, last["names"][p], T, d, b, d / b))
                bad.append((p, T, d, b))
    k = 0
    for step in steps:      # every sample's loss, at its step's weights
        for p, rec in enumerate(step["samples"]):
            d, b = abs(float(dev["mse"][k]) - float(rec["tensors"]["mse"])), rec["bound"]["mse"]
            worst["mse"] = max(worst.get("mse", 0.0), d / b)
            if not d <= b:
                print("  %s loss %d (%s) %.3e %.3e %.3f" % (name, k, step["names"][p], d, b, d / b))
                bad.append((k, "mse", d, b))
            k += 1
    print("  %s per-sample, largest d_dev/bound: %s" % (name, " ".join("%s:%.3f" % kv for kv in worst.items())))
    if name == "Td":
        assert (np.abs(dev["buf"]["a8"]) == 1.0).any() and (np.abs(dev["buf"]["a6"]) == 1.0).any()      # the device saturates where the reference does
    assert k == len(dev["mse"]) and not bad, bad


def test_the_same_call_gives_the_same_bits(runs, w128):
    again = _run("T33", w128)
    assert np.array_equal(again["w"], runs["T33"]["w"]) and np.array_equal(again["mse"], runs["T33"]["mse"])
    for T in ts.PER_SAMPLE[:-1]:
        assert np.array_equal(again["buf"][T], runs["T33"]["buf"][T]), T


def test_inference_copies_follow_the_step(runs, refs, w128):
    """ht_cnn_eval_sized(128) after T5x2 reads conv2 and the last layer from copies packed for MFMA.  Its output on the four frames matches the float64
    forward at the stepped weights within the rule, and differs from the forward at the starting weights by more than that bound: a stale W2p or W4p shows."""
    from hand_tracking_samples_amd import native
    fx = np.stack([ts.sample("f%d" % f)[0] for f in ts.FRAMES]); ft = np.stack([ts.sample("f%d" % f)[1] for f in ts.FRAMES])
    ctx = native.Context(None, 8)
    try:
        got = _run("T5x2", w128, ctx)
        assert np.array_equal(got["w"], runs["T5x2"]["w"])
        out = ctx.cnn128_eval(fx)
    finally:
        ctx.close()
    stepped = refs["T5x2"][-1]
    y64 = ts.step(stepped["w64"], fx, ft, 0.001, 128, "f64", want_delta=False)["y"]
    y32 = ts.step(stepped["w32"], fx, ft, 0.001, 128, "f32", want_delta=False)["y"]
    y0 = ts.step(np.float64(w128), fx, ft, 0.001, 128, "f64", want_delta=False)["y"]
    for f in range(len(fx)):
        bound = 4.0 * ts.dist(y32[f], y64[f]) + 4.0 * 2.0 ** -24 * float(np.abs(y64[f]).max())
        d, moved = ts.dist(out[f], y64[f]), ts.dist(y0[f], y64[f])
        print("frame %d: |dev - f64| %.3e, bound %.3e, the two steps move the output by %.3e (%.0f x the bound)" % (ts.FRAMES[f], d, bound, moved, moved / bound))
        assert moved > bound, "the steps' effect must exceed the bound for this test to tell a stale copy"
        assert d <= bound and ts.dist(out[f], y0[f]) > bound


def test_pool_form_on_a_side_stream_equals_the_host_form_on_the_gathered_samples(w128):
    from hand_tracking_samples_amd import native
    x, t = ts.pool_arrays("T5x2")
    order = np.array([9, 3, 3, 0, 7, 1, 4, 4, 8, 2, 6, 5], np.int32)      # three steps of four, repeats inside and across steps
    a = native.Context(None, 1); b = native.Context(None, 1)
    try:
        a.load_weights128(w128); b.load_weights128(w128)
        m_ref = a.cnn_train_batch(x[order], t[order], 4, 0.001, side=128)
        tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV); tm = torch.full((len(order),), -1.0, device=DEV)
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        b.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), len(x), 4, order=order, alpha=0.001, d_mse=tm.data_ptr(), stream=s.cuda_stream, side=128)
        s.synchronize()
        assert np.array_equal(tm.cpu().numpy(), m_ref)
        assert np.array_equal(b.cnn_get_weights(side=128), a.cnn_get_weights(side=128))
    finally:
        a.close(); b.close()


def test_side_64_is_the_unsized_call(weights):
    """S5 of tests/train_batch_ref.py through the sized entry points at side 64 and through ht_cnn_train_batch: the same bits"""
    from hand_tracking_samples_amd import native
    x, t = tb.pool_arrays("S5", weights)
    a = native.Context(None, 1); b = native.Context(None, 1)
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
    try:
        a.load_weights(weights); b.load_weights(weights)
        m_ref = a.cnn_train_batch(x, t, 5, 0.001)
        m = np.zeros(5, np.float32)
        assert b.L.ht_cnn_train_batch_sized(b.h, 64, fp(x), fp(t), 5, 5, 0.001, fp(m)) == 0
        assert np.array_equal(m, m_ref)
        w = np.empty(native.CNNB_COUNT, np.float32)
        assert b.L.ht_cnn_get_weights_sized(b.h, 64, fp(w), w.size) == 0
        assert np.array_equal(w, a.cnn_get_weights())
        ra = a.cnn_train_batch_buffers(5)
        rb = {k: np.empty_like(v) for k, v in ra.items()}
        assert b.L.ht_debug_train_batch_buffers_sized(b.h, 64, 5, *[fp(rb[k]) for k in ("a3", "a6", "a8", "e9", "e7", "e6", "e3")]) == 0
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k
        # and the pool form
        a.load_weights(weights); b.load_weights(weights)
        tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV)
        a.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), 5, 5, order=[0, 3, 3, 1, 4])
        assert b.L.ht_cnn_train_batch_sized_dev(b.h, 64, tx.data_ptr(), tt.data_ptr(), 5, np.array([0, 3, 3, 1, 4], np.int32).ctypes.data_as(C.POINTER(C.c_int)), 1, 5, 0.001, None, None) == 0
        assert np.array_equal(b.cnn_get_weights(), a.cnn_get_weights())
    finally:
        a.close(); b.close()


def test_training_one_net_leaves_the_other_as_it_was(weights, w128):
    from hand_tracking_samples_amd import native
    x64, t64 = tb.pool_arrays("S5", weights)
    x, t = ts.pool_arrays("T5")
    ctx = native.Context(None, 8)
    try:
        ctx.load_weights(weights); ctx.load_weights128(w128)
        y64, y128 = ctx.cnn_eval(x64), ctx.cnn128_eval(x)
        ctx.cnn_train_batch(x, t, 5, 0.001, side=128)
        assert np.array_equal(ctx.cnn_get_weights(), weights) and np.array_equal(ctx.cnn_eval(x64), y64)
        w1 = ctx.cnn_get_weights(side=128)
        assert not np.array_equal(w1, w128) and not np.array_equal(ctx.cnn128_eval(x), y128)
        y128 = ctx.cnn128_eval(x)
        assert np.isfinite(y128).all()
        ctx.cnn_train_batch(x64, t64, 5, 0.001)
        assert not np.array_equal(ctx.cnn_get_weights(), weights)
        assert np.array_equal(ctx.cnn_get_weights(side=128), w1) and np.array_equal(ctx.cnn128_eval(x), y128)
        assert ctx.cnn_train_batch_buffers(5, side=128)["a3"].shape == (5, 16, 31, 31) and ctx.cnn_train_batch_buffers(5)["a3"].shape == (5, 16, 15, 15)
    finally:
        ctx.close()


def test_refused_calls_leave_the_context_as_it_was(runs, weights, w128):
    from hand_tracking_samples_amd import native
    x, t = ts.pool_arrays("T5")
    tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ctx = native.Context(None, 8)
    try:
        call = lambda side, *a: ctx.L.ht_cnn_train_batch_sized_dev(ctx.h, side, *a, None, None)
        err = lambda: ctx.L.ht_last_error(ctx.h).decode()
        assert call(128, tx.data_ptr(), tt.data_ptr(), 5, None, 1, 5, 0.001) == 1 and "128x128" in err()      # nothing loaded
        ctx.load_weights(weights)
        assert call(128, tx.data_ptr(), tt.data_ptr(), 5, None, 1, 5, 0.001) == 1 and "128x128" in err()      # only the 64-input net
        assert ctx.L.ht_cnn_train_batch_sized(ctx.h, 128, fp(x), fp(t), 5, 5, 0.001, None) == 1
        wbuf = np.empty(30429920, np.float32)
        assert ctx.L.ht_cnn_get_weights_sized(ctx.h, 128, fp(wbuf), wbuf.size) != 0
        ctx.load_weights128(w128)
        assert call(96, tx.data_ptr(), tt.data_ptr(), 5, None, 1, 5, 0.001) == 1 and "64 or 128" in err()
        assert ctx.L.ht_cnn_get_weights_sized(ctx.h, 128, fp(wbuf), 9458400) == 1 and ctx.L.ht_cnn_get_weights_sized(ctx.h, 96, fp(wbuf), wbuf.size) == 1
        assert ctx.L.ht_debug_train_batch_buffers_sized(ctx.h, 128, 5, *([fp(wbuf)] * 7)) != 0      # no step of that net has run
        good = np.arange(5, dtype=np.int32)
        for args, word in (((tx.data_ptr(), tt.data_ptr(), 5, ip(good), 1, 0, 0.001), "batch"), ((tx.data_ptr(), tt.data_ptr(), 5, ip(good), 1, 257, 0.001), "batch"),
                           ((tx.data_ptr(), tt.data_ptr(), 5, ip(good), 1, -1, 0.001), "batch"), ((None, tt.data_ptr(), 5, ip(good), 1, 5, 0.001), "inputs"),
                           ((tx.data_ptr(), None, 5, ip(good), 1, 5, 0.001), "targets"), ((tx.data_ptr(), tt.data_ptr(), 0, ip(good), 1, 5, 0.001), "n_pool"),
                           ((tx.data_ptr(), tt.data_ptr(), 5, ip(good), -1, 5, 0.001), "n_steps"), ((tx.data_ptr(), tt.data_ptr(), 5, None, 2, 5, 0.001), "n_steps * batch"),
                           ((tx.data_ptr(), tt.data_ptr(), 5, ip(np.array([0, 1, 2, 3, 5], np.int32)), 1, 5, 0.001), "order[4]"),
                           ((tx.data_ptr(), tt.data_ptr(), 5, ip(np.array([0, -1, 2, 3, 4], np.int32)), 1, 5, 0.001), "order[1]")):
            assert call(128, *args) == 1 and word in err(), (args, err())
        assert ctx.L.ht_cnn_train_batch_sized(ctx.h, 128, fp(x), fp(t), 5, 0, 0.001, None) == 1 and ctx.L.ht_cnn_train_batch_sized(ctx.h, 128, None, fp(t), 5, 5, 0.001, None) == 1
        assert ctx.L.ht_cnn_train_batch_sized(ctx.h, 128, fp(x), fp(t), 0, 5, 0.001, None) == 1
        with pytest.raises(ValueError):
            ctx.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), 5, 5, order=[0, 1, 2], n_steps=1, side=128)
        assert np.array_equal(ctx.cnn_get_weights(side=128), w128) and np.array_equal(ctx.cnn_get_weights(), weights)
        got = _run("T5", w128, ctx)      # a good call after the refusals: the bits of a fresh context
        assert np.array_equal(got["w"], runs["T5"]["w"]) and np.array_equal(got["mse"], runs["T5"]["mse"])
        assert ctx.L.ht_debug_train_batch_buffers_sized(ctx.h, 128, 4, *([fp(wbuf)] * 7)) == 1 and "sample count" in err()
    finally:
        ctx.close()


def test_tile_inputs_equal_the_host_transform():
    """ht_cnn_input_sized_dev(128) on the four frames (and on all 64, past max_batch) against ho_cnn_input, bit for bit; side 64 forwards to ht_cnn_input_dev"""
    from hand_tracking_samples_amd import native
    z = np.load(os.path.join(HERE, "golden", "frames5_64.npz"))
    depth = np.ascontiguousarray(z["depth"].reshape(64, -1)); cams = np.ascontiguousarray(z["cam"], np.float32)
    ref = np.zeros((64, 16384), np.float32)
    for f in range(64):
        ol.lib().ho_cnn_input(ol.u16ptr(depth[f]), 16384, float(cams[f][4]), 0.1, 0.7, ol.fptr(ref[f]))
    for k, f in enumerate(ts.FRAMES):
        assert np.array_equal(ref[f], ts.sample("f%d" % f)[0])
    ctx = native.Context(None, 2)
    try:
        td = torch.from_numpy(depth.view(np.int16)).to(DEV); tc = torch.from_numpy(cams).to(DEV); out = torch.full((64, 16384), -1.0, device=DEV)
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        ctx.cnn_input_dev(td.data_ptr(), tc.data_ptr(), 64, out.data_ptr(), stream=s.cuda_stream, side=128)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref)
        # side 64: the same tiles through both entry points
        t64 = torch.from_numpy(depth[:, :4096].copy().view(np.int16)).to(DEV); o1 = torch.zeros((64, 4096), device=DEV); o2 = torch.zeros((64, 4096), device=DEV)
        ctx.cnn_input_dev(t64.data_ptr(), tc.data_ptr(), 64, o1.data_ptr())
        assert ctx.L.ht_cnn_input_sized_dev(ctx.h, 64, t64.data_ptr(), tc.data_ptr(), 64, o2.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(o1, o2)
        assert ctx.L.ht_cnn_input_sized_dev(ctx.h, 128, td.data_ptr() + 2, tc.data_ptr(), 1, out.data_ptr(), None) == 1      # the alignment rule
        assert ctx.L.ht_cnn_input_sized_dev(ctx.h, 96, td.data_ptr(), tc.data_ptr(), 1, out.data_ptr(), None) == 1
    finally:
        ctx.close()


def test_side128_labels_are_the_labels_of_the_halved_camera():
    """HT_LABELS_SIDE128 on the 64 fixture poses: bit for bit the unflagged call on cameras whose four intrinsics are halved (the kernel reads only focal / sub and
    principal / sub, and a division by a power of two is exact), and host ht_expected_cnn_full on them; also combined with HT_LABELS_SEGMENT_FRAME, and on device buffers"""
    from hand_tracking_samples_amd import native
    z = np.load(os.path.join(HERE, "golden", "frames5_64.npz"))
    P = np.ascontiguousarray(z["startpose"], np.float32); cams = np.ascontiguousarray(z["cam"], np.float32)
    half = cams.copy(); half[:, :4] *= np.float32(0.5)
    moved = cams.copy(); moved[:, 5:8] += np.array([0.01, -0.02, 0.03], np.float32)      # a camera off the origin, so that the segment frame matters
    mhalf = moved.copy(); mhalf[:, :4] *= np.float32(0.5)
    ctx = native.Context(MODEL26, 4)
    try:
        e, ip, v = ctx.expected_cnn_batch(P, cams, side=128)
        e0, ip0, v0 = ctx.expected_cnn_batch(P, half)
        he, hip, hv = pf.host_labels(P, half)
        for a, b, c in ((e, e0, he), (ip, ip0, hip), (v, v0, hv)):
            assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
        assert e.max() > 0 and not np.array_equal(e, ctx.expected_cnn_batch(P, cams)[0])
        for k, f in enumerate(ts.FRAMES):
            assert np.array_equal(e[f], ts.sample("f%d" % f)[1])
        s1, s0 = ctx.expected_cnn_batch(P, moved, segment_frame=True, side=128), ctx.expected_cnn_batch(P, mhalf, segment_frame=True)
        for a, b in zip(s1, s0):
            assert np.array_equal(a, b, equal_nan=True)
        tp = torch.from_numpy(P).to(DEV); tc = torch.from_numpy(cams).to(DEV); te = torch.zeros((64, 2304), device=DEV)
        ctx.expected_cnn_dev(tp.data_ptr(), tc.data_ptr(), 64, te.data_ptr(), side=128)
        torch.cuda.synchronize()
        assert np.array_equal(te.cpu().numpy(), e)
        assert ctx.L.ht_expected_cnn_dev(ctx.h, tp.data_ptr(), tc.data_ptr(), 64, 4, te.data_ptr(), None, None, None) == 1      # an unknown flag
    finally:
        ctx.close()
