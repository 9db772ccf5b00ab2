"""The mini-batch training step (csrc/ht_train_batch.hip, ht_cnn_train_batch / ht_cnn_train_batch_dev) against the float64 references of
tests/train_batch_ref.py, on every weight and on every per-sample tensor of the step.

Per weight tensor T of W1 B1 W2 B2 W3 B3 W4 B4 (all 9 458 400 weights):
    max|T_dev' - T_64'| <= 4 d_orc(T) + 4 * 2^-24 max|T_64'|,   d_orc(T) = max|T_32' - T_64'|  (the composed float32 oracle's own distance)
Per sample of the latest step, for a3 a6 a8 e9 e7 e6 e3 (ht_debug_train_batch_buffers) and for every sample's loss: the same expression on that sample's own
float64 / oracle step (train_ref.bound for a case of train_ref.CASES).  tests/test_train_batch_ref.py shows what this tells from rounding.
Every batch runs once per module; the results are shared by the tests and left unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as ol
import train_batch_ref as tb
import train_ref as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run(name, weights, ctx=None):
    """the batch through ht_cnn_train_batch (ht_cnn_train_batch_dev when it has an order): weights after, losses, the latest step's tensors"""
    from hand_tracking_samples_amd import native
    B = tb.BATCHES[name]
    x, t = tb.pool_arrays(name, weights)
    own = ctx is None
    if own:
        ctx = native.Context(ol.MODEL, 1)
    try:
        ctx.load_weights(tb.start_weights(B["w"], weights))
        seq, steps = tb.sequence(name)
        if B["order"] is None:
            mse = ctx.cnn_train_batch(x, t, B["batch"], B["alpha"])
        else:
            tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV); tm = torch.full((len(seq),), -1.0, device=DEV)
            ctx.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), len(x), B["batch"], order=B["order"], alpha=B["alpha"], d_mse=tm.data_ptr())
            torch.cuda.synchronize()
            mse = tm.cpu().numpy()
        return dict(w=ctx.cnn_get_weights(), mse=mse, buf=ctx.cnn_train_batch_buffers(steps[-1][1] - steps[-1][0]))
    finally:
        if own:
            ctx.close()


@pytest.fixture(scope="module")
def refs(weights):
    return tb.references(tb.GPU_BATCHES, weights)


@pytest.fixture(scope="module")
def runs(weights):
    return {name: _run(name, weights) for name in tb.GPU_BATCHES}


@pytest.mark.parametrize("name", tb.GPU_BATCHES)
def test_every_weight_and_every_sample_tensor_matches_float64(name, runs, refs):
    dev, steps = runs[name], refs[name]
    last = steps[-1]
    bad = []
    print("batch %s: tensor d_dev bound d_dev/bound" % name)
    P, Q = tr.split(dev["w"]), tr.split(last["w64"])
    for T in tb.TENSORS:
        d, b = tr.dist(P[T], Q[T]), last["bound"][T]
        print("  %s %-4s %.3e %.3e %.3f" % (name, T, d, b, d / b))
        if not d <= b:
            bad.append((T, d, b))
    for p, rec in enumerate(last["samples"]):      # the latest step's per-sample tensors
        for T in tb.PER_SAMPLE[:-1]:
            d, b = tr.dist(dev["buf"][T][p], rec["tensors"][T].reshape(dev["buf"][T][p].shape)), rec["bound"][T]
            if p < 5 or not d <= b:
                print("  %s sample %d (%s) %-3s %.3e %.3e %.3f" % (name, p, last["names"][p], T, d, b, d / b))
            if not d <= b:
                bad.append((p, T, d, b))
    k = 0
    for step in steps:      # every sample's loss, at its step's weights
        for p, rec in enumerate(step["samples"]):
            d, b = abs(float(dev["mse"][k]) - float(rec["tensors"]["mse"])), rec["bound"]["mse"]
            print("  %s loss %d (%s) %.3e %.3e %.3f" % (name, k, step["names"][p], d, b, d / b))
            if not d <= b:
                bad.append((k, "mse", d, b))
            k += 1
    assert k == len(dev["mse"]) and not bad, bad


def test_a_batch_of_one_is_cnn_train(runs, refs, weights):
    """two implementations of one function: ht_cnn_train_batch with batch = 1 against ht_cnn_train on the same sample, under the same rule;
    the pooled outputs of both convolutions, which the two steps compute with shared code, bit for bit"""
    from hand_tracking_samples_amd import native
    x, t = tb.pool_arrays("S1", weights)
    ctx = native.Context(ol.MODEL, 1)
    try:
        ctx.load_weights(tb.start_weights("seed", weights))
        mse = ctx.cnn_train(x, t, tb.BATCHES["S1"]["alpha"])
        w1 = ctx.cnn_get_weights()
        buf1 = ctx.cnn_train_buffers()
    finally:
        ctx.close()
    step = refs["S1"][0]
    P, Q = tr.split(runs["S1"]["w"]), tr.split(w1)
    bad = []
    for T in tb.TENSORS:
        d, b = tr.dist(P[T], Q[T]), step["bound"][T]
        print("  batch 1 against ht_cnn_train %-4s %.3e %.3e %.3f" % (T, d, b, d / b))
        if not d <= b:
            bad.append((T, d, b))
    d, b = abs(float(mse[0]) - float(runs["S1"]["mse"][0])), step["samples"][0]["bound"]["mse"]
    print("  loss %.3e %.3e" % (d, b))
    assert not bad and d <= b, (bad, d, b)
    # both convolutions forward are one piece of code for the two steps (csrc/ht_train_shared.hpp): the same bits from the same weights
    for T in ("a3", "a6"):
        assert np.array_equal(buf1[T].reshape(-1), runs["S1"]["buf"][T][0].reshape(-1)), T


def test_the_same_call_gives_the_same_bits(runs, weights):
    again = _run("S33", weights)
    assert np.array_equal(again["w"], runs["S33"]["w"]) and np.array_equal(again["mse"], runs["S33"]["mse"])
    for T in tb.PER_SAMPLE[:-1]:
        assert np.array_equal(again["buf"][T], runs["S33"]["buf"][T]), T


def test_inference_copies_follow_the_step(runs, weights):
    """cnn_eval after S5 reads conv2 and the last layer from copies packed for MFMA: they hold the stepped weights (bounds of tests/test_gpu_cnn.py)"""
    from hand_tracking_samples_amd import native
    x, _ = tb.pool_arrays("S5", weights)
    ctx = native.Context(ol.MODEL, 8)
    try:
        got = _run("S5", weights, ctx)
        assert np.array_equal(got["w"], runs["S5"]["w"])
        out = ctx.cnn_eval(x)
        _, a6, a8, lg = ctx.cnn_layers(len(x))
    finally:
        ctx.close()
    L = ol.lib()
    worst = {}
    for f in range(len(x)):
        for label, w in (("stepped", got["w"]), ("start", tb.start_weights("seed", weights))):
            layers = [np.zeros(n, np.float32) for n in tr.SIZES]
            y = np.zeros(2304, np.float32)
            L.ho_cnn_eval(ol.fptr(np.ascontiguousarray(w, np.float32)), ol.fptr(np.ascontiguousarray(x[f])), ol.fptr(y), (C.POINTER(C.c_float) * 11)(*[ol.fptr(a) for a in layers]))
            for k, a, b in (("conv2+pool", a6[f], layers[6]), ("fc1", a8[f], layers[8]), ("fc2", lg[f], layers[9]), ("softmax", out[f], y)):
                worst[label, k] = max(worst.get((label, k), 0.0), float(np.abs(a - b).max()))
    print({"%s %s" % k: "%.2e" % v for k, v in worst.items()})
    assert worst["stepped", "conv2+pool"] <= 5e-6 and worst["stepped", "fc1"] <= 1e-5 and worst["stepped", "fc2"] <= 1e-4 and worst["stepped", "softmax"] <= 2e-5
    # the step is visible at these bounds, and so is either packed copy left stale on its own (the oracle on the stepped weights with W2 / W4 put back)
    O = tr.OFF
    assert worst["start", "conv2+pool"] > 50e-6 and worst["start", "fc2"] > 10e-4
    for k, li, tol in (("W2", 6, 5e-6), ("W4", 9, 1e-4)):
        stale = got["w"].copy(); stale[O[k]:O[k] + int(np.prod(tr.SHAPE[k]))] = weights[O[k]:O[k] + int(np.prod(tr.SHAPE[k]))]
        moved = 0.0
        for f in range(len(x)):
            pair = []
            for w in (got["w"], stale):
                layers = [np.zeros(n, np.float32) for n in tr.SIZES]
                y = np.zeros(2304, np.float32)
                L.ho_cnn_eval(ol.fptr(w), ol.fptr(np.ascontiguousarray(x[f])), ol.fptr(y), (C.POINTER(C.c_float) * 11)(*[ol.fptr(a) for a in layers]))
                pair.append(layers[li])
            moved = max(moved, float(np.abs(pair[0] - pair[1]).max()))
        print("a stale %s alone moves layer %d by %.3e, %.0f x its bound" % (k, li, moved, moved / tol))
        assert moved > 10.0 * tol


def test_pool_form_on_a_side_stream_equals_the_host_form_on_the_gathered_samples(weights):
    from hand_tracking_samples_amd import native
    B = tb.BATCHES["S5x2"]
    x, t = tb.pool_arrays("S5x2", weights)
    order = np.array([9, 3, 3, 0, 7, 1, 4, 4, 8, 2, 6, 5], np.int32)      # three steps of four, repeats inside and across steps
    a = native.Context(ol.MODEL, 1); b = native.Context(ol.MODEL, 1)
    try:
        a.load_weights(weights); b.load_weights(weights)
        m_ref = a.cnn_train_batch(x[order], t[order], 4, B["alpha"])
        tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV); tm = torch.full((len(order),), -1.0, device=DEV)
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        b.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), len(x), 4, order=order, alpha=B["alpha"], d_mse=tm.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(tm.cpu().numpy(), m_ref)
        assert np.array_equal(b.cnn_get_weights(), a.cnn_get_weights())
        # a remainder: 10 samples in steps of 4 are 4 + 4 + 2, the same as the pool form's 2 steps of 4 followed by a call with batch 2
        a.load_weights(weights); b.load_weights(weights)
        m_ref = a.cnn_train_batch(x, t, 4, B["alpha"])
        b.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), len(x), 4, n_steps=2, alpha=B["alpha"], d_mse=tm.data_ptr())
        b.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), len(x), 2, order=[8, 9], alpha=B["alpha"], d_mse=tm.data_ptr() + 32)
        torch.cuda.synchronize()
        assert np.array_equal(tm.cpu().numpy()[:10], m_ref)
        assert np.array_equal(b.cnn_get_weights(), a.cnn_get_weights())
    finally:
        a.close(); b.close()


def test_refused_calls_leave_the_context_as_it_was(runs, weights):
    from hand_tracking_samples_amd import native, weights as make_w
    x, t = tb.pool_arrays("S5", weights)
    tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ctx = native.Context(ol.MODEL, 1)
    try:
        call = lambda *a: ctx.L.ht_cnn_train_batch_dev(ctx.h, *a, None, None)
        err = lambda: ctx.L.ht_last_error(ctx.h).decode()
        assert call(tx.data_ptr(), tt.data_ptr(), 5, None, 1, 5, 0.001) == 1 and "weights" in err()      # nothing loaded
        ctx.load_weights128(make_w.make_cnnb128())
        assert call(tx.data_ptr(), tt.data_ptr(), 5, None, 1, 5, 0.001) == 1 and "64x64" in err()          # only the 128-input net
        assert ctx.L.ht_cnn_train_batch(ctx.h, fp(x), fp(t), 5, 5, 0.001, None) == 1
        ctx.load_weights(weights)
        good = np.arange(5, dtype=np.int32)
        for args, word in (((tx.data_ptr(), tt.data_ptr(), 5, ip(good), 1, 0, 0.001), "batch"), ((tx.data_ptr(), tt.data_ptr(), 5, ip(good), 1, 257, 0.001), "batch"),
                           ((tx.data_ptr(), tt.data_ptr(), 5, ip(good), 1, -1, 0.001), "batch"), ((None, tt.data_ptr(), 5, ip(good), 1, 5, 0.001), "inputs"),
                           ((tx.data_ptr(), None, 5, ip(good), 1, 5, 0.001), "targets"), ((tx.data_ptr(), tt.data_ptr(), 0, ip(good), 1, 5, 0.001), "n_pool"),
                           ((tx.data_ptr(), tt.data_ptr(), 5, ip(good), -1, 5, 0.001), "n_steps"), ((tx.data_ptr(), tt.data_ptr(), 5, None, 2, 5, 0.001), "n_steps * batch"),
                           ((tx.data_ptr(), tt.data_ptr(), 5, ip(np.array([0, 1, 2, 3, 5], np.int32)), 1, 5, 0.001), "order[4]"),
                           ((tx.data_ptr(), tt.data_ptr(), 5, ip(np.array([0, -1, 2, 3, 4], np.int32)), 1, 5, 0.001), "order[1]")):
            assert call(*args) == 1 and word in err(), (args, err())
        assert ctx.L.ht_cnn_train_batch(ctx.h, fp(x), fp(t), 5, 0, 0.001, None) == 1 and ctx.L.ht_cnn_train_batch(ctx.h, None, fp(t), 5, 5, 0.001, None) == 1
        assert ctx.L.ht_cnn_train_batch(ctx.h, fp(x), fp(t), 0, 5, 0.001, None) == 1
        with pytest.raises(ValueError):
            ctx.cnn_train_batch_dev(tx.data_ptr(), tt.data_ptr(), 5, 5, order=[0, 1, 2], n_steps=1)
        assert np.array_equal(ctx.cnn_get_weights(), weights)
        got = _run("S5", weights, ctx)      # a good call after the refusals: the bits of a fresh context
        assert np.array_equal(got["w"], runs["S5"]["w"]) and np.array_equal(got["mse"], runs["S5"]["mse"])
    finally:
        ctx.close()
