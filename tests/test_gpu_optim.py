"""The mini-batch gradient as a buffer (ht_cnn_grad_*) and the optimiser steps over it (ht_cnn_opt_*, ht_cnn_train_opt_sized_dev; csrc/ht_optim.hip) on the device.

Gradient tensors, per tensor T of W1 B1 W2 B2 W3 B3 W4 B4 of G (DESIGN.md section 18.1's rule with d32):
    max|G_dev - G_64| <= 4 d32(G) + 4 * 2^-24 max|G_64|,   d32(G) = max|G_f32 - G_64|
both references from tests/train_ref_sized.py's step(..., alpha=1.0, ...) alone (tests/optim_ref.py: grad_reference; tests/test_optim_ref.py shows what the rule tells
from rounding).  Measured d_dev / bound, the largest tensor per batch (MI355X): S5 0.271, S5r 0.277, S33 0.222, Sd 0.304, T5 0.291, the ten
accumulated samples 0.285.
The optimiser step is held bit for bit to the numpy restatement tests/optim_ref.py: every weight, m, v and t."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import optim_ref as orf
import train_batch_ref as tb
import train_ref_sized as ts
from hand_tracking_samples_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAD_CASES = (("S5", 64), ("S5r", 64), ("S33", 64), ("Sd", 64), ("T5", 128))
FC = ("W3", "B3", "W4", "B4")


@pytest.fixture(scope="module")
def w128():
    return W.make_cnnb128()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _batch(name, weights, w128):
    """(side, starting weights, pool inputs, pool targets, order or None)"""
    if name[0] == "S":
        B = tb.BATCHES[name]
        x, t = tb.pool_arrays(name, weights)
        return 64, tb.start_weights(B["w"], weights), x, t, B["order"]
    B = ts.BATCHES[name]
    x, t = ts.pool_arrays(name)
    return 128, ts.start_weights(B["w"], w128), x, t, B["order"]


def _load(ctx, side, w):
    ctx.load_weights(w) if side == 64 else ctx.load_weights128(w)


def _grad(ctx, side, x, t, order=None, accumulate=False):
    """one gradient call: the host form, or the pool form when there is an order; returns the losses"""
    if order is None:
        return ctx.cnn_grad_batch(x, t, accumulate, side=side)
    tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV); tm = torch.full((len(order),), -1.0, device=DEV)
    ctx.cnn_grad_batch_dev(tx.data_ptr(), tt.data_ptr(), len(x), len(order), order=order, accumulate=accumulate, d_mse=tm.data_ptr(), side=side)
    torch.cuda.synchronize()
    return tm.cpu().numpy()


def _rule(G, ref, side, label):
    """d_dev / bound per tensor, printed; the tensors beyond 1.0"""
    P, Q = ts.split(G, side), ts.split(ref["G64"], side)
    bad = []
    for T in ts.TENSORS:
        d, b = ts.dist(P[T], Q[T]), ref["bound"][T]
        print("  %s %-2s d_dev %.3e bound %.3e d_dev/bound %.3f" % (label, T, d, b, d / b))
        if not d <= b:
            bad.append((T, d, b))
    return bad


@pytest.mark.parametrize("name,side", GRAD_CASES)
def test_gradient_tensors_match_float64(name, side, weights, w128):
    from hand_tracking_samples_amd import native
    side_, w, x, t, order = _batch(name, weights, w128)
    assert side_ == side
    xs, tsel = (x, t) if order is None else (x[order], t[order])
    ref = orf.grad_reference(name, w, xs, tsel, side)
    ctx = native.Context(None, 1)
    try:
        _load(ctx, side, w)
        mse = _grad(ctx, side, x, t, order)
        G = ctx.cnn_grad_get(side=side)
        assert _same(ctx.cnn_get_weights(side=side), w), "the gradient call must not touch the weights"
        p, n = ctx.cnn_grad_ptr(side=side)
        assert p and n == G.size == ts.layout(side)[2]
    finally:
        ctx.close()
    assert np.isfinite(G).all()
    bad = _rule(G, ref, side, name)
    for b in range(len(xs)):
        d = abs(float(mse[b]) - float(ref["mse"][b]))
        if not d <= ref["mse_bound"][b]:
            bad.append(("mse", b, d, ref["mse_bound"][b]))
    assert not bad, bad


def test_accumulation(weights):
    """S5, then STEP2's five on top: the ten-sample gradient within the rule; bit for bit the first call's G plus the second call's fresh G in float32; weights untouched"""
    from hand_tracking_samples_amd import native
    w = tb.start_weights("seed", weights)
    x1, t1 = tb.pool_arrays("S5", weights)
    xt = [tb.sample(s, weights) for s in tb.STEP2]
    x2 = np.stack([a for a, _ in xt]); t2 = np.stack([b for _, b in xt])
    ctx = native.Context(None, 1)
    try:
        ctx.load_weights(w)
        ctx.cnn_grad_batch(x1, t1, False)
        G1 = ctx.cnn_grad_get()
        ctx.cnn_grad_batch(x2, t2, True)
        G12 = ctx.cnn_grad_get()
        ctx.cnn_grad_batch(x2, t2, False)
        G2 = ctx.cnn_grad_get()
        assert _same(ctx.cnn_get_weights(), w)
    finally:
        ctx.close()
    ref = orf.grad_reference("S5+STEP2", w, np.concatenate([x1, x2]), np.concatenate([t1, t2]), 64)
    assert not _rule(G12, ref, 64, "S5+STEP2")
    A, B = ts.split(G12, 64), ts.split(G1 + G2, 64)
    for T in ts.TENSORS:      # the FC epilogue is one add per element; so is the convolutions' reduction
        assert _same(A[T], B[T]), T
    assert not _same(G12, G1) and not _same(G12, G2)


@pytest.mark.parametrize("name", ["S5", "S33"])
def test_sgd_from_the_gradient_is_the_fused_step(name, weights):
    """ht_cnn_grad_batch_sized then HT_OPT_SGD with lr = alpha: W3 B3 W4 B4 bit for bit what ht_cnn_train_batch_sized leaves (the same products, the same
    w - alpha * acc); W1 B1 W2 B2 within the weight rule of DESIGN.md section 20 (alpha moves from inside the sum to outside)"""
    from hand_tracking_samples_amd import native
    B = tb.BATCHES[name]
    w = tb.start_weights(B["w"], weights)
    x, t = tb.pool_arrays(name, weights)
    a = native.Context(None, 1); b = native.Context(None, 1)
    try:
        a.load_weights(w); b.load_weights(w)
        m_ref = a.cnn_train_batch(x, t, len(x), B["alpha"], side=64)
        wa = a.cnn_get_weights()
        m = b.cnn_grad_batch(x, t)
        b.cnn_opt_step(native.Opt.default("sgd", lr=B["alpha"]))
        wb = b.cnn_get_weights()
        assert b.cnn_opt_last() == (-1.0, np.float32(1))
    finally:
        a.close(); b.close()
    assert _same(m, m_ref)
    P, Q = ts.split(wa, 64), ts.split(wb, 64)
    for T in FC:
        assert _same(P[T], Q[T]), T
    step = tb.references((name,), weights)[name][0]
    R = ts.split(step["w64"], 64)
    for T in ("W1", "B1", "W2", "B2"):
        d = ts.dist(Q[T], R[T])
        print("%s %s: |w_dev - w_64| %.3e, bound %.3e (%.3f)" % (name, T, d, step["bound"][T], d / step["bound"][T]))
        assert d <= step["bound"][T], T
    assert not _same(wb, w)


# ---- the optimiser step, bit for bit --------------------------------------------------------------------------------------------------------
def _opt_pair(kind, **kw):
    """the same optimiser as the restatement's dict and as an ht_opt"""
    from hand_tracking_samples_amd import native
    o = orf.opt(kind, **kw)
    return o, native.Opt.default(kind, **{k: (int(v) if k == "decoupled_decay" else float(v)) for k, v in o.items() if k != "kind"})


def _two_steps(ctx, side, state, o, no, t0):
    """seed the device, two steps, each compared with the restatement (fed the device's own clip factor); returns the (norm, factor) pairs"""
    w, G, m, v = state
    _load(ctx, side, w)
    ctx.cnn_grad_set(G, side=side)
    ctx.cnn_opt_set_state(m, v, t0, side=side)
    cur = (w, m, v, t0)
    seen = []
    for k in range(2):
        ctx.cnn_opt_step(no, side=side)
        norm, c = ctx.cnn_opt_last(side=side)
        ref = orf.step(cur[0], G, cur[1], cur[2], cur[3], o, side, c=c)
        dw = ctx.cnn_get_weights(side=side); dm, dv, dt = ctx.cnn_opt_state(side=side)
        keeps_m, keeps_v = o["kind"] != orf.SGD, o["kind"] == orf.ADAM
        for what, dev, want in (("w", dw, ref[0]), ("m", dm, ref[1] if keeps_m else cur[1]), ("v", dv, ref[2] if keeps_v else cur[2])):
            diff = np.flatnonzero(_bits(dev) != _bits(want))
            assert diff.size == 0, "step %d: %d of %s differ, first at %d: %r against %r" % (k + 1, diff.size, what, diff[0], dev[diff[0]], want[diff[0]])
        assert dt == ref[3]
        assert _same(ctx.cnn_grad_get(side=side), G)
        cur = (ref[0], ref[1] if keeps_m else cur[1], ref[2] if keeps_v else cur[2], ref[3])
        seen.append((norm, c, ref[4]))
    return seen


@pytest.fixture(scope="module")
def state64():
    return orf.seed_state(64)


@pytest.fixture(scope="module")
def ctx64():
    from hand_tracking_samples_amd import native
    ctx = native.Context(None, 1)
    yield ctx
    ctx.close()


STEP_CASES = [(k, t, dict(weight_decay=wd)) for k in ("sgd", "momentum", "nesterov", "adam") for t in (0, 7) for wd in (0.0, 0.01)] + \
             [("adam", t, dict(weight_decay=0.01, decoupled_decay=1)) for t in (0, 7)]


@pytest.mark.parametrize("kind,t0,kw", STEP_CASES)
def test_optimiser_step_is_the_restatement_bit_for_bit(kind, t0, kw, ctx64, state64):
    o, no = _opt_pair(kind, grad_scale=1.0 / 64, **kw)
    seen = _two_steps(ctx64, 64, state64, o, no, t0)
    assert all(n == -1.0 and c == np.float32(1) for n, c, _ in seen)


@pytest.mark.parametrize("where", ["above", "below"])
def test_clip(where, ctx64, state64):
    G = state64[1]
    norm = float(np.sqrt(np.sum((np.float64(G) / 64.0) ** 2)))
    o, no = _opt_pair("nesterov", grad_scale=1.0 / 64, weight_decay=0.01, clip_norm=norm * (0.25 if where == "above" else 1.5))
    want = orf.clip_factor(G, o)[1]
    for got_norm, c, ref_norm in _two_steps(ctx64, 64, state64, o, no, 0):
        print("clip %s: device norm %.17g, numpy %.17g (%.1e relative); factor %r against %r" % (where, got_norm, ref_norm, abs(got_norm - ref_norm) / ref_norm, c, want))
        assert abs(got_norm - ref_norm) <= 1e-12 * ref_norm
        assert abs(float(c) - float(want)) <= float(np.spacing(want))
        assert (c < 1) if where == "above" else (_bits(c) == _bits(np.float32(1)))


def test_adam_at_side_128(w128):
    """the other vector tail and the other range table"""
    from hand_tracking_samples_amd import native
    o, no = _opt_pair("adam", grad_scale=1.0 / 64, weight_decay=0.01, decoupled_decay=1)
    ctx = native.Context(None, 1)
    try:
        _two_steps(ctx, 128, orf.seed_state(128), o, no, 7)
    finally:
        ctx.close()


def test_inference_follows_the_step(weights):
    """after an Adam step ht_cnn_eval_sized equals the float64 forward at the read-back weights within forward_bounds, and the step moves the outputs by far more"""
    from hand_tracking_samples_amd import native
    w = tb.start_weights("seed", weights)
    x, t = tb.pool_arrays("S5", weights)
    fx = x[[0, 3]]
    ctx = native.Context(None, 2)
    try:
        ctx.load_weights(w)
        ctx.cnn_grad_batch(x, t)
        ctx.cnn_opt_step(native.Opt.default("adam", lr=0.0002))      # Adam's first step moves every weight by about lr: enough to show, not enough to overflow the float32 soft-max
        out = ctx.cnn_eval(fx)
        w1 = ctx.cnn_get_weights()
    finally:
        ctx.close()
    f64, f32 = ts.forward(np.float64(w1), fx, 64, "f64"), ts.forward(w1, fx, 64, "f32")
    bound = ts.forward_bounds(f64, f32)["y"][0]
    y0 = ts.forward(np.float64(w), fx, 64, "f64")["y"]
    for f in range(2):
        d, moved = ts.dist(out[f], f64["y"][f]), ts.dist(y0[f], f64["y"][f])
        print("sample %d: |dev - f64| %.3e, bound %.3e, the step moves the output by %.3e (%.0f x the bound)" % (f, d, bound[f], moved, moved / bound[f]))
        assert moved > 10.0 * bound[f], "the step's effect must exceed the bound for this test to tell a stale copy"
        assert d <= bound[f] and ts.dist(out[f], y0[f]) > bound[f]


def _pool10(weights):
    x1, t1 = tb.pool_arrays("S5", weights)
    xt = [tb.sample(s, weights) for s in tb.STEP2]
    return np.concatenate([x1, np.stack([a for a, _ in xt])]), np.concatenate([t1, np.stack([b for _, b in xt])])


def test_one_call_loop_is_the_sequence_of_calls(weights):
    from hand_tracking_samples_amd import native
    w = tb.start_weights("seed", weights)
    x, t = _pool10(weights)
    order = np.array([9, 3, 3, 0, 7, 1, 4, 4, 8, 2, 6, 5, 0, 1, 2, 9, 8, 7, 7, 5], np.int32)      # 2 steps x 2 gradient calls x 5, repeats inside and across calls
    opt = native.Opt.default("adam", lr=0.002, weight_decay=0.01, clip_norm=0.001, grad_scale=0.1)      # a threshold every gradient here exceeds
    tx = torch.from_numpy(x).to(DEV); tt = torch.from_numpy(t).to(DEV)

    def loop():
        ctx = native.Context(None, 1)
        try:
            ctx.load_weights(w)
            tm = torch.full((20,), -1.0, device=DEV)
            s = torch.cuda.Stream(device=DEV)
            s.wait_stream(torch.cuda.current_stream(DEV))
            ctx.cnn_train_opt_dev(tx.data_ptr(), tt.data_ptr(), 10, 5, opt, accum=2, order=order, n_steps=2, d_mse=tm.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            return (ctx.cnn_get_weights(), ctx.cnn_grad_get()) + ctx.cnn_opt_state() + (tm.cpu().numpy(),) + ctx.cnn_opt_last()
        finally:
            ctx.close()
    one, again = loop(), loop()
    ctx = native.Context(None, 1)
    try:
        ctx.load_weights(w)
        tm = torch.full((20,), -1.0, device=DEV)
        for k in range(4):
            ctx.cnn_grad_batch_dev(tx.data_ptr(), tt.data_ptr(), 10, 5, order=order[5 * k:5 * k + 5], accumulate=bool(k & 1), d_mse=tm.data_ptr() + 4 * 5 * k)
            if k & 1:
                ctx.cnn_opt_step(opt)
        torch.cuda.synchronize()
        calls = (ctx.cnn_get_weights(), ctx.cnn_grad_get()) + ctx.cnn_opt_state() + (tm.cpu().numpy(),) + ctx.cnn_opt_last()
    finally:
        ctx.close()
    assert one[4] == 2 and one[7] < 1 and (one[5] > 0).all() and not _same(one[0], w)
    for a, b, c in zip(one, again, calls):
        if isinstance(a, np.ndarray) and a.ndim:
            assert _same(a, b) and _same(a, c)
        else:
            assert a == b == c


def test_refused_calls_leave_the_context_as_it_was(weights):
    from hand_tracking_samples_amd import native
    w = tb.start_weights("seed", weights)
    x, t = tb.pool_arrays("S5", weights)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rng = np.random.default_rng(3)
    G = rng.standard_normal(native.CNNB_COUNT).astype(np.float32); m = rng.standard_normal(native.CNNB_COUNT).astype(np.float32); v = rng.random(native.CNNB_COUNT).astype(np.float32)
    ctx = native.Context(None, 1)
    try:
        L, h = ctx.L, ctx.h
        err = lambda: L.ht_last_error(h).decode()
        good = native.Opt.default("adam")
        assert L.ht_cnn_grad_batch_sized(h, 64, fp(x), fp(t), 5, 0, None) == 1      # no weights yet
        ctx.load_weights(w)
        buf = np.empty(native.CNNB_COUNT, np.float32); p = C.c_void_p(); n = C.c_size_t()
        # before a buffer exists
        assert L.ht_cnn_grad_batch_sized(h, 64, fp(x), fp(t), 5, 1, None) == 4 and "accumulate" in err()
        assert L.ht_cnn_grad_get_sized(h, 64, fp(buf), buf.size) == 4 and L.ht_cnn_grad_ptr_sized(h, 64, C.byref(p), C.byref(n)) == 4
        assert L.ht_cnn_opt_step_sized_dev(h, 64, C.byref(good), None) == 4 and "gradient" in err()
        assert L.ht_cnn_opt_last_sized(h, 64, None, None) == 4
        ctx.cnn_grad_set(G); ctx.cnn_opt_set_state(m, v, 5)
        for field, value in (("kind", 4), ("kind", -1), ("lr", -1.0), ("lr", float("nan")), ("lr", float("inf")), ("momentum", 1.0), ("momentum", -0.1), ("beta1", 1.0), ("beta1", float("nan")),
                             ("beta2", 1.5), ("beta2", -0.5), ("eps", 0.0), ("eps", float("inf")), ("weight_decay", float("nan")), ("decoupled_decay", 2), ("grad_scale", float("inf")),
                             ("grad_scale", float("nan")), ("clip_norm", -1.0), ("clip_norm", float("nan"))):
            assert L.ht_cnn_opt_step_sized_dev(h, 64, C.byref(good.but(**{field: value})), None) == 1 and field in err(), (field, value, err())
            assert L.ht_cnn_train_opt_sized_dev(h, 64, 1, 1, 5, None, 1, 5, 1, C.byref(good.but(**{field: value})), None, None) == 1 and field in err(), (field, value, err())
        assert L.ht_cnn_opt_step_sized_dev(h, 64, C.byref(native.Opt.default("sgd", decoupled_decay=1)), None) == 1 and "decoupled_decay" in err()
        assert L.ht_cnn_opt_step_sized_dev(h, 64, None, None) == 1
        assert L.ht_cnn_opt_step_sized_dev(h, 96, C.byref(good), None) == 1 and "64 or 128" in err()
        assert L.ht_cnn_opt_step_sized_dev(h, 128, C.byref(good), None) == 1 and "128x128" in err()      # no weights of that net
        assert L.ht_cnn_grad_batch_sized(h, 96, fp(x), fp(t), 5, 0, None) == 1 and "64 or 128" in err()
        assert L.ht_cnn_grad_batch_sized(h, 64, fp(x), fp(t), 0, 0, None) == 1 and L.ht_cnn_grad_batch_sized(h, 64, fp(x), fp(t), 257, 0, None) == 1 and "batch" in err()
        assert L.ht_cnn_grad_batch_sized(h, 64, None, fp(t), 5, 0, None) == 1
        bad_order = np.array([0, 1, 2, 3, 5], np.int32)
        assert L.ht_cnn_grad_batch_sized_dev(h, 64, 1, 1, 5, bad_order.ctypes.data_as(C.POINTER(C.c_int)), 5, 0, None, None) == 1 and "order[4]" in err()
        assert L.ht_cnn_grad_batch_sized_dev(h, 64, 1, 1, 4, None, 5, 0, None, None) == 1
        assert L.ht_cnn_grad_get_sized(h, 64, fp(buf), 5) == 1 and L.ht_cnn_grad_set_sized(h, 64, fp(buf), 5) == 1 and L.ht_cnn_grad_get_sized(h, 96, fp(buf), buf.size) == 1
        assert L.ht_cnn_opt_state_set_sized(h, 64, fp(buf), None, 5, 0) == 1 and L.ht_cnn_opt_state_set_sized(h, 64, None, None, 0, -1) == 1
        assert L.ht_cnn_opt_state_get_sized(h, 64, fp(buf), None, 5, None) == 1
        assert L.ht_cnn_train_opt_sized_dev(h, 64, 1, 1, 5, None, 1, 5, 0, C.byref(good), None, None) == 1 and "accum" in err()
        assert L.ht_cnn_train_opt_sized_dev(h, 64, 1, 1, 5, None, 1, 5, 2, C.byref(good), None, None) == 1      # ten samples of a pool of five
        assert L.ht_cnn_train_opt_sized_dev(h, 64, 1, 1, 5, None, -1, 5, 1, C.byref(good), None, None) == 1
        # nothing moved
        dm, dv, dt = ctx.cnn_opt_state()
        assert _same(ctx.cnn_get_weights(), w) and _same(ctx.cnn_grad_get(), G) and _same(dm, m) and _same(dv, v) and dt == 5
        ctx.cnn_opt_reset()
        dm, dv, dt = ctx.cnn_opt_state()
        assert not dm.any() and not dv.any() and dt == 0
    finally:
        ctx.close()


def test_cxx_wrapper_equals_the_c_calls(tmp_path, weights):
    """tests/cxx_optim_example.cpp: two momentum steps through Optimizer / CNN::GradBatch / CNN::Step, bit for bit the C calls"""
    from hand_tracking_samples_amd import native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w = tb.start_weights("seed", weights)
    x, t = tb.pool_arrays("S5", weights)
    exe = str(tmp_path / "optim")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(root, "tests", "cxx_optim_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    w.tofile(str(tmp_path / "in.cnnb"))
    with open(str(tmp_path / "samples.bin"), "wb") as f:
        f.write(x.tobytes()); f.write(t.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.cnnb"), str(tmp_path / "samples.bin"), "5", str(tmp_path / "out.cnnb"), str(tmp_path / "out.mse")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    ctx = native.Context(None, 1)
    try:
        ctx.load_weights(w)
        o = native.Opt.default("momentum", lr=0.002, grad_scale=0.5)
        mse = []
        for k in range(2):
            mse.append(ctx.cnn_grad_batch(x, t))
            ctx.cnn_opt_step(o)
        want = ctx.cnn_get_weights()
    finally:
        ctx.close()
    assert _same(np.fromfile(str(tmp_path / "out.cnnb"), np.float32), want) and not _same(want, w)
    assert _same(np.fromfile(str(tmp_path / "out.mse"), np.float32), np.concatenate(mse))
