"""tests/train_ref.py's float64 training step with the net's dimensions as parameters (side 64 or 128, .cnnb order, cnnb_count(side)), a float32 mode of
the same step, and the mini-batch composition of tests/train_batch_ref.py on them.  A helper, not a test; it needs no GPU and no compiled oracle.

forward(w, X, side, mode) is the forward pass alone (the inference tests' reference: tests/test_cnn_forward_ref.py, tests/test_gpu_cnn_forward.py); step() calls it.
step(w, X, T, alpha, side, mode) steps every row of X [n, side*side] / T [n, 2304] at the same weights w:
    mode "f64"   train_ref.train_step's arithmetic (the same tap loops, the same products), float64, the n samples side by side
    mode "f32"   float32 throughout, every sum accumulated in third_party/cnn.h's order as oracle/ho_cnn.c restates it: one multiply and one add per term
                 (an axpy over the summed index, or a running sum), never a pairwise sum; exp is the C library's expf (csrc/ht_expf.hpp's restatement)
and returns the per-sample tensors a3 a6 a8 e9 e7 e6 e3 mse (and the forward layers logits, y), per sample and weight tensor how far the sample moves it
("effect"), and the batch's summed weight difference  sum_b (step_b(w) - w)  in float64.  One batch at a time: a float64 weight vector of the larger net is
243 MB, so no per-sample weight differences are kept.

One step on samples s_0..s_{n-1}:   w64' = w64 + sum_b d64_b,   w32' = w32 + sum_b d32_b (sums in float64; a later step starts from w64' and from w32' rounded
to float32).  The rule is DESIGN.md section 18.1's with the float32 mode in the oracle's place:
    max|T_dev - T_64| <= 4 d32(T) + 4 * 2^-24 max|T_64|,   d32(T) = max|T_32 - T_64|
tests/test_train_sized_ref.py shows at side 64 that d32 is no looser than the pinned oracle's distance, and at side 128 that the forward pass is the
reference's own (tests/golden/cnn128.htfx).

Samples at side 128: "f<k>" = the net's input of frame k of tests/golden/frames5_64.npz with the labels of its start pose at camsub(cam, 8) (host
ht_expected_cnn on the camera with halved intrinsics), "z0" / "z1" an all-0 / all-1 tile, "x<i>" dense default_rng(100 + i) inputs and targets.
Batches (name -> weights, pool, order, samples per step, alpha):
    T1    [x0]                                  one sample
    T5    [f0, z0, z1, x0, f9]                  no multiple of 4 (a padded k-slot), an all-0 and an all-1 tile
    T5r   T5 with order [0, 3, 3, 1, 4]         a sample twice
    T33   T5 + [f33, f60] + x1..x26             one row past a 32-sample tile
    Td    [x0, x1] on the scaled weights        tanh at exactly +-1.0f
    T5x2  T5 + [f33, f60, x1, x2, x3], 5 a step the second step starts from the first's weights
    T5x2stale (the second step's samples at the seeded weights) serves tests/test_train_sized_ref.py only.
Results are cached per batch and not to be modified."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNKS = [(256 * c, 256) for c in range(8)] + [(2048 + 16 * c, 16) for c in range(16)]      # LSoftMaxChunked of handtrack.h:118
PER_SAMPLE = ("a3", "a6", "a8", "e9", "e7", "e6", "e3", "mse")
TENSORS = ("W1", "B1", "W2", "B2", "W3", "B3", "W4", "B4")
# batch Td: W1 and W2 times SAT_SCALE128 (train_ref.SAT_SCALE) and W3 times SAT_FC1_SCALE128: the convolutions alone saturate a6 but leave the 12544-term sums under
# a8 near 4; with W3 times 4 they reach 17 (exp(2 t) overflows past 44).  tests/test_train_sized_ref.py asserts that the float32 mode stays finite and reaches exact +-1.0f.
SAT_SCALE128, SAT_FC1_SCALE128 = 8.0, 4.0


def dims(side):
    c1 = side - 4; p2 = c1 // 4; c2 = p2 - 3; p3 = c2 // 2
    return dict(side=side, c1=c1, p2=p2, c2=c2, p3=p3, fc=64 * p3 * p3)


def layout(side):
    """(OFF, SHAPE, COUNT) of the .cnnb order (CNN::saveb cnn.h:591-593)"""
    fc = dims(side)["fc"]
    shape = {"W1": (16, 5, 5), "B1": (16,), "W2": (64, 16, 4, 4), "B2": (64,), "W3": (fc, 2048), "B3": (2048,), "W4": (2048, 2304), "B4": (2304,)}
    off, o = {}, 0
    for k in TENSORS:
        off[k] = o; o += int(np.prod(shape[k]))
    return off, shape, o


def split(w, side):
    off, shape, _ = layout(side)
    return {k: w[off[k]:off[k] + int(np.prod(shape[k]))].reshape(shape[k]) for k in TENSORS}


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ---- pieces shared by the two modes -------------------------------------------------------------------------------------------------------
def _pool(a):
    """2x2 max-pool of [n,C,H,W]: the maxima and which of the window's entries (0..3, x fastest) is the first maximum"""
    q = np.stack([a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 0::2], a[..., 1::2, 1::2]], -1)
    return q.max(-1), q.argmax(-1)


def _unpool(e, k):
    d = np.zeros(e.shape[:-2] + (2 * e.shape[-2], 2 * e.shape[-1]), e.dtype)
    for v in range(4):
        d[..., v >> 1::2, v & 1::2] = np.where(k == v, e, 0)
    return d


_EXPF_TAB = np.array([0x3ff0000000000000, 0x3fefd9b0d3158574, 0x3fefb5586cf9890f, 0x3fef9301d0125b51, 0x3fef72b83c7d517b, 0x3fef54873168b9aa, 0x3fef387a6e756238, 0x3fef1e9df51fdee1,
                      0x3fef06fe0a31b715, 0x3feef1a7373aa9cb, 0x3feedea64c123422, 0x3feece086061892d, 0x3feebfdad5362a27, 0x3feeb42b569d4f82, 0x3feeab07dd485429, 0x3feea47eb03a5585,
                      0x3feea09e667f3bcd, 0x3fee9f75e8ec5f74, 0x3feea11473eb0187, 0x3feea589994cce13, 0x3feeace5422aa0db, 0x3feeb737b0cdc5e5, 0x3feec49182a3f090, 0x3feed503b23e255d,
                      0x3feee89f995ad3ad, 0x3feeff76f2fb5e47, 0x3fef199bdd85529c, 0x3fef3720dcef9069, 0x3fef5818dcfba487, 0x3fef7c97337b9b5f, 0x3fefa4afa2a490da, 0x3fefd0765b6e4540], np.uint64)


def _exp32(x):
    """the C library's expf as csrc/ht_expf.hpp restates it, operation for operation in double (2^(k/32) from a table times a polynomial, rounded once);
    beyond its main path (|x| >= 88) the double exponential rounded to float32"""
    xd = np.asarray(x, np.float32).astype(np.float64)
    big = np.abs(xd) >= 88.0
    xs = np.where(big, 0.0, xd)
    z = (float.fromhex("0x1.71547652b82fep+0") * 32) * xs
    kd = z + float.fromhex("0x1.8p+52")
    ki = kd.view(np.uint64)
    r = z - (kd - float.fromhex("0x1.8p+52"))
    s = (_EXPF_TAB[(ki % np.uint64(32)).astype(np.intp)] + (ki << np.uint64(47))).view(np.float64)
    c0, c1, c2 = float.fromhex("0x1.c6af84b912394p-5") / 32 / 32 / 32, float.fromhex("0x1.ebfce50fac4f3p-3") / 32 / 32, float.fromhex("0x1.62e42ff0c52d6p-1") / 32
    y = ((c0 * r + c1) * (r * r) + (c2 * r + 1.0)) * s
    if big.any():
        with np.errstate(over="ignore"):
            y = np.where(big, np.exp(xd), y)
    return y.astype(np.float32)


def _tanh32(x):
    e = _exp32(np.float32(2) * x)      # TanH::f cnn.h:31
    return (e - np.float32(1)) / (e + np.float32(1))


def _seqsum(a, axis=-1):
    """a running sum in the array's own precision, first element first (np.cumsum adds one element at a time)"""
    return np.take(np.cumsum(a, axis=axis, dtype=a.dtype), -1, axis=axis)


def forward(w, X, side, mode="f64", mut=None):
    """the forward pass of every row of X [n, side*side] at the weights w: the layers a3 [n,16,p2,p2], a6 [n,fc], a8 [n,2048], logits, y [n,2304] (and what the
    backward pass needs of it: a1, a5 and the pooling choices k1 k2 k3).  step() calls it, so the inference tests and the training tests share one text.
    `mut` (float64 mode only; tests/test_cnn_forward_ref.py) makes one mistake of a banded or tiled kernel, on whole rows since a single pixel can lose its pooling window:
        conv1_row (ch, r)              conv1's output row r of channel ch misses its ky = 0 taps
        pool_row (ch, r, r_from)       row r of a3's channel ch is taken from row r_from
        conv2_row (oz, r, iz, ky, kx)  conv2's output row r of channel oz misses one tap
        fc1_slab k0 / fc2_block k0     the product misses the 32 / 16 rows of its weights from k0 on
        act3_swap c                    columns c and c + 1 of a8 change places on their way into the last layer
        softmax_sum (c, c_from)        soft-max chunk c is divided by chunk c_from's sum"""
    D = dims(side)
    S, c1, c2, fc = side, D["c1"], D["c2"], D["fc"]
    f32 = mode == "f32"
    mut = mut or {}
    assert not (f32 and mut)
    dt = np.float32 if f32 else np.float64
    w = np.asarray(w, dt)
    P = split(w, side)
    X = np.asarray(X, dt).reshape(-1, S, S)
    n = X.shape[0]
    W1, W2, W3, W4 = P["W1"], P["W2"], P["W3"], P["W4"]
    tanh = _tanh32 if f32 else np.tanh
    # ho_cnn_eval_sized: taps ky, kx (then the input channel), every position of a map at once
    z = np.broadcast_to(P["B1"][None, :, None, None], (n, 16, c1, c1)).copy()
    for ky in range(5):
        for kx in range(5):
            z += X[:, None, ky:ky + c1, kx:kx + c1] * W1[None, :, ky, kx, None, None]
    if "conv1_row" in mut:
        ch, r = mut["conv1_row"]
        for kx in range(5):
            z[:, ch, r] -= X[:, r, kx:kx + c1] * W1[ch, 0, kx]
    a1 = tanh(z)
    a2, k1 = _pool(a1)
    a3, k2 = _pool(a2)
    if "pool_row" in mut:
        ch, r, r_from = mut["pool_row"]
        a3[:, ch, r] = a3[:, ch, r_from]
    z = np.broadcast_to(P["B2"][None, :, None, None], (n, 64, c2, c2)).copy()
    for ky in range(4):
        for kx in range(4):
            for iz in range(16):
                z += a3[:, None, iz, ky:ky + c2, kx:kx + c2] * W2[None, :, iz, ky, kx, None, None]
    if "conv2_row" in mut:
        oz, r, iz, ky, kx = mut["conv2_row"]
        z[:, oz, r] -= a3[:, iz, r + ky, kx:kx + c2] * W2[oz, iz, ky, kx]
    a5 = tanh(z)
    a6m, k3 = _pool(a5)
    a6 = a6m.reshape(n, fc)
    if f32:      # LFull::forward cnn.h:405-429: Y = B, then row i of W times x[i], i ascending
        y7 = np.broadcast_to(P["B3"], (n, 2048)).copy()
        for i in range(fc):
            y7 += a6[:, i, None] * W3[i][None]
        a8 = tanh(y7)
        logits = np.broadcast_to(P["B4"], (n, 2304)).copy()
        for i in range(2048):
            logits += a8[:, i, None] * W4[i][None]
        y = _exp32(logits)
    else:
        xs = a6
        if "fc1_slab" in mut:
            xs = a6.copy(); xs[:, mut["fc1_slab"]:mut["fc1_slab"] + 32] = 0.0
        a8 = np.tanh(P["B3"] + xs @ W3)
        xs = a8
        if "fc2_block" in mut:
            xs = a8.copy(); xs[:, mut["fc2_block"]:mut["fc2_block"] + 16] = 0.0
        if "act3_swap" in mut:
            c = mut["act3_swap"]
            xs = a8.copy(); xs[:, [c, c + 1]] = xs[:, [c + 1, c]]
        logits = P["B4"] + xs @ W4
        y = np.exp(logits)
    sums = [(_seqsum(y[:, b:b + m]) if f32 else y[:, b:b + m].sum(-1)) for b, m in CHUNKS]
    if "softmax_sum" in mut:
        sums[mut["softmax_sum"][0]] = sums[mut["softmax_sum"][1]]
    for (b, m), sm in zip(CHUNKS, sums):
        y[:, b:b + m] /= sm[:, None]
    return dict(a3=a3, a6=a6, a8=a8, logits=logits, y=y, a1=a1, a5=a5, k1=k1, k2=k2, k3=k3)


def step(w, X, T, alpha, side, mode="f64", want_delta=True):
    D = dims(side)
    S, c1, p2, c2, p3, fc = side, D["c1"], D["p2"], D["c2"], D["p3"], D["fc"]
    f32 = mode == "f32"
    dt = np.float32 if f32 else np.float64
    w = np.asarray(w, dt)
    P = split(w, side)
    X = np.asarray(X, dt).reshape(-1, S, S); T = np.asarray(T, dt).reshape(-1, 2304)
    n = X.shape[0]
    alpha = dt(np.float32(alpha))
    one = dt(1)
    W1, W2, W3, W4 = P["W1"], P["W2"], P["W3"], P["W4"]
    F = forward(w, X, side, mode)
    a1, a3, a5, a6, a8, logits, y, k1, k2, k3 = (F[k] for k in ("a1", "a3", "a5", "a6", "a8", "logits", "y", "k1", "k2", "k3"))
    # errors (ho_cnn_train)
    e10 = y - T
    sq = e10 * e10
    mse = (_seqsum(sq) if f32 else sq.sum(-1)) / dt(2304)
    e9 = np.empty((n, 2304), dt)
    for b, m in CHUNKS:
        pr = e10[:, b:b + m] * y[:, b:b + m]
        dp = _seqsum(pr) if f32 else pr.sum(-1)
        e9[:, b:b + m] = y[:, b:b + m] * (e10[:, b:b + m] - dp[:, None])
    if f32:      # LFull::backward cnn.h:430-437: d[i] = sum_j W[i][j] E[j], j ascending
        W4t = np.ascontiguousarray(W4.T); e8 = np.zeros((n, 2048), dt)
        for j in range(2304):
            e8 += W4t[j][None] * e9[:, j, None]
        del W4t
    else:
        e8 = e9 @ W4.T
    e7 = (one - a8 * a8) * e8
    if f32:
        W3t = np.ascontiguousarray(W3.T); e6 = np.zeros((n, fc), dt)
        for j in range(2048):
            e6 += W3t[j][None] * e7[:, j, None]
        del W3t
    else:
        e6 = e7 @ W3.T
    e5 = _unpool(e6.reshape(n, 64, p3, p3), k3)
    e4 = (one - a5 * a5) * e5
    e3 = np.zeros((n, 16, p2, p2), dt)
    if f32:      # LConv::backward cnn.h:236-250: output channel, output y, output x ascending for every input position
        for oz in range(64):
            for ky in range(3, -1, -1):
                for kx in range(3, -1, -1):
                    e3[:, :, ky:ky + c2, kx:kx + c2] += W2[None, oz, :, ky, kx, None, None] * e4[:, oz, None]
    else:      # train_ref.train_step: partial sums over groups of four output channels, then the groups
        part3 = np.zeros((16, n, 16, p2, p2))
        for g in range(16):
            for ky in range(4):
                for kx in range(4):
                    part3[g, :, :, ky:ky + c2, kx:kx + c2] += np.einsum("oi,noyx->niyx", W2[4 * g:4 * g + 4, :, ky, kx], e4[:, 4 * g:4 * g + 4])
        e3 = part3.sum(0)
    e2 = _unpool(e3, k2)
    e1 = _unpool(e2, k1)
    e0 = (one - a1 * a1) * e1
    r = dict(a3=a3, a6=a6, a8=a8, logits=logits, y=y, e9=e9, e7=e7, e6=e6, e3=e3, mse=mse, n=n)
    if not want_delta:
        return r
    # updates: every sample's own step from w, its difference from w added up in float64
    off, shape, count = layout(side)
    delta = np.zeros(count)
    Dl = split(delta, side)
    effect = [dict() for _ in range(n)]

    def conv_diff(Wt, Bt, xin, e, kh):
        """one sample's conv weights and bias after LConv::update (cnn.h:252-279), minus before, float64"""
        if not f32:
            oh = e.shape[-1]
            dW = np.zeros(Wt.shape)
            for ky in range(kh):
                for kx in range(kh):
                    dW[:, :, ky, kx] = -alpha * np.einsum("oyx,iyx->oi", e, xin[:, ky:ky + oh, kx:kx + oh])
            return dW, -alpha * e.sum((1, 2))
        # per weight: the output positions in x-then-y order, W += X * (-alpha * e) one position at a time (positions with e = 0 add a zero)
        win = np.lib.stride_tricks.sliding_window_view(xin, e.shape[-2:], axis=(1, 2))      # [ic, kh, kw, oh, ow]
        s = (-alpha) * e
        oc, ic = Wt.shape[0], Wt.shape[1]
        Wn = np.empty(Wt.shape, np.float32)
        for o in range(oc):
            terms = np.concatenate([Wt[o].reshape(ic * kh * kh, 1), (win * s[o]).reshape(ic * kh * kh, -1)], 1)
            Wn[o] = _seqsum(terms).reshape(Wt.shape[1:])
        Bn = _seqsum(np.concatenate([Bt[:, None], -(e.reshape(oc, -1) * alpha)], 1))
        return np.float64(Wn) - np.float64(Wt), np.float64(Bn) - np.float64(Bt)

    W1s = W1.reshape(16, 1, 5, 5)
    for b in range(n):
        dW1, dB1 = conv_diff(W1s, P["B1"], X[b][None], e0[b], 5)
        dW2, dB2 = conv_diff(W2, P["B2"], a3[b], e4[b], 4)
        Dl["W1"] += dW1.reshape(16, 5, 5); Dl["B1"] += dB1; Dl["W2"] += dW2; Dl["B2"] += dB2
        effect[b].update(W1=float(np.abs(dW1).max()), B1=float(np.abs(dB1).max()), W2=float(np.abs(dW2).max()), B2=float(np.abs(dB2).max()))
    if f32:      # LFull::update cnn.h:438-445: w -= x[i] * e[j] * alpha, B -= e[j] * alpha
        for k, xs, es in (("3", a6, e7), ("4", a8, e9)):
            Wt, Bt = P["W" + k], P["B" + k]
            W64 = np.float64(Wt)
            for b in range(n):
                t = np.multiply.outer(xs[b], es[b]); t *= alpha
                np.subtract(Wt, t, out=t)
                d = t - W64
                Dl["W" + k] += d
                dB = np.float64(Bt - es[b] * alpha) - np.float64(Bt)
                Dl["B" + k] += dB
                effect[b]["W" + k] = float(np.abs(d).max()); effect[b]["B" + k] = float(np.abs(dB).max())
    else:
        for k, xs, es in (("3", a6, e7), ("4", a8, e9)):
            Dl["W" + k] -= alpha * (xs.T @ es); Dl["B" + k] -= alpha * es.sum(0)
            for b in range(n):
                effect[b]["W" + k] = float(alpha * np.abs(xs[b]).max() * np.abs(es[b]).max()); effect[b]["B" + k] = float(alpha * np.abs(es[b]).max())
    r.update(delta=delta, effect=effect)
    return r


def single(w, x, t, alpha, side, mode="f64"):
    """one sample's step as train_ref.train_step names it: its tensors and the stepped weights"""
    r = step(w, x, t, alpha, side, mode)
    out = {k: r[k][0] for k in ("a3", "a6", "a8", "logits", "y", "e9", "e7", "e6", "e3")}
    out["mse"] = float(r["mse"][0])
    out["w"] = np.asarray(w, np.float64) + r["delta"]
    out.update(split(out["w"], side))
    return out


# ---- samples and batches at side 128 ----------------------------------------------------------------------------------------------------
T5 = ["f0", "z0", "z1", "x0", "f9"]
STEP2 = ["f33", "f60", "x1", "x2", "x3"]
BATCHES = {
    "T1": dict(w="seed", pool=["x0"], order=None, batch=1, alpha=0.001),
    "T5": dict(w="seed", pool=T5, order=None, batch=5, alpha=0.001),
    "T5r": dict(w="seed", pool=T5, order=[0, 3, 3, 1, 4], batch=5, alpha=0.001),
    "T33": dict(w="seed", pool=T5 + ["f33", "f60"] + ["x%d" % i for i in range(1, 27)], order=None, batch=33, alpha=0.001),
    "Td": dict(w="sat", pool=["x0", "x1"], order=None, batch=2, alpha=0.001),
    "T5x2": dict(w="seed", pool=T5 + STEP2, order=None, batch=5, alpha=0.001),
    "T5x2stale": dict(w="seed", pool=STEP2, order=None, batch=5, alpha=0.001),
}
GPU_BATCHES = ("T1", "T5", "T5r", "T33", "Td", "T5x2")
FRAMES = (0, 9, 33, 60)      # of tests/golden/frames5_64.npz, as tests/test_cnn128.py
_cache = {}


def _frames():
    if "frames" not in _cache:
        from hand_tracking_samples_amd import native
        L = native.load()
        z = np.load(os.path.join(HERE, "golden", "frames5_64.npz"))
        fp = C.POINTER(C.c_float)
        out = {}
        for f in FRAMES:
            x = _tile_input(z["depth"][f], z["cam"][f][4])
            cam = np.array(z["cam"][f], np.float32); cam[:4] *= np.float32(0.5)      # camsub(cam, 8) = camsub of the halved camera by 4
            pose = np.ascontiguousarray(z["startpose"][f], np.float32)
            t = np.zeros(2304, np.float32)
            assert L.ht_expected_cnn(pose.ctypes.data_as(fp), cam.ctypes.data_as(fp), t.ctypes.data_as(fp)) == 0
            out["f%d" % f] = (x, t)
        _cache["frames"] = out
    return _cache["frames"]


def sample(name):
    """(input [16384], target [2304]) float32"""
    if name[0] == "f":
        return _frames()[name]
    if name in ("z0", "z1"):
        return np.full(16384, 0.0 if name == "z0" else 1.0, np.float32), _frames()["f33" if name == "z0" else "f60"][1]
    rng = np.random.default_rng(100 + int(name[1:]))
    return rng.random(16384).astype(np.float32), rng.random(2304).astype(np.float32)


# ---- the inference nets' cases (tests/test_cnn_forward_ref.py, tests/test_gpu_cnn_forward.py) ---------------------------------------------
FWD_TENSORS = ("a3", "a6", "a8", "logits", "y")
FWD_SEED = ("f0", "f9", "z0", "z1", "x0", "x1")      # on the seeded weights
FWD_SAT = ("x0", "x1")                               # on the weights scaled as batch Td (side 128) / case d (side 64) scales them: "Td:x0", "Td:x1"
FWD_CASES = FWD_SEED + tuple("Td:" + s for s in FWD_SAT)


def _tile_input(depth, dscale):
    """ho_cnn_input, handtrack.h:700, float32 operation for operation"""
    d = np.asarray(depth).reshape(-1).astype(np.float32) * np.float32(dscale)
    v = np.float32(1) - (d - np.float32(0.1)) / (np.float32(0.7) - np.float32(0.1))
    return np.minimum(np.maximum(v, np.float32(0)), np.float32(1)).astype(np.float32)


def forward_input(name, side):
    """the input [side*side] float32 of a sample: sample(name)[0] at side 128; at side 64 "f<k>" is tile k of tests/golden/frames256.npz, the others the same
    constructions on 4096 values.  No labels, so no library is needed."""
    n = side * side
    if name[0] == "f":
        z = np.load(os.path.join(HERE, "golden", "frames5_64.npz" if side == 128 else "frames256.npz"))
        k = int(name[1:])
        return _tile_input(z["depth"][k], z["cam"][k][4])
    if name in ("z0", "z1"):
        return np.full(n, 0.0 if name == "z0" else 1.0, np.float32)
    return np.random.default_rng(100 + int(name[1:])).random(n).astype(np.float32)


def forward_weights(key, w, side):
    """"seed": w itself; "sat": start_weights("sat") at side 128, train_ref's case d (W1 and W2 times SAT_SCALE) at side 64"""
    if key == "seed":
        return np.array(w, np.float32, copy=True)
    if side == 128:
        return start_weights("sat", w)
    import train_ref
    off, _, _ = layout(64)
    w = np.array(w, np.float32, copy=True)
    w[off["W1"]:off["B1"]] *= np.float32(train_ref.SAT_SCALE); w[off["W2"]:off["B2"]] *= np.float32(train_ref.SAT_SCALE)
    return w


def forward_bounds(f64, f32):
    """per tensor the rule's bound of every row: 4 d32 + 4 * 2^-24 max|T_64|, and d32"""
    out = {}
    for T in FWD_TENSORS:
        a, b = np.asarray(f64[T], np.float64).reshape(len(f64[T]), -1), np.asarray(f32[T], np.float64).reshape(len(f64[T]), -1)
        d32 = np.abs(a - b).max(1)
        out[T] = (4.0 * d32 + 4.0 * 2.0 ** -24 * np.abs(a).max(1), d32)
    return out


def forward_references(side, w):
    """the eight cases of a side at the seeded weights w of that side: names, X [8, side*side], which weights a case runs on, and per case (row) the float64 forward, the
    float32 forward in the reference's order and the rule's bound per tensor.  Computed once per side and not to be modified."""
    key = ("fwd", side)
    if key not in _cache:
        X = np.stack([forward_input(s.split(":")[-1], side) for s in FWD_CASES])
        wkey = ["sat" if s.startswith("Td:") else "seed" for s in FWD_CASES]
        f64 = {T: [None] * len(FWD_CASES) for T in FWD_TENSORS}; f32 = {T: [None] * len(FWD_CASES) for T in FWD_TENSORS}
        for k in ("seed", "sat"):
            rows = [i for i, q in enumerate(wkey) if q == k]
            wk = forward_weights(k, w, side)
            a, b = forward(np.float64(wk), X[rows], side, "f64"), forward(wk, X[rows], side, "f32")
            for T in FWD_TENSORS:
                for j, i in enumerate(rows):
                    f64[T][i] = np.asarray(a[T][j]).reshape(-1); f32[T][i] = np.asarray(b[T][j]).reshape(-1)
        f64 = {T: np.stack(v) for T, v in f64.items()}; f32 = {T: np.stack(v) for T, v in f32.items()}
        bd = forward_bounds(f64, f32)
        _cache[key] = dict(names=FWD_CASES, X=X, wkey=wkey, f64=f64, f32=f32, bound={T: bd[T][0] for T in FWD_TENSORS}, d32={T: bd[T][1] for T in FWD_TENSORS})
    return _cache[key]


def start_weights(key, w128):
    w = np.array(w128, np.float32, copy=True)
    if key == "sat":
        off, _, _ = layout(128)
        w[off["W1"]:off["B1"]] *= np.float32(SAT_SCALE128); w[off["W2"]:off["B2"]] *= np.float32(SAT_SCALE128); w[off["W3"]:off["B3"]] *= np.float32(SAT_FC1_SCALE128)
    return w


def sequence(name):
    """the samples of a batch in the order they are trained on, and its steps as (first, last) positions of that sequence"""
    B = BATCHES[name]
    seq = [B["pool"][i] for i in B["order"]] if B["order"] is not None else list(B["pool"])
    return seq, [(k, min(k + B["batch"], len(seq))) for k in range(0, len(seq), B["batch"])]


def pool_arrays(name):
    xt = [sample(s) for s in BATCHES[name]["pool"]]
    return np.stack([x for x, _ in xt]), np.stack([t for _, t in xt])


def one_step(w64, w32, names, alpha, side=128, samples=None):
    """a step record: w64 / w32 after the step, d32 and bound per weight tensor, per position of the step its tensors (float64), their bounds and its effect"""
    xt = samples if samples is not None else [sample(s) for s in names]
    X = np.stack([x for x, _ in xt]); T = np.stack([t for _, t in xt])
    f = step(w64, X, T, alpha, side, "f64")
    o = step(w32, X, T, alpha, side, "f32")
    e64 = np.asarray(w64, np.float64) + f.pop("delta")
    e32 = np.float64(w32) + o.pop("delta")
    P, Q = split(e64, side), split(e32, side)
    d32 = {k: dist(Q[k], P[k]) for k in TENSORS}
    bound = {k: 4.0 * d32[k] + 4.0 * 2.0 ** -24 * float(np.abs(P[k]).max()) for k in TENSORS}
    recs = []
    for b in range(len(xt)):
        ten = {k: np.array(f[k][b]) for k in PER_SAMPLE}
        bnd = {k: 4.0 * dist(o[k][b], f[k][b]) + 4.0 * 2.0 ** -24 * float(np.abs(f[k][b]).max()) for k in PER_SAMPLE}
        recs.append(dict(tensors=ten, bound=bnd, effect=f["effect"][b], a8_32=np.array(o["a8"][b]), finite32=bool(all(np.isfinite(o[k][b]).all() for k in PER_SAMPLE))))
    return dict(w64=e64, w32=e32.astype(np.float32), d32=d32, bound=bound, samples=recs, names=list(names))


def references(names, w128):
    """{batch: [step record, ...]}; the steps of a call one after the other, each from the step before it"""
    for n in names:
        if n in _cache:
            continue
        B = BATCHES[n]
        seq, steps = sequence(n)
        w32 = start_weights(B["w"], w128); w64 = np.float64(w32)
        out = []
        for a, b in steps:
            key = ("first", B["w"], tuple(seq[a:b]), B["alpha"]) if a == 0 else None      # a call's first step is shared by the batches that begin alike (T5, T5x2)
            if key not in _cache:
                _cache[key] = one_step(w64, w32, seq[a:b], B["alpha"])
            out.append(_cache[key])
            w64, w32 = out[-1]["w64"], out[-1]["w32"]
        _cache.pop(None, None)
        _cache[n] = out
    return {n: _cache[n] for n in names}
