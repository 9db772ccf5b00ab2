"""A float64 restatement of one CNN::Train step (cnn.h:558-580) on .cnnb-ordered weights, written from oracle/ho_cnn.c (ho_cnn_eval_sized,
ho_cnn_train), and the table of cases the training kernels (csrc/ht_train.hip) are checked on.  Test infrastructure only.

train_step() returns every forward layer output, every backward error, the loss and the stepped weights, all float64.  Every position of a
convolution is summed in the same order (a loop over taps on whole maps), so equal inputs give equal outputs and a constant tile is a tie in
every pooling window, as it is in float32.  Max-pool backward gives the error to the first maximum in x-then-y order (np.argmax returns the
first occurrence, which is what the oracle's strict `>` scan keeps).

`mut` drops one term the way a kernel bug would (tests/test_train_ref.py shows that each moves its tensor far beyond the comparison rule):
  conv1_tap (oz, ky, kx) / conv2_tap (oz, iz, ky, kx)   the forward convolution of one output channel misses one tap
  conv1_bias oz                                          ... or its bias
  fc1_slab ks / fc2_slab ks                              the forward product misses one of the 32 split-K row slabs
  chunk_dp c                                             soft-max backward of chunk c misses its dot product dp
  w4_trip i / w3_trip i                                  the backward product of row i misses its last 256-column trip
  fold_row i                                             (1 - x^2) is not applied to row i of the error under FC2
  part3_group g                                          conv2's backward misses the four output channels of group g
  pool3 (oz, p) / pool2 (c, p) / pool1 (c, p)            one pooling window (p: flat index of the pooled map) routes the error to its second maximum
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (57600, 57600, 14400, 3600, 9216, 9216, 2304, 2048, 2048, 2304, 2304)      # CNN::Eval's layer outputs
NW3, NW4 = 2304 * 2048, 2048 * 2304
OFF = {"W1": 0, "B1": 400, "W2": 416, "B2": 16800, "W3": 16864, "B3": 16864 + NW3, "W4": 16864 + NW3 + 2048, "B4": 16864 + NW3 + 2048 + NW4}
SHAPE = {"W1": (16, 5, 5), "B1": (16,), "W2": (64, 16, 4, 4), "B2": (64,), "W3": (2304, 2048), "B3": (2048,), "W4": (2048, 2304), "B4": (2304,)}
COUNT = OFF["B4"] + 2304
CHUNKS = [(256 * c, 256) for c in range(8)] + [(2048 + 16 * c, 16) for c in range(16)]      # LSoftMaxChunked of handtrack.h:118
KSPLIT, GROUPS = 32, 16


def split(w):
    """named views of a flat .cnnb weight vector (conv W index = kx + KW*(ky + KH*(ic + IC*oc)))"""
    return {k: w[OFF[k]:OFF[k] + int(np.prod(SHAPE[k]))].reshape(SHAPE[k]) for k in OFF}


def _pool(a):
    """2x2 max-pool of [C,H,W]: the maxima and which of the window's entries (0..3, x fastest) is the first maximum"""
    q = np.stack([a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]], -1)
    return q.max(-1), q.argmax(-1), q


def _second(q, c, p):
    """index of the second maximum of window p of channel c (the later one of equal values)"""
    v = q.reshape(q.shape[0], -1, 4)[c, p]
    return int(np.argsort(-v, kind="stable")[1])


def _unpool(e, k):
    d = np.zeros((e.shape[0], 2 * e.shape[1], 2 * e.shape[2]))
    for v in range(4):
        d[:, v >> 1::2, v & 1::2] = np.where(k == v, e, 0.0)
    return d


def _route(name, mut, q, k):
    if name in mut:
        c, p = mut[name]
        k = k.copy(); k.reshape(k.shape[0], -1)[c, p] = _second(q, c, p)
    return k


def train_step(w, x, t, alpha, mut=None, fc_update=True):
    mut = mut or {}
    w = np.asarray(w, np.float64)
    P = split(w)
    x = np.asarray(x, np.float64).reshape(64, 64); t = np.asarray(t, np.float64).reshape(2304)
    alpha = float(np.float32(alpha))
    W1, W2, W3, W4 = P["W1"], P["W2"], P["W3"], P["W4"]
    r = {}
    # forward (ho_cnn_eval_sized)
    W1f = W1
    if "conv1_tap" in mut:
        W1f = W1.copy(); W1f[mut["conv1_tap"]] = 0.0
    z = np.broadcast_to(P["B1"][:, None, None], (16, 60, 60)).copy()
    if "conv1_bias" in mut:
        z[mut["conv1_bias"]] = 0.0
    for ky in range(5):
        for kx in range(5):
            z += x[None, ky:ky + 60, kx:kx + 60] * W1f[:, ky, kx, None, None]
    a1 = np.tanh(z)
    a2, k1, q1 = _pool(a1)
    a3, k2, q2 = _pool(a2)
    W2f = W2
    if "conv2_tap" in mut:
        W2f = W2.copy(); W2f[mut["conv2_tap"]] = 0.0
    z = np.broadcast_to(P["B2"][:, None, None], (64, 12, 12)).copy()
    for ky in range(4):
        for kx in range(4):
            for iz in range(16):
                z += a3[None, iz, ky:ky + 12, kx:kx + 12] * W2f[:, iz, ky, kx, None, None]
    a5 = np.tanh(z)
    a6m, k3, q3 = _pool(a5)
    a6 = a6m.reshape(2304)
    xs = a6
    if "fc1_slab" in mut:
        xs = a6.copy(); xs[72 * mut["fc1_slab"]:72 * (mut["fc1_slab"] + 1)] = 0.0
    a8 = np.tanh(P["B3"] + xs @ W3)
    xs = a8
    if "fc2_slab" in mut:
        xs = a8.copy(); xs[64 * mut["fc2_slab"]:64 * (mut["fc2_slab"] + 1)] = 0.0
    logits = P["B4"] + xs @ W4
    y = np.exp(logits)
    for b, n in CHUNKS:
        y[b:b + n] /= y[b:b + n].sum()
    r.update(a1=a1, a2=a2, a3=a3, a5=a5, a6=a6, a8=a8, logits=logits, y=y)
    # errors (ho_cnn_train)
    e10 = y - t
    mse = float((e10 * e10).sum() / 2304)
    e9 = np.empty(2304)
    for c, (b, n) in enumerate(CHUNKS):
        dp = 0.0 if mut.get("chunk_dp") == c else (e10[b:b + n] * y[b:b + n]).sum()
        e9[b:b + n] = y[b:b + n] * (e10[b:b + n] - dp)
    e8 = W4 @ e9
    if "w4_trip" in mut:
        i = mut["w4_trip"]; e8[i] = W4[i, :2048] @ e9[:2048]
    fold = 1.0 - a8 * a8
    if "fold_row" in mut:
        fold[mut["fold_row"]] = 1.0
    e7 = fold * e8
    e6 = W3 @ e7
    if "w3_trip" in mut:
        i = mut["w3_trip"]; e6[i] = W3[i, :1792] @ e7[:1792]
    e5 = _unpool(e6.reshape(64, 6, 6), _route("pool3", mut, q3, k3))
    e4 = (1.0 - a5 * a5) * e5
    part3 = np.zeros((GROUPS, 16, 15, 15))
    for g in range(GROUPS):
        if mut.get("part3_group") == g:
            continue
        for ky in range(4):
            for kx in range(4):
                part3[g, :, ky:ky + 12, kx:kx + 12] += np.einsum("oi,oyx->iyx", W2[4 * g:4 * g + 4, :, ky, kx], e4[4 * g:4 * g + 4])
    e3 = part3.sum(0)
    e2 = _unpool(e3, _route("pool2", mut, q2, k2))
    e1 = _unpool(e2, _route("pool1", mut, q1, k1))
    e0 = (1.0 - a1 * a1) * e1
    r.update(e10=e10, mse=mse, e9=e9, e8=e8, e7=e7, e6=e6, e5=e5, e4=e4, part3=part3, e3=e3, e2=e2, e1=e1, e0=e0)
    # updates
    wn = w.copy() if fc_update else w[:OFF["W3"]].copy()
    N = split(wn) if fc_update else {k: wn[OFF[k]:OFF[k] + int(np.prod(SHAPE[k]))].reshape(SHAPE[k]) for k in ("W1", "B1", "W2", "B2")}
    for ky in range(5):
        for kx in range(5):
            N["W1"][:, ky, kx] -= alpha * np.einsum("oyx,yx->o", e0, x[ky:ky + 60, kx:kx + 60])
    N["B1"] -= alpha * e0.sum((1, 2))
    for ky in range(4):
        for kx in range(4):
            N["W2"][:, :, ky, kx] -= alpha * np.einsum("oyx,iyx->oi", e4, a3[:, ky:ky + 12, kx:kx + 12])
    N["B2"] -= alpha * e4.sum((1, 2))
    if fc_update:
        N["W3"] -= alpha * np.outer(a6, e7); N["B3"] -= alpha * e7
        N["W4"] -= alpha * np.outer(a8, e9); N["B4"] -= alpha * e9
    r["w"] = wn
    for k in ("W1", "B1", "W2", "B2"):
        r[k] = N[k]
    return r


# ---- the oracle's own float32 step with its intermediates --------------------------------------------------------------------------------
def oracle_step(w, x, t, alpha):
    """ho_cnn_train_layers on a copy of w: the same names as train_step, float32"""
    import oracle_lib as ol
    w = np.array(w, np.float32, copy=True)
    outs = [np.zeros(n, np.float32) for n in SIZES]; errs = [np.zeros(n, np.float32) for n in SIZES]
    fp = C.POINTER(C.c_float)
    mse = ol.lib().ho_cnn_train_layers(ol.fptr(w), ol.fptr(np.ascontiguousarray(x, np.float32).reshape(-1)), ol.fptr(np.ascontiguousarray(t, np.float32).reshape(-1)), float(alpha),
                                       (fp * 11)(*[ol.fptr(a) for a in outs]), (fp * 11)(*[ol.fptr(a) for a in errs]))
    r = dict(a1=outs[1].reshape(16, 60, 60), a2=outs[2].reshape(16, 30, 30), a3=outs[3].reshape(16, 15, 15), a5=outs[5].reshape(64, 12, 12), a6=outs[6], a8=outs[8],
             logits=outs[9], y=outs[10], e10=errs[10], e9=errs[9], e8=errs[8], e7=errs[7], e6=errs[6], e5=errs[5].reshape(64, 12, 12), e4=errs[4].reshape(64, 12, 12),
             e3=errs[3].reshape(16, 15, 15), e2=errs[2].reshape(16, 30, 30), e1=errs[1].reshape(16, 60, 60), e0=errs[0].reshape(16, 60, 60), mse=float(mse), w=w)
    r.update(split(w))
    return r


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# what the device's tensors are compared on ("e3" is the device's sum_g part3[g])
COMPARED = ("a1", "a3", "a5", "a6", "a8", "e9", "e7", "e6", "e3", "mse", "W1", "B1", "W2", "B2")
# name -> (weight scale of the two convolutions, input, target, alpha); "b" is two cases, one per constant
CASES = ("a", "b0", "b1", "c", "d", "e")
SAT_SCALE = 8.0      # case d: W1 and W2 times this; tests/test_train_ref.py asserts that the oracle stays finite and reaches exact +-1.0f
_cache = {}


def _fixture():
    if "G" not in _cache:
        import htfx
        import oracle_lib as ol
        G = htfx.load(os.path.join(HERE, "golden", "train3.htfx"))
        xs = []
        for f in range(3):
            x = np.zeros(4096, np.float32)
            ol.lib().ho_cnn_input(ol.u16ptr(np.ascontiguousarray(G["f%d/depth" % f].reshape(-1))), 4096, float(G["f%d/cam" % f][4]), 0.1, 0.7, ol.fptr(x))
            xs.append(x)
        _cache["G"] = (xs, [np.ascontiguousarray(G["f%d/labels" % f], np.float32) for f in range(3)])
    return _cache["G"]


def case(name, weights):
    """(weights, input [4096], target [2304], alpha) of a case, float32; `weights` is the seeded set of the suite's fixture"""
    xs, ts = _fixture()
    w = np.array(weights, np.float32, copy=True)
    dense_x = np.random.default_rng(11).random(4096).astype(np.float32); dense_t = np.random.default_rng(12).random(2304).astype(np.float32)
    if name == "a":
        return w, xs[0], ts[0], 0.001
    if name in ("b0", "b1"):
        return w, np.full(4096, 0.0 if name == "b0" else 1.0, np.float32), ts[1], 0.001
    if name == "c":
        return w, dense_x, dense_t, 0.001
    if name == "d":
        w[OFF["W1"]:OFF["B1"]] *= np.float32(SAT_SCALE); w[OFF["W2"]:OFF["B2"]] *= np.float32(SAT_SCALE)
        return w, dense_x, dense_t, 0.001
    if name == "e":
        return w, xs[2], ts[2], 0.25
    raise KeyError(name)


def reference(name, weights):
    """(float64 step, oracle's float32 step) of a case, computed once per session and not to be modified"""
    if name not in _cache:
        w, x, t, alpha = case(name, weights)
        _cache[name] = (train_step(w, x, t, alpha), oracle_step(w, x, t, alpha))
    return _cache[name]


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def bound(name, tensor, weights):
    """the rule of the layer tests: 4 * d_orc(T) + 4 * 2^-24 * max|T_f64|, d_orc = the oracle's own float32 distance from float64"""
    f64, o32 = reference(name, weights)
    return 4.0 * dist(o32[tensor], f64[tensor]) + 4.0 * 2.0 ** -24 * float(np.abs(f64[tensor]).max())
