"""The optimiser step of csrc/ht_optim.hip (ht_cnn_opt_step_sized_dev) restated in numpy.  A helper, not a test; it needs no GPU and no library.

step(w, G, m, v, t, o, side, mode="f32") applies one step of the optimiser o (a dict of ht_opt's fields; opt() fills ht_opt_default's values) to all weights of a
net in .cnnb order and returns (w', m', v', t', norm, c):
    mode "f32"   np.float32 arrays and np.float32 scalars throughout, one rounding per written operation, in the order the header comment of csrc/ht_optim.hip gives;
                 omb1 / omb2 formed in float32, bc1 / bc2 from Python doubles (1.0 - beta ** t') rounded to float32, the clip factor from a float64 np.sum
    mode "f64"   the same formulas in float64 (the float32 options widened), the yardstick of tests/test_optim_ref.py
`c` may be given (the device's own reported factor); otherwise it is derived from G.  `fault` seeds one mistake (tests/test_optim_ref.py shows that each changes bits
on the test state):
    "decay_bias"     decay applied to the bias ranges too
    "no_bias_corr"   Adam's bias correction skipped (bc1 = bc2 = 1)
    "t_stuck"        t not advanced before the bias correction
    "scale_after"    grad_scale applied after the clip test instead of before (the norm is taken of G itself)
    "plain_momentum" Nesterov written as plain momentum
seed_state(side, seed) is the state the GPU test seeds the device with."""
import numpy as np

import train_ref_sized as ts

SGD, MOMENTUM, NESTEROV, ADAM = 0, 1, 2, 3
KINDS = {"sgd": SGD, "momentum": MOMENTUM, "nesterov": NESTEROV, "adam": ADAM}
_F = np.float32


def opt(kind, **kw):
    """ht_opt_default's values, then the fields given; the floats as np.float32"""
    o = dict(kind=KINDS.get(kind, kind), lr=0.001, momentum=0.9, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled_decay=0, grad_scale=1.0, clip_norm=0.0)
    o.update(kw)
    return {k: (v if k in ("kind", "decoupled_decay") else _F(v)) for k, v in o.items()}


def weight_mask(side):
    """True where an element of the .cnnb order belongs to W1 W2 W3 W4"""
    off, shape, count = ts.layout(side)
    mask = np.zeros(count, bool)
    for k in ("W1", "W2", "W3", "W4"):
        mask[off[k]:off[k] + int(np.prod(shape[k]))] = True
    return mask


def clip_factor(G, o, fault=None):
    """(norm, c): norm = sqrt(SUM ((double)G * (double)gs)^2) in float64, c = norm > clip_norm ? (float)(clip_norm / norm) : 1.0f; clipping off: (-1, 1)"""
    if not float(o["clip_norm"]) > 0.0:
        return -1.0, _F(1)
    x = np.asarray(G, np.float64) * (1.0 if fault == "scale_after" else float(o["grad_scale"]))
    norm = float(np.sqrt(np.sum(x * x)))
    clip = float(o["clip_norm"])
    return norm, (_F(clip / norm) if norm > clip else _F(1))


def step(w, G, m, v, t, o, side, mode="f32", c=None, fault=None):
    dt = np.float32 if mode == "f32" else np.float64
    S = lambda x: dt(x)      # a float32 option as a scalar of the mode
    w = np.array(w, dt); G = np.asarray(G, dt)
    m = np.zeros_like(w) if m is None else np.array(m, dt); v = np.zeros_like(w) if v is None else np.array(v, dt)
    norm, c_own = clip_factor(G, o, fault)
    c = c_own if c is None else _F(c)
    kind = o["kind"]
    isw = np.ones(w.size, bool) if fault == "decay_bias" else weight_mask(side)
    wd = S(o["weight_decay"])
    g = (G * S(o["grad_scale"])) * S(c)
    if not o["decoupled_decay"] and float(o["weight_decay"]) != 0.0:
        g = np.where(isw, g + wd * w, g)
    lr = S(o["lr"])
    if kind == SGD:
        w = w - lr * g
    elif kind in (MOMENTUM, NESTEROV):
        mu = S(o["momentum"])
        m = mu * m + g
        w = w - lr * m if (kind == MOMENTUM or fault == "plain_momentum") else w - lr * (g + mu * m)
    else:
        t1 = t if fault == "t_stuck" else t + 1
        t = t + 1
        b1, b2 = S(o["beta1"]), S(o["beta2"])
        omb1, omb2 = dt(1) - b1, dt(1) - b2
        if fault == "no_bias_corr":
            bc1 = bc2 = dt(1)
        else:
            with np.errstate(divide="ignore"):
                bc1 = dt(_F(1.0 - float(o["beta1"]) ** t1) if mode == "f32" else 1.0 - float(o["beta1"]) ** t1)
                bc2 = dt(_F(1.0 - float(o["beta2"]) ** t1) if mode == "f32" else 1.0 - float(o["beta2"]) ** t1)
        m = b1 * m + omb1 * g
        v = b2 * v + (omb2 * g) * g
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (m / bc1) / (np.sqrt(v / bc2) + S(o["eps"]))
        if o["decoupled_decay"]:
            u = np.where(isw, u + wd * w, u)
        w = w - lr * u
    assert w.dtype == dt and m.dtype == dt and v.dtype == dt
    return w, m, v, t, norm, c


_grad_cache = {}


def grad_reference(key, w32, X, T, side):
    """The gradient yardstick of a batch at the float32 weights w32: train_ref_sized.step(w, X, T, alpha=1.0, side, mode), whose delta is -SUM_b g_b(w) (a product
    with 1 is exact).  G64 from the float64 mode, G32 from the float32 mode (the reference's own order), per tensor d32 = max|G32 - G64| and the rule's
    bound 4 d32 + 4 * 2^-24 max|G64|, the float64 losses with their bounds, and per sample how far it moves each tensor.  Cached under `key`; not to be modified."""
    if key not in _grad_cache:
        f = ts.step(np.float64(w32), X, T, 1.0, side, "f64")
        o = ts.step(np.asarray(w32, np.float32), X, T, 1.0, side, "f32")
        G64, G32 = -f["delta"], -o["delta"]
        P, Q = ts.split(G64, side), ts.split(G32, side)
        d32 = {k: ts.dist(Q[k], P[k]) for k in ts.TENSORS}
        bound = {k: 4.0 * d32[k] + 4.0 * 2.0 ** -24 * float(np.abs(P[k]).max()) for k in ts.TENSORS}
        mse_bound = 4.0 * np.abs(np.float64(o["mse"]) - f["mse"]) + 4.0 * 2.0 ** -24 * np.abs(f["mse"])
        _grad_cache[key] = dict(G64=G64, G32=G32, d32=d32, bound=bound, mse=np.array(f["mse"]), mse_bound=mse_bound, effect=f["effect"])
    return _grad_cache[key]


def seed_state(side, seed=7):
    """(w, G, m, v): random from a fixed seed; v >= 0; a stretch with G = m = v = 0 across the B1 / W2 boundary, gradients around 1e-20 and around 1e3 in W3 and in B4"""
    off, shape, count = ts.layout(side)
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(count, np.float32) * _F(0.05)).astype(np.float32)
    G = (rng.standard_normal(count, np.float32) * _F(0.3)).astype(np.float32)
    m = (rng.standard_normal(count, np.float32) * _F(0.1)).astype(np.float32)
    v = (rng.random(count, np.float32) * _F(0.01)).astype(np.float32)
    G[390:440] = 0; m[390:440] = 0; v[390:440] = 0
    a = off["W3"] + 1001
    G[a:a + 64] *= _F(1e-20 / 0.3); G[a + 64:a + 128] *= _F(1e3 / 0.3)
    b = off["B4"] + 5
    G[b:b + 8] *= _F(1e-20 / 0.3); G[b + 8:b + 16] *= _F(1e3 / 0.3)
    return w, G, m, v
