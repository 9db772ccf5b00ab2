"""The numpy restatement of the optimiser step (tests/optim_ref.py) and the gradient yardstick the GPU test uses (tests/test_gpu_optim.py).  CPU only.

Shown here: the float32 restatement stays within a few float32 spacings of |w| of the same formulas in float64, for every kind; a norm below the threshold gives
a clip factor of exactly 1.0f; each of five seeded faults changes at least one weight's bits on the state the GPU test uses; the gradient yardstick
(train_ref_sized.step at alpha = 1) is alpha-free, and a forgotten sample or a repeat counted once lands far outside the rule's bound."""
import numpy as np
import pytest

import optim_ref as orf
import train_batch_ref as tb
import train_ref_sized as ts

KINDS = ("sgd", "momentum", "nesterov", "adam")


@pytest.fixture(scope="module")
def state():
    return orf.seed_state(64)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", KINDS)
def test_float32_restatement_stays_near_float64(kind, state):
    """Two steps.  The distance is counted in float32 spacings (2^-23 relative) of the largest quantity an element's step passes through: |w| before and after, the
    step itself, lr |g| and lr |m'| (the terms of Nesterov's sum can cancel).  A step is at most ten rounded operations per element, each off by at most half a
    spacing of its result, and the second step starts from the first's error: at most ten spacings over the two steps, 16 being the next power of two."""
    w, G, m, v = state
    o = orf.opt(kind, weight_decay=0.01, grad_scale=1.0 / 64)
    a = (w, m, v, 3); b = (np.float64(w), np.float64(m), np.float64(v), 3)
    lr = float(o["lr"])
    scale = np.abs(np.float64(w))
    for k in range(2):
        a = orf.step(a[0], G, a[1], a[2], a[3], o, 64, "f32")[:4]
        before = b[0]
        b = orf.step(b[0], G, b[1], b[2], b[3], o, 64, "f64")[:4]
        for q in (np.abs(b[0]), np.abs(b[0] - before), lr * np.abs(np.float64(G) / 64.0 + 0.01 * before), lr * np.abs(b[1])):
            scale = np.maximum(scale, q)
        ulps = np.abs(np.float64(a[0]) - b[0]) / (np.maximum(scale, 2.0 ** -126) * 2.0 ** -23)
        print("%s step %d: float32 within %.2f float32 spacings of float64 (t = %d)" % (kind, k + 1, ulps.max(), a[3]))
        assert ulps.max() <= 16.0 and a[3] == b[3] == (3 + k + 1 if kind == "adam" else 3)


def test_a_norm_below_the_threshold_does_not_clip(state):
    w, G, m, v = state
    norm = float(np.sqrt(np.sum((np.float64(G) / 64.0) ** 2)))
    below, above = orf.opt("sgd", grad_scale=1.0 / 64, clip_norm=norm * 1.01), orf.opt("sgd", grad_scale=1.0 / 64, clip_norm=norm * 0.5)
    n1, c1 = orf.clip_factor(G, below)
    n2, c2 = orf.clip_factor(G, above)
    assert c1.dtype == np.float32 and _bits(c1) == _bits(np.float32(1)) and abs(n1 - norm) <= 1e-12 * norm
    assert c2 < 1 and abs(float(c2) - 0.5) <= 2.0 ** -23 and n2 == n1
    off = orf.clip_factor(G, orf.opt("sgd", grad_scale=1.0 / 64))
    assert off[0] == -1.0 and _bits(off[1]) == _bits(np.float32(1))
    assert np.array_equal(_bits(orf.step(w, G, m, v, 0, below, 64)[0]), _bits(orf.step(w, G, m, v, 0, orf.opt("sgd", grad_scale=1.0 / 64), 64)[0]))


@pytest.mark.parametrize("fault,kind,kw,t", [
    ("decay_bias", "sgd", dict(weight_decay=0.01), 0), ("decay_bias", "adam", dict(weight_decay=0.01, decoupled_decay=1), 0),
    ("no_bias_corr", "adam", {}, 0), ("t_stuck", "adam", {}, 7), ("scale_after", "momentum", dict(clip_norm=60.0), 0), ("plain_momentum", "nesterov", {}, 0)])
def test_a_seeded_fault_changes_bits(fault, kind, kw, t, state):
    w, G, m, v = state
    if "clip_norm" in kw:      # eight times the norm of G / 64: below the norm of G itself
        kw = dict(kw, clip_norm=8.0 * float(np.sqrt(np.sum((np.float64(G) / 64.0) ** 2))))
    o = orf.opt(kind, grad_scale=1.0 / 64, **kw)
    good = orf.step(w, G, m, v, t, o, 64)
    bad = orf.step(w, G, m, v, t, o, 64, fault=fault)
    changed = int((_bits(good[0]) != _bits(bad[0])).sum())
    print("%s in %s: %d of %d weights change bits" % (fault, kind, changed, w.size))
    assert changed >= 1
    if fault == "decay_bias":      # and only biases do
        assert not (_bits(good[0]) != _bits(bad[0]))[orf.weight_mask(64)].any()
    if fault == "scale_after":     # the state's norm sits between the two readings of the threshold
        assert good[5] == np.float32(1) and bad[5] < 1


# ---- the gradient yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s5(weights):
    x, t = tb.pool_arrays("S5", weights)
    return x, t, orf.grad_reference("S5", tb.start_weights("seed", weights), x, t, 64)


def test_the_yardstick_does_not_depend_on_alpha(s5, weights):
    x, t, ref = s5
    w = np.float64(tb.start_weights("seed", weights))
    lo = ts.step(w, x, t, 0.001, 64, "f64")["delta"] / -np.float64(np.float32(0.001))
    P, Q = ts.split(ref["G64"], 64), ts.split(lo, 64)
    for T in ts.TENSORS:
        rel = ts.dist(P[T], Q[T]) / float(np.abs(P[T]).max())
        print("%s: -delta(alpha = 1) against -delta(alpha = 0.001) / alpha: %.1e relative" % (T, rel))
        assert rel <= 1e-12, T


def test_a_forgotten_sample_and_a_repeat_counted_once_show(s5, weights):
    """a sample's own gradient against the rule's bound on the five-sample gradient, tensor by tensor; and on S5r, where sample "c" counts twice"""
    x, t, ref = s5
    names = tb.BATCHES["S5"]["pool"]
    print("S5: sample tensor |its gradient| / bound")
    for s, eff in zip(names, ref["effect"]):
        ratios = {T: eff[T] / ref["bound"][T] for T in ts.TENSORS}
        print("  %-3s" % s, " ".join("%s:%.0f" % kv for kv in ratios.items()))
        for T, q in ratios.items():
            if (s, T) == ("b0", "W1"):
                assert eff[T] == 0.0      # an all-0 tile moves no tap of conv1
            else:
                assert q >= 10.0, (s, T, q)
    order = tb.BATCHES["S5r"]["order"]
    rr = orf.grad_reference("S5r", tb.start_weights("seed", weights), x[order], t[order], 64)
    c = names.index("c")
    assert order.count(c) == 2
    ratios = {T: ref["effect"][c][T] / rr["bound"][T] for T in ts.TENSORS}
    print("S5r, c once instead of twice:", " ".join("%s:%.0f" % kv for kv in ratios.items()))
    assert min(ratios.values()) >= 10.0, ratios
