"""The references the sized mini-batch step is held to (tests/train_ref_sized.py; tests/test_gpu_train_sized.py), checked against what is pinned.  CPU only.

No golden of the backward pass exists at side 128 (the reference harness has no such mode), so the yardstick is pinned by construction:
(a) at side 64 the float64 mode is tests/train_ref.py's step, tensor by tensor, to 1e-12 relative: the same arithmetic in the same precision;
(b) at side 64 the float32 mode is no looser a yardstick than the pinned oracle: d32(T) <= 2 d_orc(T) for every tensor of every case;
(c) at side 128 the forward pass is the reference's own layers (tests/golden/cnn128.htfx): the float32 mode bit for bit, the float64 mode within the rounding
    a float32 sum of that length typically gathers: layer l against 2 sqrt(K_l) * 2^-24 * max(1, max|layer|), K_l = the terms summed per output up to and
    including that layer (25, + 256, + 12544, + 2048): K roundings of half an ulp with random signs add up like sqrt(K), and 2 is the margin (the worst case, K
    itself, is 60 x looser at the logits and would pass a reference that is wrong in the fourth digit);
(d) at side 128 a step that forgets a sample, counts a repeat once, takes the second step at the first step's weights or leaves a sample out of one tensor's
    sum lands outside the rule  max|T' - T_64'| <= 4 d32(T) + 4 * 2^-24 max|T_64'|  (the factors are printed)."""
import os

import numpy as np
import pytest

import htfx
import train_ref as tr
import train_ref_sized as ts
from hand_tracking_samples_amd import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
CMP64 = ("a3", "a6", "a8", "e9", "e7", "e6", "e3", "mse")


@pytest.fixture(scope="module")
def w128():
    return W.make_cnnb128()


@pytest.fixture(scope="module")
def refs(w128):
    return ts.references(("T5", "T5r", "T5x2", "T5x2stale"), w128)


def test_the_layouts_are_the_cnnb_orders():
    off, shape, count = ts.layout(64)
    assert off == tr.OFF and shape == tr.SHAPE and count == tr.COUNT == W.cnnb_count(64)
    assert ts.layout(128)[2] == W.cnnb_count(128) == 30429920 and ts.dims(128)["fc"] == W.features(128)


@pytest.mark.parametrize("name", tr.CASES)
def test_side_64_float64_is_train_ref_and_float32_is_no_looser_than_the_oracle(name, weights):
    w, x, t, alpha = tr.case(name, weights)
    f64, o32 = tr.reference(name, weights)
    f64 = dict(f64, **tr.split(f64["w"]))
    g64 = ts.single(np.float64(w), x, t, alpha, 64, "f64")
    g32 = ts.single(w, x, t, alpha, 64, "f32")
    bad = []
    for T in CMP64 + ("logits", "y", "w") + ts.TENSORS:
        a, b = np.asarray(g64[T], np.float64).reshape(-1), np.asarray(f64[T], np.float64).reshape(-1)
        rel = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
        if not rel <= 1e-12:
            bad.append(("f64", T, rel))
    print("case %s: tensor d32 d_orc d32/d_orc" % name)
    for T in CMP64 + ts.TENSORS:
        d32, dorc = ts.dist(g32[T], np.asarray(f64[T]).reshape(np.shape(g32[T]))), ts.dist(o32[T], f64[T])
        print("  %s %-4s %.3e %.3e %.3f" % (name, T, d32, dorc, d32 / dorc if dorc else float(d32 != 0)))
        if not d32 <= 2.0 * dorc:
            bad.append(("f32", T, d32, dorc))
    assert not bad, bad


def test_side_128_forward_is_the_reference_and_td_saturates(w128):
    G = htfx.load(os.path.join(HERE, "golden", "cnn128.htfx"))
    assert [int(i) for i in G["frames"]] == list(ts.FRAMES)
    x, t = ts.sample("f0")
    assert np.array_equal(x.reshape(128, 128), G["f0/cnn_input"])
    r32 = ts.step(w128, x[None], t[None], 0.001, 128, "f32", want_delta=False)
    r64 = ts.step(np.float64(w128), x[None], t[None], 0.001, 128, "f64", want_delta=False)
    K = 0
    for key, name, k in (("a3", "f0/layer3", 25), ("a6", "f0/layer6", 256), ("a8", "f0/layer8", 12544), ("logits", "f0/layer9", 2048), ("y", "f0/cnn_output", 0)):
        K += k
        g = G[name].reshape(-1)
        d32, d64 = ts.dist(r32[key][0].reshape(-1), g), ts.dist(r64[key][0].reshape(-1), g)
        allowed = 2.0 * K ** 0.5 * 2.0 ** -24 * max(1.0, float(np.abs(g).max()))
        print("%s: float32 mode %.3e, float64 mode %.3e (allowed %.3e)" % (name, d32, d64, allowed))
        assert np.array_equal(r32[key][0].reshape(-1), g), name
        assert d64 <= allowed, name
    # batch Td: on the scaled weights the float32 mode reaches tanh = +-1.0f exactly and stays finite
    wd = ts.start_weights("sat", w128)
    X, T = ts.pool_arrays("Td")
    rd = ts.step(wd, X, T, 0.001, 128, "f32", want_delta=False)
    sat = int((np.abs(rd["a8"]) == 1.0).sum())
    print("Td: %d of %d a8 at exactly +-1.0f" % (sat, rd["a8"].size))
    assert sat >= 1 and all(np.isfinite(rd[k]).all() for k in ts.PER_SAMPLE)


def _factors(effect, bound):
    return {T: effect[T] / bound[T] for T in ts.TENSORS}


def test_a_forgotten_sample_shows(refs):
    step = refs["T5"][0]
    print("T5: sample, |its term| / bound per tensor")
    for s, rec in zip(step["names"], step["samples"]):
        q = _factors(rec["effect"], step["bound"])
        print("  %-3s" % s, " ".join("%s:%.1f" % kv for kv in q.items()))
        assert max(q.values()) > 1.0, (s, q)


def test_a_repeat_counted_once_shows(refs):
    step = refs["T5r"][0]
    assert step["names"].count("x0") == 2
    q = _factors(step["samples"][step["names"].index("x0")]["effect"], step["bound"])
    print("T5r, x0 once instead of twice:", " ".join("%s:%.1f" % kv for kv in q.items()))
    assert max(q.values()) > 1.0, q


def test_a_second_step_from_the_first_steps_weights_shows(refs, w128):
    one, two, stale = refs["T5x2"][0], refs["T5x2"][1], refs["T5x2stale"][0]
    wrong = one["w64"] + (stale["w64"] - np.float64(ts.start_weights("seed", w128)))
    P, Q = ts.split(two["w64"], 128), ts.split(wrong, 128)
    q = {T: ts.dist(P[T], Q[T]) / two["bound"][T] for T in ts.TENSORS}
    print("T5x2, second step at the starting weights:", " ".join("%s:%.1f" % kv for kv in q.items()))
    assert max(q.values()) > 1.0, q


def test_a_sample_missing_from_one_tensor_shows_in_that_tensor(refs):
    """x0 left out of one tensor's sum only: that tensor is off by x0's term there, which is its effect"""
    step = refs["T5"][0]
    q = _factors(step["samples"][step["names"].index("x0")]["effect"], step["bound"])
    print("T5 without x0 in one tensor:", " ".join("%s:%.1f" % kv for kv in q.items()))
    assert min(q.values()) > 1.0, q
