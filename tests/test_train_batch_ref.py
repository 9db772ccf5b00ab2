"""What the rule the mini-batch step is held to (tests/test_gpu_train_batch.py) tells from rounding.  CPU only.

Per weight tensor T:  max|T_dev' - T_64'| <= bound(T) = 4 d_orc(T) + 4 * 2^-24 max|T_64'|, references from tests/train_batch_ref.py.  Shown here, in
float64: a step that forgets a sample, counts a repeated sample once, takes the second step's gradients at the first step's weights, or leaves one
sample out of one layer's sum lands at least 10 x the bound away (1000 x at alpha = 0.25), tensor by tensor."""
import numpy as np
import pytest

import train_batch_ref as tb
import train_ref as tr


@pytest.fixture(scope="module")
def refs(weights):
    return tb.references(("S1", "S3", "S5", "S3hi", "S5r", "S5x2", "S5x2stale"), weights)


def test_a_batch_of_one_is_the_single_sample_reference(refs, weights):
    f64, _ = tr.reference("c", weights)
    step = refs["S1"][0]
    assert np.abs(step["w64"] - f64["w"]).max() <= 1e-15
    for T in tb.PER_SAMPLE:
        assert step["samples"][0]["bound"][T] == tr.bound("c", T, weights), T
        assert np.array_equal(step["samples"][0]["tensors"][T], f64[T]), T
    for T in tb.TENSORS:      # and the batch rule on one sample is the layer tests' rule on that case
        if T in tr.COMPARED:
            assert abs(step["bound"][T] - tr.bound("c", T, weights)) <= 1e-12 * step["bound"][T], T


@pytest.mark.parametrize("name,need", [("S3", 10.0), ("S5", 10.0), ("S3hi", 1000.0)])
def test_a_dropped_sample_moves_every_tensor_it_can_move(name, need, refs):
    step = refs[name][0]
    bad = []
    print("batch %s: sample tensor |its term| / bound" % name)
    for s, rec in zip(step["names"], step["samples"]):
        ratios = {T: rec["effect"][T] / step["bound"][T] for T in tb.TENSORS}
        print("  %-3s" % s, " ".join("%s:%.0f" % kv for kv in ratios.items()))
        for T, q in ratios.items():
            if (s, T) == ("b0", "W1"):
                assert rec["effect"][T] == 0.0      # an all-0 tile moves no tap of conv1: the one pair there is nothing to see on
            elif q < need:
                bad.append((s, T, q))
    assert not bad, bad


def test_a_repeat_counted_once_shows(refs):
    """S5r trains on sample 3 ("c") twice: counting it once is off by its whole term"""
    step = refs["S5r"][0]
    assert step["names"].count("c") == 2
    rec = step["samples"][step["names"].index("c")]
    ratios = {T: rec["effect"][T] / step["bound"][T] for T in tb.TENSORS}
    print("S5r, c once instead of twice:", " ".join("%s:%.0f" % kv for kv in ratios.items()))
    assert min(ratios.values()) >= 10.0, ratios


def test_a_second_step_from_the_first_steps_weights_shows(refs, weights):
    """S5x2's second step with its gradients taken at the call's starting weights (all ten samples at w) against taken at the first step's result"""
    one, two, stale = refs["S5x2"][0], refs["S5x2"][1], refs["S5x2stale"][0]
    w = np.float64(tb.start_weights("seed", weights))
    wrong = one["w64"] + (stale["w64"] - w)
    P, Q = tr.split(two["w64"]), tr.split(wrong)
    ratios = {T: tr.dist(P[T], Q[T]) / two["bound"][T] for T in tb.TENSORS}
    print("S5x2, second step at the starting weights:", " ".join("%s:%.0f" % kv for kv in ratios.items()))
    assert min(ratios.values()) >= 10.0, ratios


def test_a_sample_missing_from_one_layer_shows_in_that_layer(refs, weights):
    """sample "c" left out of one tensor's sum only: that tensor is off by its term, the others not at all"""
    step = refs["S5"][0]
    rec = step["samples"][step["names"].index("c")]
    x, t = tb.sample("c", weights)
    w = np.float64(tb.start_weights("seed", weights))
    term = tr.split(tr.train_step(w, x, t, tb.BATCHES["S5"]["alpha"])["w"] - w)
    for T in tb.TENSORS:
        wrong = step["w64"].copy()
        tr.split(wrong)[T][...] -= term[T]
        P, Q = tr.split(step["w64"]), tr.split(wrong)
        d = {U: tr.dist(P[U], Q[U]) for U in tb.TENSORS}
        print("S5 without c in %s: %.0f x its bound" % (T, d[T] / step["bound"][T]))
        assert d[T] >= 10.0 * step["bound"][T] and abs(d[T] - rec["effect"][T]) <= 1e-12 * rec["effect"][T], T
        assert all(d[U] == 0.0 for U in tb.TENSORS if U != T), T
