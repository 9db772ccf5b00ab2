"""The float64 model of a training step (tests/train_ref.py) pinned to the oracle, and the proof that the rule the device is held to
(tests/test_gpu_train_layers.py: max|T_dev - T_f64| <= 4 d_orc(T) + 4 * 2^-24 max|T_f64|) tells a dropped term from rounding.  CPU only.

ho_cnn_train is pinned bit for bit to the reference (test_train.py::test_oracle_training_matches_reference); ho_cnn_train_layers is the same
function returning its intermediates.  d_orc(T) = max|T_oracle32 - T_f64| is the float32 oracle's own distance from float64 per tensor and case."""
import numpy as np
import pytest

import oracle_lib as ol
import train_ref as tr

# what a float32 evaluation in the reference's order may differ from float64 by, relative to the tensor's largest entry: sums of at most 2304
# terms of mixed sign, errors that pass through two 4.7 M-entry products.  Far above what is measured (3e-5 at most, case d), far below a dropped term.
D_ORC_REL = 1e-3


@pytest.mark.parametrize("name", tr.CASES)
def test_oracle_is_finite_and_near_float64(name, weights):
    f64, o32 = tr.reference(name, weights)
    w, x, t, alpha = tr.case(name, weights)
    for k, v in o32.items():
        assert np.isfinite(v).all(), k
    ref = np.array(w, np.float32, copy=True)
    mse = ol.lib().ho_cnn_train(ol.fptr(ref), ol.fptr(x), ol.fptr(t), alpha)
    assert np.array_equal(ref, o32["w"]) and np.float32(mse) == np.float32(o32["mse"])      # the variant with intermediates is the pinned step
    print("case %s: tensor  d_orc  max|T_f64|" % name)
    for T in tr.COMPARED + ("e4", "e0", "e2", "W3", "B3", "W4", "B4"):
        a = o32[T] if T in o32 else tr.split(o32["w"])[T]
        b = f64[T] if T in f64 else tr.split(f64["w"])[T]
        d, m = tr.dist(a, b), float(np.abs(b).max())
        print("  %-4s %.3e %.3e" % (T, d, m))
        assert d <= D_ORC_REL * m, (T, d, m)
    if name == "d":
        a5 = o32["a5"]
        assert (np.abs(a5) == 1.0).any() and (np.abs(a5) < 1.0).any()      # tanh saturates to exactly +-1.0f somewhere, not everywhere
        q = a5.reshape(64, 6, 2, 6, 2).transpose(0, 1, 3, 2, 4).reshape(64, 36, 4)
        tie = ((q == 1.0).sum(-1) >= 2) & (q.min(-1) < 1.0)
        assert tie.any()      # a tie at 1.0f inside a window that is not constant
        assert not (np.abs(o32["a1"]) == 1.0).all() and np.ptp(o32["a5"][np.nonzero(tie)[0][0]]) > 0
    if name in ("b0", "b1"):
        assert np.ptp(o32["a1"], axis=(1, 2)).max() == 0 and np.ptp(f64["a1"], axis=(1, 2)).max() == 0      # every pooling window a tie, in both
        assert np.ptp(o32["a5"], axis=(1, 2)).max() == 0 and np.ptp(f64["a5"], axis=(1, 2)).max() == 0
        for k in ("e4", "e0"):      # and both gave every error to the window's first entry
            assert not f64[k][:, 1::2, :].any() and not f64[k][:, :, 1::2].any() and not o32[k][:, 1::2, :].any() and not o32[k][:, :, 1::2].any()
    if name == "b0":
        assert np.array_equal(f64["W1"], np.float64(tr.split(w)["W1"])) and np.array_equal(o32["W1"], tr.split(w)["W1"])      # a zero input leaves conv1's taps alone


def _windows(a, s):
    """largest |a| per s x s window of [C,H,W] -> [C, (H/s)*(W/s)]"""
    c, h, w = a.shape
    return np.abs(a).reshape(c, h // s, s, w // s, s).max((2, 4)).reshape(c, -1)


def _pick(a):
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(a)), a.shape))


def mutations(f64, w):
    """one instance of each kind of dropped term, placed where the unmutated step says it matters (a kernel bug would drop it everywhere)"""
    oz = int(np.abs(f64["a5"]).max((1, 2)).argmin())      # conv2's least saturated output channel
    return {
        "conv1_tap": (3, 2, 2), "conv1_bias": 3, "conv2_tap": (oz,) + _pick(np.abs(tr.split(np.float64(w))["W2"][oz])),
        "fc1_slab": 5, "fc2_slab": 5, "chunk_dp": 3, "chunk_dp/16": 20,
        "w4_trip": int(np.abs(f64["e8"]).argmax()), "w3_trip": int(np.abs(f64["e6"]).argmax()), "fold_row": int(np.abs(f64["a8"] ** 2 * f64["e8"]).argmax()),
        "part3_group": 7, "pool3": _pick(_windows(f64["e4"], 2)), "pool2": _pick(_windows(f64["e0"], 4)), "pool1": _pick(_windows(f64["e0"], 2)),
    }


# tensor -> the dropped terms that must move it by >= 100 x the rule's bound, in every case but the exemptions below
REQUIRED = {
    "a1": ("conv1_tap", "conv1_bias"), "a3": ("conv1_tap", "conv1_bias"), "a5": ("conv2_tap",), "a6": ("conv2_tap",), "a8": ("fc1_slab",),
    "e9": ("fc2_slab", "chunk_dp", "chunk_dp/16"), "mse": ("fc2_slab",), "e7": ("w4_trip", "fold_row"), "e6": ("w3_trip",), "e3": ("part3_group", "pool3"),
    "W1": ("part3_group", "pool1", "pool2"), "B1": ("part3_group",), "W2": ("fc2_slab", "pool3"), "B2": ("w3_trip",),
}
# (case, tensor, term) that contribute exactly nothing by construction: every other term of that tensor still has to show the ratio
EXEMPT = {
    ("b0", "a1", "conv1_tap"): "the input is zero: a tap adds 0 * w", ("b0", "a3", "conv1_tap"): "the same",
    ("b0", "W1", "part3_group"): "the input is zero: conv1's taps do not move at all (asserted above, and bit for bit on the device)",
    ("b0", "W1", "pool1"): "the same", ("b0", "W1", "pool2"): "the same",
    ("b1", "W1", "pool1"): "the input is constant: the position the error goes to does not matter", ("b1", "W1", "pool2"): "the same",
    ("b0", "W2", "pool3"): "conv2's input is constant per channel: the position does not matter", ("b1", "W2", "pool3"): "the same",
}


@pytest.mark.parametrize("name", tr.CASES)
def test_rule_discriminates(name, weights):
    """Each dropped term moves its tensor by at least 100 x the bound the device is held to."""
    f64, _ = tr.reference(name, weights)
    w, x, t, alpha = tr.case(name, weights)
    muts = mutations(f64, w)
    bad = []
    for m, v in muts.items():
        r = tr.train_step(w, x, t, alpha, mut={m.split("/")[0]: v}, fc_update=False)
        ratios = {T: tr.dist(r[T], f64[T]) / tr.bound(name, T, weights) for T in tr.COMPARED}
        print("case %s %-11s %-16s" % (name, m, v), " ".join("%s:%.0f" % (T, q) for T, q in ratios.items() if q >= 0.5))
        for T, req in REQUIRED.items():
            if m in req:
                if (name, T, m) in EXEMPT:
                    assert ratios[T] < 1e-6, (name, T, m)      # exempt only because it is nothing (float64 rounding of a reordered sum at the most)
                elif ratios[T] < 100.0:
                    bad.append((T, m, ratios[T]))
    assert not bad, bad
    for T in tr.COMPARED:      # no tensor / case pair rests on exemptions alone
        assert (name, T) == ("b0", "W1") or any((name, T, m) not in EXEMPT for m in REQUIRED[T]), T
