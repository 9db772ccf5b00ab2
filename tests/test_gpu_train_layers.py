"""The device training step (csrc/ht_train.hip) layer by layer and on every weight, against the float64 model of tests/train_ref.py.

One native.Context per weight set, one ht_cnn_train step per case of train_ref.CASES; the step's buffers (ht_debug_train_buffers) and the
weights are read back once and shared by the tests below.

Per tensor (a1 a3 a5 a6 a8, e9 e7 e6, sum_g part3[g], the returned mse, W1 B1 W2 B2):
    max|T_dev - T_f64| <= 4 d_orc(T) + 4 * 2^-24 max|T_f64|
d_orc(T) is the float32 oracle's own distance from float64 on the same case, never the device's.  The device sums the same terms in another
order (split-K, wave shuffles, contracted multiply-adds), so its error is of the oracle's order; tests/test_train_ref.py shows that a
dropped term moves each tensor by at least 100 x this bound.

Every weight of W3 B3 W4 B4, element by element: w_old - x[i] e[j] alpha in float64 from the device's own x (a6, a8) and e (e7, e9) of the
same step and the weights loaded before it.  The bound is one float32 spacing of |w_old| wherever the update is small beside the weight.
Where it is not (a weight near zero, or alpha = 0.25) even the correctly rounded float32 result misses that: the final rounding is half a
spacing of the RESULT, and the product x e alpha carries two roundings of its own (one when contracted).  There the bound is what the
number format gives, 0.5 spacing(|w_new|) + 2^-23 |x e alpha|; the bound in force is the larger of the two.  A skipped or doubled update
is off by |x e alpha| itself, thousands of spacings on nearly every entry."""
import numpy as np
import pytest

import oracle_lib as ol
import train_ref as tr

pytestmark = pytest.mark.gpu


def fc_check(name, w_old, w_new, x, e, alpha):
    """every entry of a fully connected layer's matrix (or bias, x = [1]) against float64 from the device's own factors"""
    a = float(np.float32(alpha))
    u = np.multiply.outer(np.float64(x), np.float64(e)).reshape(w_old.shape) * a
    exp = np.float64(w_old) - u
    diff = np.abs(np.float64(w_new) - exp)
    literal = np.float64(np.spacing(np.abs(w_old)))
    fmt = 0.5 * np.float64(np.spacing(np.abs(exp).astype(np.float32))) + 2.0 ** -23 * np.abs(u)
    tol = np.maximum(literal, fmt)
    ratio = diff / tol
    i = int(ratio.argmax())
    return dict(name=name, n=w_old.size, worst=float(ratio.flat[i]), index=i, diff=float(diff.flat[i]), tol=float(tol.flat[i]), w_old=float(w_old.flat[i]), w_new=float(w_new.flat[i]),
                expected=float(exp.flat[i]), over=int((diff > tol).sum()), over_one_spacing=int((diff > literal).sum()), format_bound_in_force=int((fmt > literal).sum()),
                moved=int((w_new != w_old).sum()))


@pytest.fixture(scope="module")
def steps(weights):
    from hand_tracking_samples_amd import native
    out = {}
    for group in (("a", "b0", "b1", "c", "e"), ("d",)):      # the seeded weights; W1 and W2 scaled
        ctx = native.Context(ol.MODEL, 1)
        try:
            for name in group:
                w, x, t, alpha = tr.case(name, weights)
                ctx.load_weights(w)
                mse = ctx.cnn_train(x[None], t[None], alpha)
                buf = ctx.cnn_train_buffers()
                wn = ctx.cnn_get_weights()
                O = tr.OFF
                r = dict(buf, mse=float(mse[0]), e3=buf["part3"].astype(np.float64).sum(0).reshape(16, 15, 15))
                r.update({k: v.copy() for k, v in tr.split(wn).items() if k in ("W1", "B1", "W2", "B2")})
                r["fc"] = [fc_check("W3", w[O["W3"]:O["B3"]].reshape(2304, 2048), wn[O["W3"]:O["B3"]].reshape(2304, 2048), buf["a6"], buf["e7"], alpha),
                           fc_check("B3", w[O["B3"]:O["W4"]], wn[O["B3"]:O["W4"]], np.ones(1), buf["e7"], alpha),
                           fc_check("W4", w[O["W4"]:O["B4"]].reshape(2048, 2304), wn[O["W4"]:O["B4"]].reshape(2048, 2304), buf["a8"], buf["e9"], alpha),
                           fc_check("B4", w[O["B4"]:], wn[O["B4"]:], np.ones(1), buf["e9"], alpha)]
                if name == "e":
                    ctx.cnn_eval(x[None])      # the inference kernels after the step
                    r["w_new"] = wn; r["eval_layers"] = [v[0].copy() for v in ctx.cnn_layers(1)[1:]]
                out[name] = r
        finally:
            ctx.close()
    return out


@pytest.mark.parametrize("name", tr.CASES)
def test_every_tensor_of_a_step_matches_float64(name, steps, weights):
    f64, _ = tr.reference(name, weights)
    dev = steps[name]
    bad = []
    print("case %s: tensor d_dev bound d_dev/bound" % name)
    for T in tr.COMPARED:
        d, b = tr.dist(dev[T], f64[T]), tr.bound(name, T, weights)
        print("  %s %-4s %.3e %.3e %.3f" % (name, T, d, b, d / b))
        if not d <= b:
            bad.append((T, d, b))
    assert not bad, bad
    if name == "b0":
        assert np.array_equal(dev["W1"], tr.split(tr.case(name, weights)[0])["W1"])      # a zero input moves no tap of conv1


@pytest.mark.parametrize("name", tr.CASES)
def test_every_fully_connected_weight_is_stepped_once(name, steps):
    bad = []
    for c in steps[name]["fc"]:
        print("case %s %s: worst |w_dev - w_f64| / bound %.3f at entry %d (%.9g, float64 %.17g, was %.9g); beyond one spacing of |w_old|: %d of %d, format bound in force on %d, moved %d"
              % (name, c["name"], c["worst"], c["index"], c["w_new"], c["expected"], c["w_old"], c["over_one_spacing"], c["n"], c["format_bound_in_force"], c["moved"]))
        if c["over"]:
            bad.append(c)
    assert not bad, bad


def eval_layers(w, x):
    """ho_cnn_eval on weights w: (pooled conv2 output a6, a8, logits, soft-max output)"""
    import ctypes as C
    layers = [np.zeros(n, np.float32) for n in tr.SIZES]
    y = np.zeros(2304, np.float32)
    ol.lib().ho_cnn_eval(ol.fptr(np.ascontiguousarray(w, np.float32)), ol.fptr(x), ol.fptr(y), (C.POINTER(C.c_float) * 11)(*[ol.fptr(a) for a in layers]))
    return layers[6], layers[8], layers[9], y


def test_inference_copies_follow_the_step(steps, weights):
    """cnn_eval after the step of case e reads conv2 and the last layer from copies packed for MFMA: they must hold the stepped weights.
    At alpha = 0.25 the stepped net's logits pass 88 on this input (the oracle's reach 185), so expf overflows and the reference's own
    soft-max output is NaN (inf / inf): there is nothing finite to hold the heat-maps to.  The layers before the soft-max are finite, so the
    comparison is made there: conv2's pooled output and FC1's output under the bounds of tests/test_gpu_cnn.py (5e-6, 1e-5), the logits
    under the rule of this file, 4 d_orc + 4 * 2^-24 max|logits|, d_orc = the oracle's distance from the float64 forward pass on the same
    weights.  Asserted first, on the CPU: the pre-step weights move these layers by more than 100 x those bounds, and each packed copy
    alone, left stale, by more than 10 x (the last layer's matrix alone: 75 x, its update is small beside FC1's on this input)."""
    w, x, t, alpha = tr.case("e", weights)
    dev = steps["e"]
    O = tr.OFF
    a6, a8, lg, y = eval_layers(dev["w_new"], x)
    assert np.isfinite(lg).all() and lg.max() > 89.0 and not np.isfinite(y).all()      # why the output itself cannot be compared
    f64 = tr.train_step(dev["w_new"], x, t, 0.0, fc_update=False)["logits"]
    tol = 4.0 * tr.dist(lg, f64) + 4.0 * 2.0 ** -24 * float(np.abs(f64).max())
    stale2 = dev["w_new"].copy(); stale2[O["W2"]:O["B2"]] = w[O["W2"]:O["B2"]]
    stale4 = dev["w_new"].copy(); stale4[O["W4"]:O["B4"]] = w[O["W4"]:O["B4"]]
    old = eval_layers(w, x)
    d6_all, d9_all = float(np.abs(old[0] - a6).max()) / 5e-6, float(np.abs(old[2] - lg).max()) / tol
    d6, d9 = float(np.abs(eval_layers(stale2, x)[0] - a6).max()) / 5e-6, float(np.abs(eval_layers(stale4, x)[2] - lg).max()) / tol
    print("pre-step weights move conv2+pool by %.0f x its bound and the logits by %.0f x theirs (%.3e); a stale conv2 copy alone %.0f x, a stale last layer alone %.0f x" % (d6_all, d9_all, tol, d6, d9))
    assert d6_all > 100.0 and d9_all > 100.0 and d6 > 10.0 and d9 > 10.0
    g6, g8, g9 = dev["eval_layers"]
    e6, e8, e9 = float(np.abs(g6 - a6).max()), float(np.abs(g8 - a8).max()), float(np.abs(g9 - lg).max())
    print("after the step, device vs oracle on the weights read back: conv2+pool %.3e, fc1 %.3e, logits %.3e (bound %.3e)" % (e6, e8, e9, tol))
    assert e6 <= 5e-6 and e8 <= 1e-5 and e9 <= tol
