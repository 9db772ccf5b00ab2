"""What the rule the inference nets are held to (tests/test_gpu_cnn_forward.py) can tell from rounding, shown on the CPU for both input sides, in the manner of
tests/test_train_ref.py.  No GPU.

For every tensor T of a3, a6, a8, logits, y and every case ("How the inference nets are checked"):
    max|T - T_f64| <= 4 d32(T) + 4 * 2^-24 max|T_f64|,   d32(T) = max|T_f32 - T_f64|
with tests/train_ref_sized.py's forward() in its two modes.  Each mutation below is one mistake a banded convolution or a tiled product can make, injected into the float64
forward on whole rows (a single pixel can lose its pooling window and vanish): on at least one case the tensor it feeds must leave the bound.  On frame 0 alone, a real depth
tile that is mostly constant background, several of them do not move the output by the 2e-5 the output-only tests allow: that is why the dense cases exist.

Where the bands lie: k_conv1<128,31,8> takes 8 pooled rows = 32 output rows a block (4 bands, the last holds 7 pooled rows: 24..30), k_conv2<31,28,4> 4 output rows (7 bands);
the 64x64 net's kernels take the whole frame (one band).  k_fc's slabs are 32 deep (K = 2304 or 12544), k_fc144_pk's blocks 16 deep, act3 is stored in k_fc<PACK16>'s order."""
import numpy as np
import pytest

import train_ref_sized as ts
from hand_tracking_samples_amd import weights as W

OUTPUT_TOL = 2e-5      # what tests/test_gpu_cnn.py, tests/test_cnn128.py and tests/test_config5_e2e.py allow on the output
CH, OZ, TAP = 3, 5, (3, 1, 2)      # conv1's channel; conv2's output channel and the tap (input channel, ky, kx) it loses


def mutations(side):
    """(name, the tensor it feeds, forward()'s mut)"""
    D = ts.dims(side)
    b1, b2 = (32, 4) if side == 128 else (D["c1"], D["c2"])      # output rows a block of conv1 / conv2 takes
    m = [("conv1 row %d (band %d) without ky=0" % (r, r // b1), "a3", {"conv1_row": (CH, r)}) for r in range(0, D["c1"], b1)]
    if side == 128:
        m.append(("a3 row 30 (last of the short band) from row 29", "a3", {"pool_row": (CH, 30, 29)}))
    m += [("conv2 row %d (band %d) without one tap" % (r, r // b2), "a6", {"conv2_row": (OZ, r) + TAP}) for r in range(0, D["c2"], b2)]
    m += [("fc1 without its first slab", "a8", {"fc1_slab": 0}), ("fc1 without its last slab", "a8", {"fc1_slab": D["fc"] - 32}),
          ("fc2 without one 16-k block", "logits", {"fc2_block": 16 * 5}), ("act3 columns 116 and 117 swapped", "logits", {"act3_swap": 16 * 7 + 4}),
          ("soft-max chunk 3 (256) with chunk 4's sum", "y", {"softmax_sum": (3, 4)}), ("soft-max chunk 20 (16) with chunk 21's sum", "y", {"softmax_sum": (20, 21)})]
    return m


@pytest.fixture(scope="module", params=(64, 128))
def net(request):
    side = request.param
    w = W.make_cnnb() if side == 64 else W.make_cnnb128()
    R = ts.forward_references(side, w)
    w64 = {k: np.float64(ts.forward_weights(k, w, side)) for k in ("seed", "sat")}
    rows = {k: [i for i, q in enumerate(R["wkey"]) if q == k] for k in ("seed", "sat")}
    moved = {}      # mutation -> tensor -> how far every case moves, [8]
    for name, _, mut in mutations(side):
        moved[name] = {T: np.zeros(len(R["names"])) for T in ts.FWD_TENSORS}
        for k in ("seed", "sat"):
            r = ts.forward(w64[k], R["X"][rows[k]], side, "f64", mut)
            for T in ts.FWD_TENSORS:
                moved[name][T][rows[k]] = np.abs(np.asarray(r[T]).reshape(len(rows[k]), -1) - R["f64"][T][rows[k]]).max(1)
    return side, R, moved


def test_the_references_are_finite_and_the_saturated_cases_saturate(net):
    side, R, _ = net
    print("side %d: the bound per tensor and case (4 d32 + 4 * 2^-24 max|T_f64|)" % side)
    print("  %-7s" % "tensor", " ".join("%-9s" % s for s in R["names"]))
    for T in ts.FWD_TENSORS:
        assert np.isfinite(R["f64"][T]).all() and np.isfinite(R["f32"][T]).all(), T
        print("  %-7s" % T, " ".join("%.3e" % v for v in R["bound"][T]))
        # a float32 sum of at most 12544 terms in the reference's order stays within 1e-3 of the tensor's largest entry (tests/test_train_ref.py's D_ORC_REL)
        assert (R["d32"][T] <= 1e-3 * np.abs(R["f64"][T]).max(1)).all(), T
    sat = [i for i, q in enumerate(R["wkey"]) if q == "sat"]
    assert (np.abs(R["f32"]["a6"][sat]) == 1.0).any() and (np.abs(R["f32"]["a6"][sat]) < 1.0).any()      # tanh reaches exactly +-1.0f somewhere, not everywhere
    for i, s in enumerate(R["names"]):
        if s in ("z0", "z1"):      # a constant tile: every position of a map equal, in both modes
            assert np.ptp(R["f64"]["a3"][i].reshape(16, -1), axis=1).max() == 0 and np.ptp(R["f32"]["a3"][i].reshape(16, -1), axis=1).max() == 0


def test_every_mutation_leaves_the_bound_of_the_tensor_it_feeds(net):
    side, R, moved = net
    bad = []
    print("side %d: mutation / bound of the tensor it feeds, per case" % side)
    for name, T, _ in mutations(side):
        q = moved[name][T] / R["bound"][T]
        print("  %-48s %-6s" % (name, T), " ".join("%s:%.3g" % (s, v) for s, v in zip(R["names"], q)), " largest %.3g" % q.max())
        if not q.max() > 1.0:
            bad.append((name, T, float(q.max())))
    assert not bad, bad


def test_frame_0_alone_lets_several_mutations_through_the_output_check(net):
    """what the output-only comparison on real frames (2e-5 on the soft-max probabilities) cannot see, and the rule on the dense cases can"""
    side, R, moved = net
    f0 = R["names"].index("f0")
    hidden = []
    print("side %d, frame 0: how far each mutation moves the output y (the output-only tests allow %.0e)" % (side, OUTPUT_TOL))
    for name, T, _ in mutations(side):
        dy = moved[name]["y"][f0]
        q = (moved[name][T] / R["bound"][T]).max()
        print("  %-48s |dy| %.2e   largest ratio under the rule %.3g" % (name, dy, q))
        if dy <= OUTPUT_TOL:
            hidden.append(name)
            assert q > 1.0, name      # ... and the rule sees each of them on some case
    if side == 128:
        assert len(hidden) >= 3, hidden
