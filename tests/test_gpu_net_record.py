"""The two pose nets of a context as two independent records (csrc/ht_host.hpp: ht_net, ht_net_of): what every sized entry point answers to a side it does not serve
and to a net without weights, code and text, and that loading, evaluating and training one net leaves the other's weights, buffers and results as they were.
Needs an MI355X: pytest -m gpu.

Two tiles per net and steps of two samples: the smallest batch with a second slot, whose stride every per-net buffer has to get right (the tile-edge and batch-edge
shapes are tests/test_gpu_cnn_forward.py's).  Contexts of max_batch 2."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as ol
from hand_tracking_samples_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OK, ARG, STATE = 0, 1, 4      # include/ht_mi355x.h
CNN_ATOL = 2e-5               # tests/test_gpu_cnn.py: the fp32 MFMA sums against the reference's, on soft-max outputs <= 1
N64, N128 = 9458400, 30429920

SIDE = "CNN input side must be 64 or 128"
NO64 = "CNN weights not loaded (ht_cnn_load_weights)"
NO128 = "weights of the 128x128 net not loaded (ht_cnn_load_weights_sized)"
TRAIN64 = ": the context holds no weights of the 64x64-input net (ht_cnn_load_weights); the 128x128-input net is trained by ht_cnn_train_batch_sized"
TRAIN128 = ": the context holds no weights of the 128x128-input net (ht_cnn_load_weights_sized)"
ALIGN = ": d_tiles and d_cnn_in must be 16-byte aligned (the input transform reads eight pixels per 128-bit load and writes float4)"
# Every sized entry point and ht_update_direct_sync, three refused calls each: side 96; side 128 on a context that holds the 64x64-input net's weights only; side 64 on a
# second context that holds no weights.  (entry point, context, arguments behind the context, status, message); a name stands for the buffer of that name in _buffers.
# Where a net without weights is no reason to refuse (the loader; the input transform, which needs no weights; the layer getter at side 64, whose buffers come with the
# context), the call is refused for a reason that shows which net, or which form of the entry point, answered: the value count, the alignment rule, the slot range.
REFUSALS = (
    ("ht_cnn_load_weights_sized", "A", (96, "w", N64), ARG, SIDE),
    ("ht_cnn_load_weights_sized", "A", (128, "w", N64), ARG, "weights: expected HT_CNNB128_COUNT fp32 values in .cnnb order"),
    ("ht_cnn_load_weights_sized", "B", (64, "w", N128), ARG, "weights: expected HT_CNNB_COUNT fp32 values in .cnnb order"),
    ("ht_cnn_eval_sized", "A", (96, "x", "y", 1), ARG, SIDE),
    ("ht_cnn_eval_sized", "A", (128, "x", "y", 1), STATE, NO128),
    ("ht_cnn_eval_sized", "B", (64, "x", "y", 1), STATE, NO64),
    ("ht_cnn_eval_sized_dev", "A", (96, "d_x", "d_y", 1, None), ARG, SIDE),
    ("ht_cnn_eval_sized_dev", "A", (128, "d_x", "d_y", 1, None), STATE, NO128),
    ("ht_cnn_eval_sized_dev", "B", (64, "d_x", "d_y", 1, None), STATE, NO64),
    ("ht_cnn_input_sized_dev", "A", (96, "d_tiles", "d_cams", 1, "d_x", None), ARG, SIDE),
    ("ht_cnn_input_sized_dev", "A", (128, "d_tiles+2", "d_cams", 1, "d_x", None), ARG, "ht_cnn_input_sized_dev" + ALIGN),
    ("ht_cnn_input_sized_dev", "B", (64, "d_tiles+2", "d_cams", 1, "d_x", None), ARG, "ht_cnn_input_dev" + ALIGN),
    ("ht_cnn_train_batch_sized", "A", (96, "x", "t", 2, 2, 0.001, "mse"), ARG, SIDE),
    ("ht_cnn_train_batch_sized", "A", (128, "x", "t", 2, 2, 0.001, "mse"), ARG, "ht_cnn_train_batch_sized" + TRAIN128),
    ("ht_cnn_train_batch_sized", "B", (64, "x", "t", 2, 2, 0.001, "mse"), ARG, "ht_cnn_train_batch" + TRAIN64),
    ("ht_cnn_train_batch_sized_dev", "A", (96, "d_x", "d_t", 2, None, 1, 2, 0.001, None, None), ARG, SIDE),
    ("ht_cnn_train_batch_sized_dev", "A", (128, "d_x", "d_t", 2, None, 1, 2, 0.001, None, None), ARG, "ht_cnn_train_batch_sized_dev" + TRAIN128),
    ("ht_cnn_train_batch_sized_dev", "B", (64, "d_x", "d_t", 2, None, 1, 2, 0.001, None, None), ARG, "ht_cnn_train_batch_dev" + TRAIN64),
    ("ht_debug_train_batch_buffers_sized", "A", (96, 2) + ("big",) * 7, ARG, SIDE),
    ("ht_debug_train_batch_buffers_sized", "A", (128, 2) + ("big",) * 7, STATE, "ht_debug_train_batch_buffers_sized: no mini-batch step has run"),
    ("ht_debug_train_batch_buffers_sized", "B", (64, 2) + ("big",) * 7, STATE, "ht_debug_train_batch_buffers: no mini-batch step has run"),
    ("ht_cnn_get_weights_sized", "A", (96, "w", N64), ARG, SIDE),
    ("ht_cnn_get_weights_sized", "A", (128, "w", N128), STATE, "no weights to read"),
    ("ht_cnn_get_weights_sized", "B", (64, "w", N64), STATE, "no weights to read"),
    ("ht_get_cnn_layers_sized", "A", (96, 0, 1, "big", "big", "big", "big"), ARG, SIDE),
    ("ht_get_cnn_layers_sized", "A", (128, 0, 1, "big", "big", "big", "big"), STATE, NO128),
    ("ht_get_cnn_layers_sized", "B", (64, 0, 3, "big", "big", "big", "big"), ARG, "slot range exceeds the capacity given to ht_create"),
    ("ht_update_direct_sync", "A", ("depth", "cams", 96, 1, "poses", "y"), ARG, "ht_update_direct: " + SIDE),
    ("ht_update_direct_sync", "A", ("depth", "cams", 128, 1, "poses", "y"), STATE, NO128),
    ("ht_update_direct_sync", "B", ("depth", "cams", 64, 1, "poses", "y"), STATE, NO64),
)


def _buffers():
    """arguments large enough for either side, so that no refusal is the only thing between a call and an overrun"""
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    host = dict(w=np.zeros(N128, np.float32), x=np.zeros((2, 16384), np.float32), y=np.zeros((2, 2304), np.float32), t=np.zeros((2, 2304), np.float32),
                mse=np.zeros(2, np.float32), big=np.zeros(3 * 16 * 31 * 31, np.float32), cams=np.zeros((2, 12), np.float32), poses=np.zeros((2, 32, 7), np.float32))
    depth = np.zeros((2, 16384), np.uint16)
    dev = dict(d_x=torch.zeros((2, 16384), device=DEV), d_y=torch.zeros((2, 2304), device=DEV), d_t=torch.zeros((2, 2304), device=DEV),
               d_tiles=torch.zeros((2, 16384), dtype=torch.int16, device=DEV), d_cams=torch.zeros((2, 12), device=DEV))
    args = {k: fp(v) for k, v in host.items()}
    args["depth"] = depth.ctypes.data_as(C.POINTER(C.c_uint16))
    args.update({k: v.data_ptr() for k, v in dev.items()})
    args["d_tiles+2"] = dev["d_tiles"].data_ptr() + 2
    return args, (host, depth, dev)      # the second: what keeps the memory alive


def _tiles(golden):
    return np.stack([golden["f%d/cnn_input" % f] for f in (0, 1)]), np.stack([golden["f%d/cnn_output" % f] for f in (0, 1)])


def test_every_sized_entry_point_refuses_with_its_code_and_text(golden, weights):
    from hand_tracking_samples_amd import native
    x, ref = _tiles(golden)
    args, keep = _buffers()
    A = native.Context(ol.MODEL, 2); B = native.Context(ol.MODEL, 2)      # A: the 64x64-input net's weights only; B: none
    try:
        A.load_weights(weights)
        before = A.cnn_eval(x)
        seen = set()
        for entry, which, a, code, text in REFUSALS:
            ctx = A if which == "A" else B
            got = getattr(ctx.L, entry)(ctx.h, *[args[v] if isinstance(v, str) else v for v in a])
            assert (got, ctx.L.ht_last_error(ctx.h).decode()) == (code, text), (entry, a)
            seen.add(entry)
        assert len(seen) == 10 and len(REFUSALS) == 30
        # the refusals left both contexts as they were: A evaluates as before, and as the reference does; B takes its weights now and gives A's bits
        after = A.cnn_eval(x)
        assert np.array_equal(after, before) and np.abs(after - ref).max() <= CNN_ATOL and np.allclose(after.sum(axis=1), 24.0, atol=1e-3)
        assert np.array_equal(A.cnn_get_weights(), weights)
        B.load_weights(weights)
        assert np.array_equal(B.cnn_eval(x), before)
    finally:
        A.close(); B.close()
    del keep


def _eval(ctx, side, x):
    return ctx.cnn_eval(x) if side == 64 else ctx.cnn128_eval(x)


def _load(ctx, side, w):
    (ctx.load_weights if side == 64 else ctx.load_weights128)(w)


def test_loading_evaluating_and_training_one_net_leaves_the_other_alone(golden, weights):
    from hand_tracking_samples_amd import native
    rng = np.random.default_rng(20261)
    X = {64: _tiles(golden)[0], 128: rng.random((2, 16384), dtype=np.float32)}
    T = {s: rng.random((2, 2304), dtype=np.float32) * np.float32(1 / 16) for s in (64, 128)}
    make = {64: W.make_cnnb, 128: W.make_cnnb128}
    ctx = native.Context(None, 2)
    try:
        _load(ctx, 64, weights); _load(ctx, 128, make[128]())
        for own, other in ((64, 128), (128, 64)):
            w_own = ctx.cnn_get_weights(side=own)
            y = _eval(ctx, own, X[own])
            a1, a2 = ctx.cnn_layers(2, side=own)[:2]
            assert np.isfinite(y).all() and np.allclose(y.sum(axis=1), 24.0, atol=1e-3) and not np.array_equal(y[0], y[1])
            assert a1.any() and a2.any() and not np.array_equal(a1[0], a1[1]) and not np.array_equal(a2[0], a2[1])
            y_other = _eval(ctx, other, X[other])
            _load(ctx, other, make[other](seed=0x5EED0002))
            assert not np.array_equal(_eval(ctx, other, X[other]), y_other)      # the other net did take the new weights
            w_other = ctx.cnn_get_weights(side=other)
            mse = ctx.cnn_train_batch(X[other], T[other], 2, 0.001, side=other)
            assert np.isfinite(mse).all() and not np.array_equal(ctx.cnn_get_weights(side=other), w_other)      # and the step
            b1, b2 = ctx.cnn_layers(2, side=own)[:2]      # the other net's evaluations and its step wrote buffers of its own
            assert np.array_equal(b1, a1) and np.array_equal(b2, a2)
            assert np.array_equal(_eval(ctx, own, X[own]), y)
            assert np.array_equal(ctx.cnn_get_weights(side=own), w_own)
            b1, b2 = ctx.cnn_layers(2, side=own)[:2]
            assert np.array_equal(b1, a1) and np.array_equal(b2, a2)
            if own == 64:
                assert np.array_equal(w_own, weights)
    finally:
        ctx.close()
