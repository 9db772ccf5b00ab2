"""CPU-only checks of the sized training calls (ht_cnn_train_batch_sized*, ht_cnn_get_weights_sized, ht_debug_train_batch_buffers_sized,
ht_cnn_input_sized_dev, HT_LABELS_SIDE128): declared and exported with the documented signatures, refusing what they must before a device is touched,
and what the compiler made of the mini-batch kernels of either net."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "ht_cnn_train_batch_sized_dev": "ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, float alpha, float *d_mse, void *stream",
    "ht_cnn_train_batch_sized": "ht_ctx *ctx, int side, const float *inputs, const float *targets, int n, int batch, float alpha, float *mse_out",
    "ht_cnn_get_weights_sized": "ht_ctx *ctx, int side, float *w, size_t n",
    "ht_debug_train_batch_buffers_sized": "ht_ctx *ctx, int side, int n, float *a3, float *a6, float *a8, float *e9, float *e7, float *e6, float *e3",
    "ht_cnn_input_sized_dev": "ht_ctx *ctx, int side, const uint16_t *d_tiles, const float *d_cams, int B, float *d_cnn_in, void *stream",
}


def test_symbols_are_declared_exported_and_bound():
    from hand_tracking_samples_amd import native
    L = native.load()
    header = open(os.path.join(ROOT, "include", "ht_mi355x.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    for name, args in NEW.items():
        assert "int %s(%s);" % (name, args) in header, name
        assert name in exported and name in native.SYMBOLS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == args.count(",") + 1, name      # the binding takes as many arguments as the declaration
    assert re.search(r"#define HT_LABELS_SIDE128 2\b", header) and native.LABELS_SIDE128 == 2
    assert native.CNN128_IN == 128 * 128 and re.search(r"#define HT_CNNB128_COUNT %d\b" % native.CNNB128_COUNT, header)
    assert L.ht_cnn_train_batch_sized_dev.argtypes[1] is C.c_int and L.ht_cnn_get_weights_sized.argtypes[3] is C.c_size_t


def test_calls_refuse_null_contexts_and_a_context_that_never_came_up():
    from hand_tracking_samples_amd import native
    L = native.load()
    x = np.zeros((2, 16384), np.float32); t = np.zeros((2, 2304), np.float32); tiles = np.zeros((2, 16384), np.uint16); cams = np.zeros((2, 12), np.float32)
    wbuf = np.zeros(16, np.float32); order = np.zeros(2, np.int32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    seven = [fp(wbuf)] * 7
    for side in (64, 128, 96):
        assert L.ht_cnn_train_batch_sized_dev(None, side, x.ctypes.data, t.ctypes.data, 2, ip(order), 1, 2, 0.001, None, None) != 0
        assert L.ht_cnn_train_batch_sized(None, side, fp(x), fp(t), 2, 2, 0.001, None) != 0
        assert L.ht_cnn_get_weights_sized(None, side, fp(wbuf), 16) != 0
        assert L.ht_debug_train_batch_buffers_sized(None, side, 1, *seven) != 0
        assert L.ht_cnn_input_sized_dev(None, side, tiles.ctypes.data, cams.ctypes.data, 1, x.ctypes.data, None) != 0
    # a context that never came up (no device here, or a missing model): every argument cnn_train_check looks at, side 96 and side 128 without weights must fail, not crash
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    try:
        bad = np.array([0, 5], np.int32)
        for side in (128, 96, 64):
            for args in ((x.ctypes.data, t.ctypes.data, 2, ip(order), 1, 2), (None, t.ctypes.data, 2, ip(order), 1, 2), (x.ctypes.data, None, 2, ip(order), 1, 2),
                         (x.ctypes.data, t.ctypes.data, 0, ip(order), 1, 2), (x.ctypes.data, t.ctypes.data, 2, ip(order), -1, 2), (x.ctypes.data, t.ctypes.data, 2, ip(order), 1, 0),
                         (x.ctypes.data, t.ctypes.data, 2, ip(order), 1, 257), (x.ctypes.data, t.ctypes.data, 2, None, 2, 2), (x.ctypes.data, t.ctypes.data, 2, ip(bad), 1, 2)):
                assert L.ht_cnn_train_batch_sized_dev(h, side, *args, 0.001, None, None) != 0, (side, args)
            for args in ((fp(x), fp(t), 2, 2), (None, fp(t), 2, 2), (fp(x), None, 2, 2), (fp(x), fp(t), 0, 2), (fp(x), fp(t), 2, 0), (fp(x), fp(t), 2, 257)):
                assert L.ht_cnn_train_batch_sized(h, side, *args, 0.001, None) != 0, (side, args)
            assert L.ht_cnn_get_weights_sized(h, side, fp(wbuf), 16) != 0 and L.ht_cnn_get_weights_sized(h, side, None, 16) != 0
            assert L.ht_debug_train_batch_buffers_sized(h, side, 1, *seven) != 0
            for args in ((tiles.ctypes.data, cams.ctypes.data, 1, x.ctypes.data), (None, cams.ctypes.data, 1, x.ctypes.data), (tiles.ctypes.data, None, 1, x.ctypes.data),
                         (tiles.ctypes.data, cams.ctypes.data, 1, None), (tiles.ctypes.data, cams.ctypes.data, -1, x.ctypes.data), (tiles.ctypes.data + 2, cams.ctypes.data, 1, x.ctypes.data)):
                assert L.ht_cnn_input_sized_dev(h, side, *args, None) != 0, (side, args)
    finally:
        if h:
            L.ht_destroy(h)


class _Refusing:
    """stands where the library would: a wrapper that reaches it has not rejected its arguments"""
    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s" % name)


def test_wrappers_reject_a_short_order_and_an_unknown_side():
    from hand_tracking_samples_amd import native
    ctx = native.Context.__new__(native.Context)
    ctx.L = _Refusing(); ctx.h = None
    for side in (64, 128):
        with pytest.raises(ValueError, match="order"):
            ctx.cnn_train_batch_dev(0, 0, 5, 5, order=[0, 1, 2], n_steps=1, side=side)
    for call in (lambda: ctx.cnn_train_batch_dev(0, 0, 5, 5, side=96), lambda: ctx.cnn_train_batch(np.zeros((1, 9216)), np.zeros((1, 2304)), 1, side=96),
                 lambda: ctx.cnn_get_weights(side=96), lambda: ctx.cnn_train_batch_buffers(1, side=96), lambda: ctx.cnn_input_dev(0, 0, 1, 0, side=96),
                 lambda: ctx.expected_cnn_dev(0, 0, 1, 0, side=96)):
        with pytest.raises(ValueError, match="64 or 128"):
            call()


def test_no_mini_batch_kernel_of_either_net_uses_scratch_or_spills():
    """every instantiation ht_train_batch.hip launches, the 64x64-input ones and the new 128x128-input ones; the larger net's conv kernels fit a CU's 160 KB of LDS"""
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not u:
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    tb = {k: v for k, v in u.items() if "k_tb_" in k}
    sized = {k: v for k, v in tb.items() if "ILi128E" in k}
    print("\n".join("%s VGPRs %d AGPRs %d LDS %d occupancy %d" % (k, v["VGPRs"], v["AGPRs"], v["LDS Size"], v["Occupancy"]) for k, v in sorted(tb.items())))
    for part in ("k_tb_conv1_tanh_poolILi128E", "k_tb_conv2_tanh_poolILi128E", "k_tb_conv2_backILi128E", "k_tb_conv_gradILi128E"):
        assert len([k for k in sized if part in k]) == 1, part
    assert len([k for k in tb if "ILi64E" in k]) == 4
    for k, v in tb.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["LDS Size"] <= 160 * 1024, (k, v)
