"""CPU-only checks of the mini-batch training entry points (ht_cnn_train_batch_dev, ht_cnn_train_batch, ht_debug_train_batch_buffers,
include/ht_mi355x.h): exported and declared with the documented signatures, refused before any device work, the ctypes wrappers check the order's
length, and CNN::TrainBatch of include/ht_handtrack.hpp compiles against them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIGNATURES = {
    "ht_cnn_train_batch_dev": "ht_ctx *ctx, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, float alpha, float *d_mse, void *stream",
    "ht_cnn_train_batch": "ht_ctx *ctx, const float *inputs, const float *targets, int n, int batch, float alpha, float *mse_out",
    "ht_debug_train_batch_buffers": "ht_ctx *ctx, int n, float *a3, float *a6, float *a8, float *e9, float *e7, float *e6, float *e3",
}


def test_symbols_exported_and_declared():
    from hand_tracking_samples_amd import native
    L = native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    header = open(os.path.join(ROOT, "include", "ht_mi355x.h")).read()
    for s, args in SIGNATURES.items():
        assert s in native.SYMBOLS and s in exported and hasattr(L, s)
        assert "int %s(%s);" % (s, args) in header, s
        assert len(getattr(L, s).argtypes) == args.count(",") + 1, s
    assert re.search(r"#define HT_TRAIN_MAX_BATCH 256\b", header)
    assert "a SUM, not a mean" in header      # alpha keeps its per-sample meaning: documented where the caller reads it


def test_calls_refuse_null_contexts_and_contexts_that_never_came_up():
    from hand_tracking_samples_amd import native
    L = native.load()
    x = np.zeros((2, 4096), np.float32); t = np.zeros((2, 2304), np.float32); order = np.zeros(2, np.int32); buf = np.zeros(2 * 3600, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = order.ctypes.data_as(C.POINTER(C.c_int))
    assert L.ht_cnn_train_batch_dev(None, x.ctypes.data, t.ctypes.data, 2, ip, 1, 2, 0.001, None, None) != 0
    assert L.ht_cnn_train_batch(None, fp(x), fp(t), 2, 2, 0.001, None) != 0
    assert L.ht_debug_train_batch_buffers(None, 2, *[fp(buf)] * 7) != 0
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))      # no device here, or a missing model: the calls below must fail, not crash
    try:
        bad = np.array([0, 5], np.int32)
        for args in ((x.ctypes.data, t.ctypes.data, 2, ip, 1, 2), (None, t.ctypes.data, 2, ip, 1, 2), (x.ctypes.data, None, 2, ip, 1, 2), (x.ctypes.data, t.ctypes.data, 0, ip, 1, 2),
                     (x.ctypes.data, t.ctypes.data, 2, ip, 1, 0), (x.ctypes.data, t.ctypes.data, 2, ip, 1, 257), (x.ctypes.data, t.ctypes.data, 2, None, 2, 2),
                     (x.ctypes.data, t.ctypes.data, 2, bad.ctypes.data_as(C.POINTER(C.c_int)), 1, 2)):
            assert L.ht_cnn_train_batch_dev(h, *args, 0.001, None, None) != 0
        assert L.ht_cnn_train_batch(h, fp(x), fp(t), 2, 2, 0.001, None) != 0 and L.ht_cnn_train_batch(h, fp(x), fp(t), 2, 0, 0.001, None) != 0
        assert L.ht_debug_train_batch_buffers(h, 2, *[fp(buf)] * 7) != 0
    finally:
        if h:
            L.ht_destroy(h)


def test_wrappers_reject_a_short_order():
    """the length of the order is the wrapper's to check: the C call reads n_steps * batch indices"""
    from hand_tracking_samples_amd import native

    class Stub(native.Context):
        def __init__(self):
            self.calls = 0

            class Lib:
                def ht_cnn_train_batch_dev(_, *a):
                    self.calls += 1
                    return 0
            self.L, self.h = Lib(), None

        def __del__(self):
            pass

    s = Stub()
    with pytest.raises(ValueError):
        s.cnn_train_batch_dev(0, 0, 8, 4, order=[0, 1, 2, 3, 4, 5, 6], n_steps=2)
    with pytest.raises(ValueError):
        s.cnn_train_batch_dev(0, 0, 8, 4, order=[0, 1, 2], n_steps=1)
    assert s.calls == 0
    s.cnn_train_batch_dev(0, 0, 8, 4, order=[0, 1, 2, 3, 4, 5, 6, 7])      # two whole steps
    s.cnn_train_batch_dev(0, 0, 8, 4, order=[0, 1, 2, 3, 4, 5, 6], n_steps=1)
    assert s.calls == 2


def test_trainbatch_of_the_cxx_surface_compiles(tmp_path):
    src = tmp_path / "tb.cpp"
    src.write_text('#include "ht_handtrack.hpp"\n'
                   "void step(ht_mi355x::CNN &cnn, const float *x, const float *t, const std::vector<int> &order, float *mse) { cnn.TrainBatch(x, t, 64, order, 16, 0.001f / 16, mse, nullptr); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
