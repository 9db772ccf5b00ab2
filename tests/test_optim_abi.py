"""CPU-only checks of the gradient and optimiser calls (ht_cnn_grad_*, ht_opt_default, ht_cnn_opt_*, ht_cnn_train_opt_sized_dev): declared and exported with
the documented signatures, ht_opt laid out as the binding lays it out, ht_opt_default's values, refusals before a device is touched, and what the compiler
made of the kernels of csrc/ht_optim.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "ht_cnn_grad_batch_sized_dev": "ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int batch, int accumulate, float *d_mse, void *stream",
    "ht_cnn_grad_batch_sized": "ht_ctx *ctx, int side, const float *inputs, const float *targets, int n, int accumulate, float *mse_out",
    "ht_cnn_grad_get_sized": "ht_ctx *ctx, int side, float *g, size_t n",
    "ht_cnn_grad_set_sized": "ht_ctx *ctx, int side, const float *g, size_t n",
    "ht_cnn_grad_ptr_sized": "ht_ctx *ctx, int side, float **d_g, size_t *n",
    "ht_opt_default": "int kind, ht_opt *o",
    "ht_cnn_opt_step_sized_dev": "ht_ctx *ctx, int side, const ht_opt *o, void *stream",
    "ht_cnn_opt_reset_sized": "ht_ctx *ctx, int side",
    "ht_cnn_opt_state_get_sized": "ht_ctx *ctx, int side, float *m, float *v, size_t n, int *t",
    "ht_cnn_opt_state_set_sized": "ht_ctx *ctx, int side, const float *m, const float *v, size_t n, int t",
    "ht_cnn_opt_last_sized": "ht_ctx *ctx, int side, double *grad_norm, float *clip_factor",
    "ht_cnn_train_opt_sized_dev": "ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, int accum, const ht_opt *o, float *d_mse, void *stream",
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
        assert len(getattr(L, name).argtypes) == args.count(",") + 1, name
    assert "enum { HT_OPT_SGD = 0, HT_OPT_MOMENTUM = 1, HT_OPT_NESTEROV = 2, HT_OPT_ADAM = 3 };" in header
    assert (native.OPT_SGD, native.OPT_MOMENTUM, native.OPT_NESTEROV, native.OPT_ADAM) == (0, 1, 2, 3)


def test_ht_opt_is_laid_out_as_the_binding_lays_it_out(tmp_path):
    """sizeof and every field's offset, from a C translation unit that includes the public header"""
    from hand_tracking_samples_amd import native
    fields = [f for f, _ in native.Opt._fields_]
    src = tmp_path / "opt_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ht_mi355x.h"\nint main(void) { printf("%zu", sizeof(ht_opt));\n'
                   + "".join('printf(" %%zu", offsetof(ht_opt, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "opt_layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(native.Opt) == 40
    assert got[1:] == [getattr(native.Opt, f).offset for f in fields]
    header = open(os.path.join(ROOT, "include", "ht_mi355x.h")).read()
    m = re.search(r"typedef struct ht_opt \{([^}]*)\} ht_opt;", header)
    assert re.findall(r"(\w+)\s*[,;]", m.group(1)) == fields


def test_ht_opt_default_values():
    from hand_tracking_samples_amd import native
    L = native.load()
    for kind in range(4):
        o = native.Opt()
        assert L.ht_opt_default(kind, C.byref(o)) == 0
        got = [getattr(o, f) for f, _ in native.Opt._fields_]
        want = [kind, np.float32(0.001), np.float32(0.9), np.float32(0.9), np.float32(0.999), np.float32(1e-8), 0.0, 0, 1.0, 0.0]
        assert got == [float(x) if isinstance(x, np.float32) else x for x in want], (kind, got)
    assert L.ht_opt_default(4, C.byref(o)) == 1 and L.ht_opt_default(-1, C.byref(o)) == 1 and L.ht_opt_default(0, None) == 1
    assert native.Opt.default("adam", lr=0.01).lr == float(np.float32(0.01)) and native.Opt.default("nesterov").kind == 2
    with pytest.raises(ValueError):
        native.Opt.default("rmsprop")
    with pytest.raises(TypeError):
        native.Opt.default("sgd", nesterov=1)


def test_calls_refuse_null_contexts_and_a_context_that_never_came_up():
    from hand_tracking_samples_amd import native
    L = native.load()
    x = np.zeros((2, 16384), np.float32); t = np.zeros((2, 2304), np.float32); buf = np.zeros(16, np.float32); order = np.zeros(8, np.int32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    o = native.Opt.default("adam")
    p = C.c_void_p(); n = C.c_size_t(); ti = C.c_int(); nrm = C.c_double(); cf = C.c_float()

    def all_calls(h, side):
        return [L.ht_cnn_grad_batch_sized_dev(h, side, x.ctypes.data, t.ctypes.data, 2, ip(order), 2, 0, None, None),
                L.ht_cnn_grad_batch_sized(h, side, fp(x), fp(t), 2, 0, None),
                L.ht_cnn_grad_get_sized(h, side, fp(buf), 16), L.ht_cnn_grad_set_sized(h, side, fp(buf), 16), L.ht_cnn_grad_ptr_sized(h, side, C.byref(p), C.byref(n)),
                L.ht_cnn_opt_step_sized_dev(h, side, C.byref(o), None), L.ht_cnn_opt_reset_sized(h, side),
                L.ht_cnn_opt_state_get_sized(h, side, fp(buf), fp(buf), 16, C.byref(ti)), L.ht_cnn_opt_state_set_sized(h, side, fp(buf), fp(buf), 16, 0),
                L.ht_cnn_opt_last_sized(h, side, C.byref(nrm), C.byref(cf)),
                L.ht_cnn_train_opt_sized_dev(h, side, x.ctypes.data, t.ctypes.data, 2, ip(order), 2, 2, 2, C.byref(o), None, None)]
    for side in (64, 128, 96):
        assert all(r != 0 for r in all_calls(None, side)), side
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    try:
        for side in (64, 128, 96):
            assert all(r != 0 for r in all_calls(h, side)), side
    finally:
        if h:
            L.ht_destroy(h)


class _Refusing:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called %s" % name)


def test_wrappers_reject_a_short_order_and_an_unknown_side():
    from hand_tracking_samples_amd import native
    ctx = native.Context.__new__(native.Context)
    ctx.L = _Refusing(); ctx.h = None
    o = native.Opt.default("sgd")
    with pytest.raises(ValueError, match="order"):
        ctx.cnn_grad_batch_dev(0, 0, 5, 5, order=[0, 1, 2])
    with pytest.raises(ValueError, match="order"):
        ctx.cnn_train_opt_dev(0, 0, 20, 5, o, accum=2, order=list(range(19)), n_steps=2)
    for call in (lambda: ctx.cnn_grad_batch(np.zeros((1, 9216)), np.zeros((1, 2304)), side=96), lambda: ctx.cnn_grad_batch_dev(0, 0, 5, 5, side=96), lambda: ctx.cnn_grad_get(side=96),
                 lambda: ctx.cnn_grad_set(np.zeros(4), side=96), lambda: ctx.cnn_grad_ptr(side=96), lambda: ctx.cnn_opt_step(o, side=96), lambda: ctx.cnn_opt_reset(side=96),
                 lambda: ctx.cnn_opt_state(side=96), lambda: ctx.cnn_opt_set_state(t=1, side=96), lambda: ctx.cnn_opt_last(side=96), lambda: ctx.cnn_train_opt_dev(0, 0, 5, 5, o, side=96)):
        with pytest.raises(ValueError, match="64 or 128"):
            call()


def test_no_optimiser_kernel_uses_scratch_or_spills_and_the_parents_counts_hold():
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not u:
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    ko = {k: v for k, v in u.items() if "k_opt_" in k}
    print("\n".join("%s VGPRs %d AGPRs %d LDS %d occupancy %d" % (k, v["VGPRs"], v["AGPRs"], v["LDS Size"], v["Occupancy"]) for k, v in sorted(ko.items())))
    for part in ("k_opt_fc_wgrad", "k_opt_conv_reduce", "k_opt_normPK", "k_opt_norm_final", "k_opt_pack_w2"):
        assert len([k for k in ko if part in k]) == 1, part
    assert len([k for k in ko if "k_opt_stepILi" in k]) == 4      # one per kind
    for k, v in ko.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    # the gradient kernel keeps its tile where the fused step keeps it: 16 accumulator registers of one 32x32 MFMA tile, no more VGPRs than the kernel that also holds W
    new = next(v for k, v in ko.items() if "k_opt_fc_wgrad" in k); old = next(v for k, v in u.items() if "k_tb_fc_wgrad" in k)
    assert new["AGPRs"] == old["AGPRs"] and (new["AGPRs"] >= 16 or new["VGPRs"] >= 16), (new, old)
    assert new["Occupancy"] >= old["Occupancy"]
    # the parent's instantiations of the mini-batch kernels: no new template parameters, no new instantiations
    tb = {k: v for k, v in u.items() if "k_tb_" in k}
    assert len([k for k in tb if "ILi64E" in k]) == 4
    for part in ("k_tb_conv1_tanh_poolILi128E", "k_tb_conv2_tanh_poolILi128E", "k_tb_conv2_backILi128E", "k_tb_conv_gradILi128E"):
        assert len([k for k in tb if part in k]) == 1, part
    assert len([k for k in tb if "k_tb_fc_wgrad" in k]) == 1 and len([k for k in tb if "k_tb_conv_apply" in k]) == 1


def test_cxx_optim_example_compiles_and_refuses_without_arguments(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "optim")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_optim_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
