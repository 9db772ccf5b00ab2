"""CPU-only checks of the two-hand calls (ht_split_hands*, ht_update_two_hands_*): declared, exported and bound with the documented signatures, refusals that need no
device, SplitHands / TwoHandTracker of the C++ header, and what the compiler made of the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np

import split_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_ARGS = "uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, int flags"
NEW = {
    "ht_split_hands": "ht_ctx *ctx, const uint16_t *depth, const float *cams, int w, int h, int B, " + SPLIT_ARGS + ", uint16_t *depth_out, float *cams_out, int32_t *info, int32_t *n_components, uint16_t *labels",
    "ht_split_hands_dev": "ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, " + SPLIT_ARGS + ", uint16_t *d_depth_out, float *d_cams_out, int32_t *d_info, int32_t *d_n_components, uint16_t *d_labels, void *stream",
    "ht_update_two_hands_sync": "ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, " + SPLIT_ARGS + ", int B, float *poses_out, int32_t *info, float *cnn_out",
    "ht_update_two_hands_dev": "ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, " + SPLIT_ARGS + ", const float *d_start_poses, int B, float *d_poses_out, int32_t *d_info, void *stream",
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
    assert "#define HT_SPLIT_RIGHT_IS_LOW_X 1" in header and "#define HT_SPLIT_MIRROR_LEFT 2" in header
    assert (native.SPLIT_RIGHT_IS_LOW_X, native.SPLIT_MIRROR_LEFT) == (S.RIGHT_IS_LOW_X, S.MIRROR_LEFT) == (1, 2)
    for cite in ("handtrack.h:280-344", "handtrack.h:285", ":287", ":343"):
        assert cite in header


def test_calls_refuse_null_contexts_and_a_context_that_never_came_up():
    from hand_tracking_samples_amd import native
    L = native.load()
    d = np.zeros((1, 8, 8), np.uint16); cams = np.zeros((1, 12), np.float32); out = np.zeros((1, 2, 8, 8), np.uint16); co = np.zeros((1, 2, 12), np.float32)
    info = np.zeros((1, 2, 8), np.int32); n = np.zeros(1, np.int32); lab = np.zeros((1, 2, 2), np.uint16); poses = np.zeros((1, 2, 17, 7), np.float32)
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)); fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 2, 0, C.byref(h))
    try:
        for ctx in (None, h):
            assert L.ht_split_hands(ctx, u16(d), fp(cams), 8, 8, 1, 0, 650, 65535, 1, 4000, 0, u16(out), fp(co), i32(info), i32(n), u16(lab)) != 0
            assert L.ht_split_hands_dev(ctx, d.ctypes.data, cams.ctypes.data, 8, 8, 1, 0, 650, 65535, 1, 4000, 0, out.ctypes.data, co.ctypes.data, info.ctypes.data, n.ctypes.data, lab.ctypes.data, None) != 0
            assert L.ht_update_two_hands_sync(ctx, 64, u16(d), fp(cams), 8, 8, 0.17, 0, 650, 65535, 1, 4000, 0, 1, fp(poses), i32(info), None) != 0
            assert L.ht_update_two_hands_dev(ctx, 64, d.ctypes.data, cams.ctypes.data, 8, 8, 0.17, 0, 650, 65535, 1, 4000, 0, None, 1, poses.ctypes.data, info.ctypes.data, None) != 0
        assert not out.any() and not info.any() and not poses.any()      # nothing was written
    finally:
        if h:
            L.ht_destroy(h)


def test_split_facades_compile_and_link(tmp_path):
    """include/ht_handtrack.hpp's SplitHands and TwoHandTracker build with plain g++ against the C-ABI library"""
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "split")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_split_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "model_hand17.htfx")], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout      # the split needs a tracker's device; no fallback


def test_split_kernels_use_no_scratch_and_the_label_kernel_fits_two_blocks_a_cu():
    """The instantiations: one k_split_label, one k_split_cams, and k_split_write for 16, 8 and 4 bytes a thread and for single pixels (<4>, <2>, <1>, <0>)."""
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not any("k_split" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    k = {n: v for n, v in u.items() if "k_split" in n}
    print("\n".join("%s VGPRs %d LDS %d occupancy %d" % (n, v["VGPRs"], v["LDS Size"], v["Occupancy"]) for n, v in sorted(k.items())))
    assert len([n for n in k if "k_split_label" in n]) == 1 and len([n for n in k if "k_split_cams" in n]) == 1
    writes = sorted(n for n in k if "k_split_write" in n)
    assert len(writes) == 4 and all(any("k_split_writeILi%dE" % i in n for n in writes) for i in (0, 1, 2, 4)), writes
    for n, v in k.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (n, v)
    label = [v for n, v in k.items() if "k_split_label" in n][0]
    assert 2 * 19200 * 2 <= label["LDS Size"] <= 80 * 1024      # Q and the labels, and two blocks in a CU's 160 KB
    assert label["VGPRs"] <= 64      # 2 x 1024 threads a CU are 8 waves a SIMD: 512 / 8 registers each
