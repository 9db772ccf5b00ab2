"""CPU-only checks of the model-split calls (ht_split_hands_model*, ht_update_two_hands_model_*): declared, exported and bound with the documented signatures,
refusals that need no device, SplitHandsByModel / TwoHandTracker::split_mode of the C++ header, and what the compiler made of k_split_model."""
import ctypes as C
import os
import subprocess

import numpy as np

import split_model_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_ARGS = "uint16_t range_lo, uint16_t range_hi, uint16_t max_step, int min_pixels, uint16_t far, float max_dist, int mode, int flags"
NEW = {
    "ht_split_hands_model": "ht_ctx *ctx, const uint16_t *depth, const float *cams, const float *poses, int w, int h, int B, " + SPLIT_ARGS +
                            ", uint16_t *depth_out, float *cams_out, int32_t *info, int32_t *n_components, int32_t *source, float *dist, uint16_t *labels",
    "ht_split_hands_model_dev": "ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_poses, int w, int h, int B, " + SPLIT_ARGS +
                                ", uint16_t *d_depth_out, float *d_cams_out, int32_t *d_info, int32_t *d_n_components, int32_t *d_source, float *d_dist, uint16_t *d_labels, void *stream",
    "ht_update_two_hands_model_sync": "ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, int w, int h, float segment_scale, " + SPLIT_ARGS + ", int B, float *poses_out, int32_t *info, int32_t *source, float *cnn_out",
    "ht_update_two_hands_model_dev": "ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, int w, int h, float segment_scale, " + SPLIT_ARGS +
                                     ", const float *d_start_poses, int B, float *d_poses_out, int32_t *d_info, int32_t *d_source, void *stream",
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
    for line in ("#define HT_SPLIT_MODEL_ALWAYS 0", "#define HT_SPLIT_MODEL_MERGED 1", "#define HT_SPLIT_USER_POSES   4"):
        assert line in header
    assert (native.SPLIT_MODEL_ALWAYS, native.SPLIT_MODEL_MERGED, native.SPLIT_USER_POSES) == (R.ALWAYS, R.MERGED, R.USER_POSES) == (0, 1, 4)
    for cite in ("physmodel.h:137-162", "misc_image.h:48"):
        assert cite in header
    assert hasattr(native.Context, "split_hands_model") and hasattr(native.Context, "update_two_hands_model")


def test_calls_refuse_null_contexts_and_a_context_that_never_came_up():
    from hand_tracking_samples_amd import native
    L = native.load()
    d = np.zeros((1, 8, 8), np.uint16); cams = np.zeros((1, 12), np.float32); out = np.zeros((1, 2, 8, 8), np.uint16); co = np.zeros((1, 2, 12), np.float32)
    info = np.zeros((1, 2, 8), np.int32); n = np.zeros(1, np.int32); src = np.zeros(1, np.int32); dist = np.zeros((1, 2, 2, 2), np.float32); lab = np.zeros((1, 2, 2), np.uint16)
    prior = np.zeros((1, 2, 17, 7), np.float32); poses = np.zeros((1, 2, 17, 7), np.float32)
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)); fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 2, 0, C.byref(h))
    try:
        for ctx in (None, h):
            assert L.ht_split_hands_model(ctx, u16(d), fp(cams), fp(prior), 8, 8, 1, 0, 650, 65535, 1, 4000, 1.0, 0, 0, u16(out), fp(co), i32(info), i32(n), i32(src), fp(dist), u16(lab)) != 0
            assert L.ht_split_hands_model_dev(ctx, d.ctypes.data, cams.ctypes.data, prior.ctypes.data, 8, 8, 1, 0, 650, 65535, 1, 4000, 1.0, 0, 0, out.ctypes.data, co.ctypes.data, info.ctypes.data, n.ctypes.data,
                                              src.ctypes.data, dist.ctypes.data, lab.ctypes.data, None) != 0
            assert L.ht_update_two_hands_model_sync(ctx, 64, u16(d), fp(cams), 8, 8, 0.17, 0, 650, 65535, 1, 4000, 1.0, 1, 0, 1, fp(poses), i32(info), i32(src), None) != 0
            assert L.ht_update_two_hands_model_dev(ctx, 64, d.ctypes.data, cams.ctypes.data, 8, 8, 0.17, 0, 650, 65535, 1, 4000, 1.0, 1, 0, None, 1, poses.ctypes.data, info.ctypes.data, src.ctypes.data, None) != 0
        assert not out.any() and not info.any() and not poses.any() and not src.any() and not dist.any() and not lab.any() and not n.any() and not co.any()      # nothing was written
    finally:
        if h:
            L.ht_destroy(h)


def test_a_context_without_a_hand_model_is_refused_with_a_state_error():
    """On a machine with a device a CNN-only context comes up and every model-split call answers HT_ERR_STATE (4) before it looks at anything else; without a device the
    context itself is refused (tests/test_gpu_split_model.py runs this on the device as well)"""
    import torch
    from hand_tracking_samples_amd import native
    if not torch.cuda.is_available():
        try:
            native.Context(None, 2)
        except native.HTError as e:
            assert "no HIP device" in str(e)
            return
        raise AssertionError("a context came up without a device")
    c = native.Context(None, 2)
    try:
        d = np.full((1, 8, 8), 400, np.uint16); cams = np.array([[20, 20, 3.5, 3.5, 0.001, 0, 0, 0, 0, 0, 0, 1]], np.float32)
        for call in (lambda: c.split_hands_model(d, cams, np.zeros((1, 2, 17, 7), np.float32), 0, 650, 4000), lambda: c.update_two_hands_model(d, cams, 0, 650, 4000)):
            try:
                call()
            except native.HTError as e:
                assert "without a hand model" in str(e) and "status 4" in str(e)
            else:
                raise AssertionError("a CNN-only context split by a model it does not have")
    finally:
        c.close()


def test_split_model_facades_compile_and_link(tmp_path):
    """include/ht_handtrack.hpp's SplitHandsByModel and TwoHandTracker::split_mode build with plain g++ against the C-ABI library"""
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "split_model")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_split_model_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "model_hand17.htfx")], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout      # the split needs a tracker's device; no fallback


def test_the_kernel_uses_no_scratch_and_two_blocks_fit_a_cu():
    """One k_split_model, no scratch, no spills; its LDS -- its own tables, plus the face planes of the model, 16 bytes each, as dynamic LDS -- is at most half a CU's
    160 KB for both stock models, and its 512 threads with at most 128 registers let two blocks share a CU's register files."""
    from hand_tracking_samples_amd import build, native
    u = build.resource_usage()
    if not any("k_split_model" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    k = {n: v for n, v in u.items() if "k_split_model" in n}
    print("\n".join("%s VGPRs %d LDS %d occupancy %d" % (n, v["VGPRs"], v["LDS Size"], v["Occupancy"]) for n, v in sorted(k.items())))
    assert len(k) == 1
    v = list(k.values())[0]
    assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0
    assert v["VGPRs"] + v.get("AGPRs", 0) <= 128 and v["Occupancy"] >= 4      # 2 x 512 threads a CU are 4 waves a SIMD: 512 / 4 registers each
    assert v["LDS Size"] % 16 == 0      # the dynamic region behind it (the planes, read 16 bytes at a time) starts 16-byte aligned
    for name in ("model_hand17.htfx", "model_hand26.htfx"):
        m = native.Model(os.path.join(ROOT, "tests", "golden", name))
        try:
            planes = sum(len(m.body(b)[2]) for b in range(m.nb))
        finally:
            m.close()
        lds = v["LDS Size"] + 16 * planes
        print(name, "planes", planes, "LDS", lds)
        assert planes > 1000 and lds <= 80 * 1024
    # the blob split's kernels are what they were: the new kernel lives in an object of its own
    assert len([n for n in u if "k_split_label" in n]) == 1 and not any("k_split_model" in n for n in open(os.path.join(build.OBJDIR, "ht_split.usage.txt")).read().split())
