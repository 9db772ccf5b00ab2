"""CPU-only checks of the accuracy calls (ht_keypoint_table, ht_keypoints*, ht_keypoint_errors*, ht_depth_compare*, ht_pose_depth_residual*): declared, exported and bound
with the documented signatures, refusals that need no device, the additions of the C++ header, and what the compiler made of the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np

import quality_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = "int which, int K, const int *bones, const float *offsets, const int *rel"
NEW = {
    "ht_keypoint_table": "ht_ctx *ctx, int which, int *K, int *bones, float *offsets, int *rel",
    "ht_keypoints": "ht_ctx *ctx, const float *poses, int B, int flags, " + TABLE + ", const uint8_t *hands, const float *cams, const uint16_t *depth, int w, int h, float near_tol, float far_tol, float *xyz, float *pix, float *zc, uint8_t *vis",
    "ht_keypoints_dev": "ht_ctx *ctx, const float *d_poses, int B, int flags, " + TABLE + ", const uint8_t *d_hands, const float *d_cams, const uint16_t *d_depth, int w, int h, float near_tol, float far_tol, float *d_xyz, float *d_pix, float *d_zc, uint8_t *d_vis, void *stream",
    "ht_keypoint_errors": "ht_ctx *ctx, const float *a, const float *b, int B, int K, const float *thr, int T, float *dist, float *frame, double *sum_kp, int64_t *hits_kp, int64_t *hits_frame",
    "ht_keypoint_errors_dev": "ht_ctx *ctx, const float *d_a, const float *d_b, int B, int K, const float *thr, int T, float *d_dist, float *d_frame, double *d_sum_kp, int64_t *d_hits_kp, int64_t *d_hits_frame, void *stream",
    "ht_depth_compare": "ht_ctx *ctx, const uint16_t *a, const uint16_t *b, int w, int h, int B, int lo, int hi, int tol, int64_t *info",
    "ht_depth_compare_dev": "ht_ctx *ctx, const uint16_t *d_a, const uint16_t *d_b, int w, int h, int B, int lo, int hi, int tol, int64_t *d_info, void *stream",
    "ht_pose_depth_residual": "ht_ctx *ctx, const float *poses, const float *cams, const uint16_t *depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *info, uint16_t *rendered",
    "ht_pose_depth_residual_dev": "ht_ctx *ctx, const float *d_poses, const float *d_cams, const uint16_t *d_depth, int w, int h, int B, int flags, float far, int lo, int hi, int tol, int64_t *d_info, uint16_t *d_rendered, void *stream",
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
    for d in ("HT_KP_COM_POSES 1", "HT_KP_FEATURE8 0", "HT_KP_SKELETON 1", "HT_KP_CALLER 2", "HT_KP_MAX 64", "HT_KP_MAX_THR 32"):
        assert "#define " + d in header
    assert (native.KP_COM_POSES, native.KP_FEATURE8, native.KP_SKELETON) == (Q.COM_POSES, Q.FEATURE8, Q.SKELETON) == (1, 0, 1)
    assert (native.KP_CALLER, native.KP_MAX, native.KP_MAX_THR) == (2, 64, 32)
    for cite in ("handtrack.h:77-81", "handtrack.h:82-84", "handtrack.h:92-96", ":632-634", "dataexporter.cpp:82,105", "annotation-fixer.cpp:315-317", "misc_image.h:48", "physics.h:142"):
        assert cite in header, cite
    for method in ("keypoint_table", "keypoints", "keypoints_dev", "keypoint_errors", "keypoint_errors_dev", "depth_compare", "depth_compare_dev", "pose_depth_residual", "pose_depth_residual_dev"):
        assert callable(getattr(native.Context, method)), method


def test_calls_refuse_null_contexts_and_a_context_that_never_came_up():
    from hand_tracking_samples_amd import native
    L = native.load()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)); u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    poses = np.zeros((1, 17, 7), np.float32); poses[..., 6] = 1; cams = np.zeros((1, 12), np.float32); cams[0, :5] = (8, 8, 4, 4, 0.001); cams[0, 11] = 1
    d = np.zeros((1, 8, 8), np.uint16); xyz = np.zeros((1, 8, 3), np.float32); pix = np.zeros((1, 8, 2), np.float32); zc = np.zeros((1, 8), np.float32); vis = np.zeros((1, 8), np.uint8)
    dist = np.zeros((1, 8), np.float32); frame = np.zeros((1, 2), np.float32); sk = np.zeros(8, np.float64); hk = np.zeros(1, np.int64); hf = np.zeros(1, np.int64)
    thr = np.array([0.02], np.float32); info = np.zeros((1, 8), np.int64); rend = np.zeros((1, 8, 8), np.uint16)
    K = C.c_int(-1); bones = np.zeros(64, np.int32); off = np.zeros((64, 3), np.float32); rel = np.zeros(64, np.int32)
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 2, 0, C.byref(h))
    try:
        for ctx in (None, h):
            assert L.ht_keypoint_table(ctx, 0, C.byref(K), ip(bones), fp(off), ip(rel)) != 0
            assert L.ht_keypoints(ctx, fp(poses), 1, 0, 0, 0, None, None, None, None, fp(cams), u16(d), 8, 8, 0.03, 0.02, fp(xyz), fp(pix), fp(zc), u8(vis)) != 0
            assert L.ht_keypoints_dev(ctx, poses.ctypes.data, 1, 0, 0, 0, None, None, None, None, cams.ctypes.data, d.ctypes.data, 8, 8, 0.03, 0.02, xyz.ctypes.data, pix.ctypes.data, zc.ctypes.data, vis.ctypes.data, None) != 0
            assert L.ht_keypoint_errors(ctx, fp(xyz), fp(xyz), 1, 8, fp(thr), 1, fp(dist), fp(frame), sk.ctypes.data_as(C.POINTER(C.c_double)), i64(hk), i64(hf)) != 0
            assert L.ht_keypoint_errors_dev(ctx, xyz.ctypes.data, xyz.ctypes.data, 1, 8, fp(thr), 1, dist.ctypes.data, frame.ctypes.data, sk.ctypes.data, hk.ctypes.data, hf.ctypes.data, None) != 0
            assert L.ht_depth_compare(ctx, u16(d), u16(d), 8, 8, 1, 0, 650, 0, i64(info)) != 0
            assert L.ht_depth_compare_dev(ctx, d.ctypes.data, d.ctypes.data, 8, 8, 1, 0, 650, 0, info.ctypes.data, None) != 0
            assert L.ht_pose_depth_residual(ctx, fp(poses), fp(cams), u16(d), 8, 8, 1, 0, 4.0, 0, 650, 0, i64(info), u16(rend)) != 0
            assert L.ht_pose_depth_residual_dev(ctx, poses.ctypes.data, cams.ctypes.data, d.ctypes.data, 8, 8, 1, 0, 4.0, 0, 650, 0, info.ctypes.data, rend.ctypes.data, None) != 0
        for a in (xyz, pix, zc, vis, dist, frame, sk, hk, hf, info, rend, bones, off, rel):
            assert not a.any()      # nothing was written
        assert K.value == -1
    finally:
        if h:
            L.ht_destroy(h)


def test_quality_additions_of_the_cxx_header_compile_and_link(tmp_path):
    """include/ht_handtrack.hpp's Skin, ImageFeaturePoints, GetKeypoints, keypoints and depth_residual build with plain g++ against the C-ABI library"""
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "quality")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_quality_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "model_hand17.htfx")], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout      # they run on a tracker's device; no fallback


def test_quality_kernels_resources():
    """One k_keypoints, one error kernel, one conversion kernel; k_depth_compare for 16, 8 and 4 bytes a thread and for single pixels (<4>, <2>, <1>, <0>), each without
    scratch or spills and within 64 VGPRs (eight waves a SIMD: the byte mover hides its loads behind other waves)."""
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not any("k_depth_compare" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    k = {n: v for n, v in u.items() if any(s in n for s in ("k_keypoints", "k_kp_errors", "k_depth_compare", "k_pose_to_render"))}
    print("\n".join("%s VGPRs %d LDS %d scratch %d" % (n, v["VGPRs"], v["LDS Size"], v["ScratchSize"]) for n, v in sorted(k.items())))
    for one in ("k_keypoints", "k_kp_errors", "k_pose_to_render"):
        assert len([n for n in k if one in n]) == 1, one
    cmp_ = sorted(n for n in k if "k_depth_compare" in n)
    assert len(cmp_) == 4 and all(any("k_depth_compareILi%dE" % i in n for n in cmp_) for i in (0, 1, 2, 4)), cmp_
    for n in cmp_:
        v = k[n]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs"] <= 64, (n, v)
    for n, v in k.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (n, v)
    reserved = ("k_solve", "k_reset", "k_cloud_rows", "k_fit_error", "k_contacts_coop", "k_conv1", "k_conv2", "k_fcI", "k_fc144")      # tests/test_build_resources.py finds its kernels by these
    assert not any(r in n for n in k for r in reserved)
