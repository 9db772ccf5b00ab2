"""CPU-only checks of the keypoint fit (ht_kpfit_default, ht_fit_keypoints, ht_fit_keypoints_dev): declared, exported and bound with the documented signatures, the
refusals that need no device, the addition of the C++ header, and what the compiler made of the kernel."""
import ctypes as C
import os
import subprocess

import numpy as np

import kpfit_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = "int which, int K, const int *bones, const float *offsets, const int *rel"
NEW = {
    "ht_kpfit_default": "ht_kpfit *o",
    "ht_fit_keypoints": "ht_ctx *ctx, int which_model, int B, " + TABLE + ", const int *kind, const float *xyz, const float *pix, const float *weights, const float *cams, const ht_kpfit *o, float *poses, float *resid",
    "ht_fit_keypoints_dev": "ht_ctx *ctx, int which_model, int B, " + TABLE + ", const int *kind, const float *d_xyz, const float *d_pix, const float *d_weights, const float *d_cams, const ht_kpfit *o, float *d_poses, float *d_resid, void *stream",
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
    assert "#define HT_KPFIT_KEEP_MOMENTA 1" in header and native.KPFIT_KEEP_MOMENTA == kr.KEEP_MOMENTA == 1
    assert "typedef struct { int steps; float max_force, ray_radius, ray_force; int flags; } ht_kpfit;" in header
    assert [f[0] for f in native.KpFit._fields_] == ["steps", "max_force", "ray_radius", "ray_force", "flags"] and C.sizeof(native.KpFit) == 20
    for cite in ("physics.h:342-346", "physics.h:337-338", "misc_image.h:48", "handtrack.h:672", "handtrack.h:686-687", "ht_mirror_poses", "prepared points empty"):
        assert cite in header, cite
    for method in ("fit_keypoints", "fit_keypoints_dev"):
        assert callable(getattr(native.Context, method)), method
    # slowfit's figures
    o = native.kpfit_default()
    assert (o.steps, o.max_force, o.ray_radius, o.ray_force, o.flags) == (6, np.float32(kr.FLT_MAX), np.float32(0.01), 100000.0, 0)
    assert native.kpfit_default(keep_momenta=True, steps=3).flags == 1
    assert L.ht_kpfit_default(None) != 0


def test_calls_refuse_null_contexts_and_a_context_that_never_came_up():
    from hand_tracking_samples_amd import native
    L = native.load()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    xyz = np.zeros((1, 8, 3), np.float32); poses = np.zeros((1, 17, 7), np.float32); resid = np.zeros((1, 2, 8), np.float32)
    o = native.kpfit_default()
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 2, 0, C.byref(h))
    try:
        for ctx in (None, h):
            assert L.ht_fit_keypoints(ctx, 0, 1, 0, 0, None, None, None, None, fp(xyz), None, None, None, C.byref(o), fp(poses), fp(resid)) != 0
            assert L.ht_fit_keypoints_dev(ctx, 0, 1, 0, 0, None, None, None, None, xyz.ctypes.data, None, None, None, C.byref(o), poses.ctypes.data, resid.ctypes.data, None) != 0
        assert not poses.any() and not resid.any()      # nothing was written
    finally:
        if h:
            L.ht_destroy(h)


def test_kpfit_addition_of_the_cxx_header_compiles_and_links(tmp_path):
    """include/ht_handtrack.hpp's HandTracker::fit_keypoints with KeypointFit / KeypointTargets builds with plain g++ against the C-ABI library"""
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "kpfit")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_kpfit_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "model_hand17.htfx"), "none", "none"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout      # it runs on a tracker's device; no fallback


def test_kpfit_kernel_resources():
    """one k_keypoint_rows: a wave a frame without scratch, spills or LDS, within 64 VGPRs"""
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not any("k_keypoint_rows" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    k = {n: v for n, v in u.items() if "k_keypoint_rows" in n}
    assert len(k) == 1
    for n, v in k.items():
        print("%s VGPRs %d LDS %d scratch %d" % (n, v["VGPRs"], v["LDS Size"], v["ScratchSize"]))
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["LDS Size"] == 0 and v["VGPRs"] <= 64, (n, v)
