"""CPU-only checks of the sensor-filter calls (ht_sensor_*): declared, exported and bound with the documented signatures, ht_sensor_out_dims against the
restatement, refusals that need no device, the RSCam facade of the C++ header, and what the compiler made of the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sensor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "ht_sensor_out_dims": "int kind, int w, int h, int max_width, int *w_out, int *h_out",
    "ht_sensor_filter": "ht_ctx *ctx, int kind, const uint16_t *depth, const uint8_t *ir, const float *cams, int w, int h, int B, int max_width, const uint16_t *background, uint16_t *depth_out, float *cams_out",
    "ht_sensor_filter_dev": "ht_ctx *ctx, int kind, const uint16_t *d_depth, const uint8_t *d_ir, const float *d_cams, int w, int h, int B, int max_width, const uint16_t *d_background, uint16_t *d_depth_out, float *d_cams_out, void *stream",
    "ht_sensor_background": "ht_ctx *ctx, const uint16_t *depth, int w, int h, int B, int fudge, int init, uint16_t *background",
    "ht_sensor_background_dev": "ht_ctx *ctx, const uint16_t *d_depth, int w, int h, int B, int fudge, int init, uint16_t *d_background, void *stream",
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
    assert "#define HT_SENSOR_IVY 0" in header and "#define HT_SENSOR_DS4 1" in header and (native.SENSOR_IVY, native.SENSOR_DS4) == (R.IVY, R.DS4) == (0, 1)
    for cite in ("dcam.h:209-226", "dcam.h:174-208", "dcam.h:157-162"):
        assert cite in header


def test_out_dims_follows_the_restatement_and_refuses_what_it_refuses():
    from hand_tracking_samples_amd import native
    L = native.load()
    cases = [(kind, w, h, mw) for kind in (0, 1, 2, -1) for (w, h) in ((640, 480), (320, 240), (1280, 960), (36, 20), (642, 480), (640, 481), (322, 240), (4, 4), (1, 1), (0, 4), (4, 0), (4096, 4096), (4097, 4), (4, 4097), (76, 20))
             for mw in (320, 9, 1, 0, -3, 4096, 160)]
    refused = 0
    for kind, w, h, mw in cases:
        wo, ho = C.c_int(-1), C.c_int(-1)
        rc = L.ht_sensor_out_dims(kind, w, h, mw, C.byref(wo), C.byref(ho))
        try:
            want = R.out_dims(kind, w, h, mw)
        except ValueError:
            want = None
        if want is None:
            refused += 1
            assert rc == 1 and (wo.value, ho.value) == (-1, -1), (kind, w, h, mw)
            with pytest.raises(ValueError):
                native.sensor_out_dims(kind, w, h, mw)
        else:
            assert rc == 0 and (wo.value, ho.value) == want == native.sensor_out_dims(kind, w, h, mw), (kind, w, h, mw)
    assert 50 < refused < len(cases) - 50
    assert L.ht_sensor_out_dims(0, 640, 480, 320, None, None) == 1


def test_calls_refuse_null_contexts_and_a_context_that_never_came_up():
    from hand_tracking_samples_amd import native
    L = native.load()
    d = np.zeros((2, 16), np.uint16); ir = np.zeros((2, 16), np.uint8); cams = np.zeros((2, 12), np.float32); out = np.zeros((2, 16), np.uint16); co = np.zeros((2, 12), np.float32)
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)); u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)); fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    try:
        for ctx in (None, h):
            for kind in (0, 1):
                assert L.ht_sensor_filter(ctx, kind, u16(d), u8(ir), fp(cams), 4, 4, 2, 320, None, u16(out), fp(co)) != 0
                assert L.ht_sensor_filter_dev(ctx, kind, d.ctypes.data, ir.ctypes.data, cams.ctypes.data, 4, 4, 2, 320, None, out.ctypes.data, co.ctypes.data, None) != 0
            assert L.ht_sensor_background(ctx, u16(d), 4, 4, 2, 3, 1, u16(out)) != 0
            assert L.ht_sensor_background_dev(ctx, d.ctypes.data, 4, 4, 2, 3, 1, out.ctypes.data, None) != 0
    finally:
        if h:
            L.ht_destroy(h)


def test_rscam_facade_compiles_and_links(tmp_path):
    """include/ht_handtrack.hpp's RSCam (FilterDS4 / FilterIvy / addbackground / image_width_max_allowed) builds with plain g++ against the C-ABI library"""
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "sensor")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_sensor_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "model_hand17.htfx")], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout      # out_dims answered without a device; the filters fail loudly, no fallback


def test_no_sensor_kernel_uses_scratch_or_spills():
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not u:
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    k = {n: v for n, v in u.items() if "k_sensor" in n}
    print("\n".join("%s VGPRs %d LDS %d occupancy %d" % (n, v["VGPRs"], v["LDS Size"], v["Occupancy"]) for n, v in sorted(k.items())))
    for part in ("k_sensor_ds4", "k_sensor_ivy", "k_sensor_background", "k_sensor_cams"):
        assert len([n for n in k if part in n]) == 1, part
    for n, v in k.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (n, v)
