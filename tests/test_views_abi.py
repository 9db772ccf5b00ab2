"""CPU-only checks of the several-views calls (include/ht_mi355x.h "several views"): declared, exported and bound with the documented signatures, and every refusal that
needs no device is made without one: a context that never came up names the argument it refuses before it reports itself."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "ht_views_default": "ht_ctx *ctx, ht_views *o",
    "ht_fuse_views": "ht_ctx *ctx, const uint16_t *depth, const float *cams, const float *planes, int w, int h, int V, int B, const ht_views *o, float *points, int cap, int *npoints, int *per_source, float *origins, int *cut",
    "ht_fuse_views_dev": "ht_ctx *ctx, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, int B, const ht_views *o, int *d_npoints, int *d_per_source, float *d_origins, int *d_cut, void *stream",
    "ht_stage_view_rows": "ht_ctx *ctx, int which, int B, float *rows, int cap, int *nrows",
    "ht_fit_views": "ht_ctx *ctx, int which, int B, int passes, float *poses",
    "ht_fit_views_dev": "ht_ctx *ctx, int which, int B, int passes, float *d_poses, void *stream",
    "ht_update_views_sync": "ht_ctx *ctx, int side, const uint16_t *depth, const float *cams, const float *planes, int w, int h, int V, float segment_scale, int B, const ht_views *o, int passes, float *poses_out, float *cnn_out",
    "ht_update_views_dev": "ht_ctx *ctx, int side, const uint16_t *d_depth, const float *d_cams, const float *d_planes, int w, int h, int V, float segment_scale, const float *d_start_poses, int B, const ht_views *o, int passes, float *d_poses_out, void *stream",
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
    assert "#define HT_VIEWS_MAX 4" in header and native.VIEWS_MAX == 4
    assert "typedef struct { float range_lo, range_hi; int fraction; float mirror_eps; } ht_views;" in header
    assert [f[0] for f in native.Views._fields_] == ["range_lo", "range_hi", "fraction", "mirror_eps"]
    for cite in ("misc_image.h:401-485", "dataset.h:24,45", "misc_image.h:462-473", ":474-479", "physmodel.h:164-181", "physmodel.h:58-64", "handtrack.h:769-780", "handtrack.h:703"):
        assert cite in header, cite
    for method in ("views_default", "fuse_views", "fuse_views_dev", "stage_view_rows", "fit_views", "fit_views_dev", "update_views_sync", "update_views_dev"):
        assert callable(getattr(native.Context, method)), method


def _call(L, ctx, what, **kw):
    """one of the calls on made-up host arrays with one argument changed -> (status, message)"""
    from hand_tracking_samples_amd import native
    a = dict(V=2, B=1, w=8, h=6, cap=64, opt=None, planes=None, points=None, passes=1, which=0)
    a.update(kw)
    V, B, w, hh = max(a["V"], 1), max(a["B"], 1), a["w"], a["h"]
    depth = np.zeros((B, V, hh, w), np.uint16); cams = np.zeros((B, V, 12), np.float32); cams[..., :5] = (8, 8, 4, 3, 0.001); cams[..., 11] = 1
    pts = np.zeros((B, a["cap"], 4), np.float32) if a["points"] is None else a["points"]
    before = pts.copy()
    n = np.zeros(B, np.int32); per = np.zeros((B, 2 * V), np.int32); org = np.zeros((B, 2 * V, 3), np.float32); cut = C.c_int(0); poses = np.zeros((B, 17, 7), np.float32)
    fp = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_float)); ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int)); u16 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint16))
    o = None if a["opt"] is None else C.byref(a["opt"])
    if what == "fuse":
        rc = L.ht_fuse_views(ctx, u16(depth), fp(cams), fp(a["planes"]), w, hh, a["V"], a["B"], o, fp(pts), a["cap"], ip(n), ip(per), fp(org), C.byref(cut))
    elif what == "fuse_dev":
        rc = L.ht_fuse_views_dev(ctx, depth.ctypes.data, cams.ctypes.data, None, w, hh, a["V"], a["B"], o, None, None, None, None, None)
    elif what == "update":
        rc = L.ht_update_views_sync(ctx, 64, u16(depth), fp(cams), fp(a["planes"]), w, hh, a["V"], 0.17, a["B"], o, a["passes"], fp(poses), None)
    elif what == "fit":
        rc = L.ht_fit_views(ctx, a["which"], a["B"], a["passes"], fp(poses))
    else:
        rows = np.zeros((B, 8, 16), np.float32)
        rc = L.ht_stage_view_rows(ctx, a["which"], a["B"], fp(rows), 8, ip(n))
    assert np.array_equal(pts.view(np.uint32), before.view(np.uint32)) and not n.any() and not per.any() and not org.any() and not poses.any() and cut.value == 0      # nothing was written
    return rc, (L.ht_last_error(ctx).decode() if ctx else "")


def test_refusals_need_no_device():
    """V outside 1..4, a bad range, fraction or eps, a plane with a non-finite or zero normal that is not the "none" plane, overlapping buffers and B beyond the batch are
    refused by name on a context whose ht_create failed (no model file, and on this machine no device); what passes those checks is refused as "not initialised"."""
    from hand_tracking_samples_amd import native
    L = native.load()
    h = C.c_void_p()
    assert L.ht_create(b"/nonexistent/model.htfx", 2, 0, C.byref(h)) != 0
    V = native.Views
    bad_planes = lambda *p: np.tile(np.array(p, np.float32), (1, 2, 1))
    try:
        for what in ("fuse", "fuse_dev"):
            for kw, text in ((dict(V=0), "between 1 and HT_VIEWS_MAX"), (dict(V=5), "between 1 and HT_VIEWS_MAX"), (dict(B=3), "batch"), (dict(B=0), "batch"),
                             (dict(opt=V(0.5, 0.5, 1, 0.02)), "bad range"), (dict(opt=V(-0.1, 0.5, 1, 0.02)), "bad range"), (dict(opt=V(0.1, float("nan"), 1, 0.02)), "bad range"),
                             (dict(opt=V(0.1, float("inf"), 1, 0.02)), "bad range"), (dict(opt=V(0.1, 0.65, 0, 0.02)), "bad fraction"), (dict(opt=V(0.1, 0.65, 1, -0.01)), "bad mirror_eps"),
                             (dict(opt=V(0.1, 0.65, 1, float("nan"))), "bad mirror_eps"), (dict(w=0), "w and h"), (dict(), "not initialised")):
                rc, msg = _call(L, h, what, **kw)
                assert rc != 0 and text in msg, (what, kw, msg)
        for planes, text in ((bad_planes(0, 0, 0, 0.5), "zero normal"), (bad_planes(0, float("nan"), 1, 0.5), "non-finite"), (bad_planes(0, 0, 1, float("inf")), "non-finite"),
                             (bad_planes(0, 0, 0, np.finfo(np.float32).max), "not initialised"), (bad_planes(0, 0, -1, 0.5), "not initialised")):
            rc, msg = _call(L, h, "fuse", planes=planes)
            assert rc != 0 and text in msg, (planes, msg)
        # an output that overlaps an input: the points handed in as the planes' memory
        shared = np.zeros((1, 64, 4), np.float32); shared[:, :2] = (0, 0, -1, 0.5)
        rc, msg = _call(L, h, "fuse", planes=shared[:, :2].reshape(1, 2, 4), points=shared)
        assert rc != 0 and "overlaps" in msg
        rc, msg = _call(L, h, "fuse", cap=0)
        assert rc != 0 and "cap" in msg
        # 4 views of 320x240 at fraction 1 could carry 307200 points a slot
        rc, msg = _call(L, h, "fuse_dev", V=4, w=320, h=240, opt=V(0.1, 0.65, 1, 0.02))
        assert rc != 0 and "307200 points" in msg
        for kw, text in ((dict(which=2), "which is 0"), (dict(passes=0), "passes"), (dict(passes=65), "passes"), (dict(B=3), "batch"), (dict(), "not initialised")):
            rc, msg = _call(L, h, "fit", **kw)
            assert rc != 0 and text in msg, (kw, msg)
        rc, msg = _call(L, h, "rows", which=-1)
        assert rc != 0 and "which is 0" in msg
        for kw in (dict(V=5), dict(B=3), dict(passes=0), dict(opt=V(0.1, 0.65, 0, 0.02)), dict()):
            assert _call(L, h, "update", **kw)[0] != 0
        for what in ("fuse", "fuse_dev", "update", "fit", "rows"):      # and without a context at all
            assert _call(L, None, what)[0] != 0
        o = V(9, 9, 9, 9)
        assert L.ht_views_default(None, C.byref(o)) != 0 and L.ht_views_default(h, None) != 0 and o.fraction == 9
        assert L.ht_views_default(h, C.byref(o)) == 0 and (o.range_lo, o.range_hi, o.fraction, o.mirror_eps) == (np.float32(0.1), np.float32(0.7), 4, np.float32(0.02))      # ht_create's parameters: drangey, subsample_fraction
    finally:
        L.ht_destroy(h)


def test_views_additions_of_the_cxx_header_compile_and_link(tmp_path):
    """include/ht_handtrack.hpp's FuseViews, update_views, ViewOptions and FusedCloud build with plain g++ against the C-ABI library"""
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "views")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_views_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "model_hand17.htfx"), "8", "8", "none.u16", "none.f32"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout      # they run on a tracker's device; no fallback
