"""CPU-only checks of the hand-size calls (include/ht_mi355x.h "the hand's size"): declared, exported and bound with the documented signatures, ht_size_default fills the
documented defaults, and every refusal that needs no device is made without one and before anything grows or runs: a context that never came up names the argument it
refuses before it reports itself.  The host-only part of the calls runs clean under the address and undefined-behaviour sanitizers in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "ht_size_default": "ht_ctx *ctx, ht_size *o",
    "ht_estimate_scale": "ht_ctx *ctx, int which, const float *poses, const uint16_t *depth, const float *cams, int w, int h, int B, const ht_size *o, float *scale_out, float *T_out, double *stats",
    "ht_estimate_scale_dev": "ht_ctx *ctx, int which, const float *d_poses, const uint16_t *d_depth, const float *d_cams, int w, int h, int B, const ht_size *o, float *d_scale_out, float *d_T_out, double *d_stats,\n"
                             "                          void *stream",
}
FIELDS = ["range_lo", "range_hi", "fraction", "mode", "free_pose", "iterations", "max_dist", "damping", "min_points", "scale0", "scale_lo", "scale_hi"]


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
    assert "typedef struct { float range_lo, range_hi; int fraction, mode, free_pose, iterations; float max_dist, damping; int min_points; float scale0, scale_lo, scale_hi; } ht_size;" in header
    assert [f[0] for f in native.Size._fields_] == FIELDS and C.sizeof(native.Size) == 12 * 4
    for define, value in (("HT_SIZE_SHARED", native.SIZE_SHARED), ("HT_SIZE_PER_SLOT", native.SIZE_PER_SLOT), ("HT_SIZE_STATS", native.SIZE_STATS), ("HT_SIZE_SLOT_STATS", native.SIZE_SLOT_STATS),
                          ("HT_SIZE_FEW_INLIERS", native.SIZE_FEW_INLIERS), ("HT_SIZE_BAD_PIVOT", native.SIZE_BAD_PIVOT), ("HT_SIZE_CLAMPED", native.SIZE_CLAMPED)):
        assert "#define %s %d\n" % (define, value) in header
    assert "#define HT_SIZE_ROW(N, B) ((N) * HT_SIZE_STATS + (B) * HT_SIZE_SLOT_STATS)\n" in header and native.size_row(2, 5) == 2 * 6 + 5 * 3
    text = header.split("the hand's size from tracked frames")[1].split("#define HT_SIZE_SHARED")[0]
    for cite in ("physmodel.h:196-219", ":304-319", "openvr-demo.cpp:109", "realtime-annotator.cpp:238", "Out of scope: left hands"):
        assert cite in text, cite
    for method in ("size_default", "estimate_scale", "estimate_scale_dev"):
        assert callable(getattr(native.Context, method)), method


def _call(L, ctx, dev=False, **kw):
    """one of the two calls on made-up host arrays with one argument changed -> (status, message); nothing may have been written"""
    a = dict(which=0, B=1, w=8, h=6, opt=None, poses=False, depth=True, cams=True, scale=True, T=True, stats=True)
    a.update(kw)
    B, w, hh = max(a["B"], 1), max(a["w"], 1), max(a["h"], 1)
    depth = np.zeros((B, hh, w), np.uint16); cams = np.zeros((B, 12), np.float32); cams[:, :5] = (8, 8, 4, 3, 0.001); cams[:, 11] = 1
    poses = np.zeros((B, 17, 7), np.float32); sc = np.zeros(B, np.float32); T = np.zeros((B, 7), np.float32); stats = np.zeros((65, 9 * B), np.float64)
    o = None if a["opt"] is None else C.byref(a["opt"])
    if dev:
        rc = L.ht_estimate_scale_dev(ctx, a["which"], poses.ctypes.data if a["poses"] else None, depth.ctypes.data if a["depth"] else None, cams.ctypes.data if a["cams"] else None, a["w"], a["h"], a["B"], o,
                                     sc.ctypes.data if a["scale"] else None, T.ctypes.data if a["T"] else None, stats.ctypes.data if a["stats"] else None, None)
    else:
        fp = lambda x, on: x.ctypes.data_as(C.POINTER(C.c_float)) if on else None      # noqa: E731
        rc = L.ht_estimate_scale(ctx, a["which"], fp(poses, a["poses"]), depth.ctypes.data_as(C.POINTER(C.c_uint16)) if a["depth"] else None, fp(cams, a["cams"]), a["w"], a["h"], a["B"], o, fp(sc, a["scale"]),
                                 fp(T, a["T"]), stats.ctypes.data_as(C.POINTER(C.c_double)) if a["stats"] else None)
    assert not T.any() and not stats.any() and not sc.any()
    return rc, (L.ht_last_error(ctx).decode() if ctx else "")


def test_defaults_and_refusals_need_no_device():
    from hand_tracking_samples_amd import native
    L = native.load()
    h = C.c_void_p()
    assert L.ht_create(b"/nonexistent/model.htfx", 2, 0, C.byref(h)) != 0
    try:
        o = native.Size(*([9] * 12))
        assert L.ht_size_default(None, C.byref(o)) != 0 and L.ht_size_default(h, None) != 0 and o.fraction == 9
        assert L.ht_size_default(h, C.byref(o)) == 0
        c = native.Calib(); assert L.ht_calib_default(h, C.byref(c)) == 0
        assert (o.range_lo, o.range_hi, o.fraction, o.max_dist, o.damping, o.min_points) == (c.range_lo, c.range_hi, c.fraction, c.max_dist, c.damping, c.min_points)
        assert (o.mode, o.free_pose, o.iterations, o.scale0, o.scale_lo, o.scale_hi) == (native.SIZE_SHARED, 1, 10, 1.0, 0.5, 2.0)

        def but(**kw):
            n = native.Size.from_buffer_copy(o)
            for k, v in kw.items():
                setattr(n, k, v)
            return n
        nan, inf = float("nan"), float("inf")
        for dev in (False, True):
            for kw, text in ((dict(B=0), "batch"), (dict(B=3), "batch"), (dict(B=-1, poses=True), "batch"), (dict(B=65536, poses=True), "batch"), (dict(w=0), "w and h"), (dict(h=4097), "w and h"),
                             (dict(depth=False), "frames"), (dict(cams=False), "cameras"), (dict(scale=False), "scale_out"), (dict(T=False), "T_out"), (dict(stats=False), "stats"), (dict(which=2), "which is 0"),
                             (dict(which=-1), "which is 0"), (dict(opt=but(fraction=0)), "bad fraction"), (dict(opt=but(range_lo=0.7)), "bad range"), (dict(opt=but(range_lo=-0.1)), "bad range"),
                             (dict(opt=but(range_hi=nan)), "bad range"), (dict(opt=but(range_hi=inf)), "bad range"), (dict(opt=but(mode=2)), "bad mode"), (dict(opt=but(mode=-1)), "bad mode"),
                             (dict(opt=but(free_pose=2)), "bad free_pose"), (dict(opt=but(free_pose=-1)), "bad free_pose"), (dict(opt=but(iterations=-1)), "bad iterations"),
                             (dict(opt=but(iterations=65)), "bad iterations"), (dict(opt=but(max_dist=0.0)), "bad max_dist"), (dict(opt=but(max_dist=nan)), "bad max_dist"), (dict(opt=but(max_dist=inf)), "bad max_dist"),
                             (dict(opt=but(damping=-1e-3)), "bad damping"), (dict(opt=but(damping=nan)), "bad damping"), (dict(opt=but(min_points=-1)), "bad min_points"),
                             (dict(opt=but(scale0=nan)), "bad scale0"), (dict(opt=but(scale0=inf)), "bad scale0"), (dict(opt=but(scale_lo=nan)), "bad scale0"), (dict(opt=but(scale_hi=inf)), "bad scale0"),
                             (dict(opt=but(scale_lo=0.0)), "bad scale0"), (dict(opt=but(scale_lo=-0.5)), "bad scale0"), (dict(opt=but(scale0=0.4)), "bad scale0"), (dict(opt=but(scale0=2.1)), "bad scale0"),
                             (dict(opt=but(scale_lo=1.5, scale0=1.6, scale_hi=1.4)), "bad scale0"),
                             (dict(w=640, h=480, opt=but(fraction=1)), "307200 points"), (dict(), "not initialised"), (dict(poses=True, B=2), "not initialised"),
                             (dict(opt=but(iterations=0, mode=native.SIZE_PER_SLOT, free_pose=0, scale0=0.5, scale_lo=0.5)), "not initialised")):
                rc, msg = _call(L, h, dev, **kw)
                assert rc != 0 and text in msg, (dev, kw, msg)
            assert _call(L, None, dev)[0] != 0      # and without a context at all
        # the device form takes outputs that are 4-byte aligned
        T = np.zeros(16, np.float32)
        for off in ((2, 0, 0), (0, 2, 0), (0, 0, 2)):
            rc = L.ht_estimate_scale_dev(h, 0, None, T.ctypes.data, T.ctypes.data, 8, 6, 1, None, T.ctypes.data + off[0], T.ctypes.data + off[1], T.ctypes.data + off[2], None)
            assert rc != 0 and "4-byte aligned" in L.ht_last_error(h).decode() and not T.any()
        # an output of the host form that overlaps an input
        cams = np.zeros((1, 12), np.float32); depth = np.zeros((1, 6, 8), np.uint16); stats = np.zeros((11, 9), np.float64); sc = np.zeros(1, np.float32)
        rc = L.ht_estimate_scale(h, 0, None, depth.ctypes.data_as(C.POINTER(C.c_uint16)), cams.ctypes.data_as(C.POINTER(C.c_float)), 8, 6, 1, None, sc.ctypes.data_as(C.POINTER(C.c_float)),
                                 cams[:, 5:].ctypes.data_as(C.POINTER(C.c_float)), stats.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc != 0 and "overlaps" in L.ht_last_error(h).decode()
    finally:
        L.ht_destroy(h)


def test_host_side_is_clean_under_the_sanitizers(tmp_path):
    """tests/hip_size_host_check.hip: a program with its own main that compiles csrc/ht_size.hip's host code with -fsanitize=address,undefined and drives the argument
    checks and the host form's staging plan on a context that never came up (everything else from the library as it is built)"""
    from hand_tracking_samples_amd import build, native
    native.load()
    exe = str(tmp_path / "size_host_check")
    libdir = os.path.dirname(native.lib_path())
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer"]
    subprocess.check_call([build.HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable"] + san +
                          [os.path.join(ROOT, "tests", "hip_size_host_check.hip"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    # where a device exists ht_create asks the HIP runtime for it, and the runtime keeps a few allocations of its own to the end of the process: those, by their library,
    # are not this project's leaks; everything else still is
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:libhsa-runtime64.so\nleak:libamdhip64.so\n")
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
                                                                         LSAN_OPTIONS="suppressions=%s:print_suppressions=0" % supp))
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "size host checks: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
