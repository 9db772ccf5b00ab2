"""CPU-only checks of the device renderer's C-ABI (ht_render_depth / ht_render_depth_dev, include/ht_mi355x.h): both are exported and
bad arguments are refused before any device work."""
import ctypes as C
import subprocess

import numpy as np


def test_render_symbols_exported():
    from hand_tracking_samples_amd import native
    L = native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    for s in ("ht_render_depth", "ht_render_depth_dev"):
        assert s in native.SYMBOLS and s in exported and hasattr(L, s)


def test_render_rejects_null_context_and_bad_arguments():
    from hand_tracking_samples_amd import native
    L = native.load()
    poses = np.zeros((1, 17, 7), np.float32); cams = np.zeros((1, 12), np.float32); depth = np.zeros((1, 8, 8), np.uint16)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dp = depth.ctypes.data_as(C.POINTER(C.c_uint16))
    # a NULL context is refused by both, whatever else is given
    assert L.ht_render_depth(None, fp(poses), fp(cams), 8, 8, 4.0, 1, dp, None) != 0
    assert L.ht_render_depth_dev(None, poses.ctypes.data, cams.ctypes.data, 8, 8, 4.0, 1, depth.ctypes.data, None, None) != 0
    assert L.ht_render_depth(None, fp(poses), fp(cams), 8, 8, 4.0, 0, dp, None) != 0
    # a context that never came up (no device here, or a missing model) is refused as well: the calls below must fail, not crash
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    try:
        for args in ((None, fp(cams), 8, 8, 4.0, 1, dp), (fp(poses), None, 8, 8, 4.0, 1, dp), (fp(poses), fp(cams), 8, 8, 4.0, 1, None),
                     (fp(poses), fp(cams), 0, 8, 4.0, 1, dp), (fp(poses), fp(cams), 8, 0, 4.0, 1, dp), (fp(poses), fp(cams), 4097, 8, 4.0, 1, dp),
                     (fp(poses), fp(cams), 8, 4097, 4.0, 1, dp), (fp(poses), fp(cams), 8, 8, 0.0, 1, dp), (fp(poses), fp(cams), 8, 8, -1.0, 1, dp)):
            assert L.ht_render_depth(h, *args, None) != 0
            dev = [a if not hasattr(a, "contents") else C.cast(a, C.c_void_p) for a in args]
            assert L.ht_render_depth_dev(h, *dev, None, None) != 0
    finally:
        if h:
            L.ht_destroy(h)
