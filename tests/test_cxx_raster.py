"""HandTracker::render_mesh_raster (include/ht_handtrack.hpp, an addition to the reference-named C++ surface) through tests/cxx_raster_example.cpp: two poses at
48x36 equal the C call ht_raster_mesh_depth, and both equal the host's definition."""
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL = os.path.join(HERE, "golden", "model_hand17.htfx")


@pytest.mark.gpu
def test_cxx_render_mesh_raster_equals_the_c_call(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    lib = os.path.dirname(native.lib_path())
    exe = str(tmp_path / "raster_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cxx_raster_example.cpp"), "-o", exe, "-L" + lib, "-lht_mi355x", "-Wl,-rpath," + lib])
    w, h, far, off = 48, 36, 0.85, 0.5
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    poses = z["gtpose"][[11, 640]].astype(np.float32)
    cam = np.array([305 * w / 320.0, 305 * w / 320.0, w / 2.0, h / 2.0, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i2f", 2, w, h, 17, far, off)); f.write(cam.tobytes()); f.write(np.ascontiguousarray(poses).tobytes())
    out = subprocess.check_output([exe, MODEL, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=300).decode()
    assert "render_mesh_raster: 2 frames of %dx%d" % (w, h) in out
    got = np.fromfile(tmp_path / "out.bin", np.uint16).reshape(2, 2, h, w)
    assert np.array_equal(got[0], got[1])
    m = native.HostModel(MODEL)
    try:
        want = np.stack([m.raster_mesh(p, cam, w, h, far, off)[0] for p in poses])
    finally:
        m.close()
    assert (want < 850).sum() > 40 and np.array_equal(got[0], want)
