"""HandTracker::render_depth (include/ht_handtrack.hpp, an addition to the reference-named C++ surface) through tests/cxx_render_driver.cpp: the ground-truth
poses of tests/golden/fullframe320.htfx rendered on the device equal the frames the reference's application rendered, bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import htfx
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.gpu
def test_cxx_render_depth_equals_the_references_frames(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    lib = os.path.dirname(native.lib_path())
    exe = str(tmp_path / "render_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cxx_render_driver.cpp"), "-o", exe, "-L" + lib, "-lht_mi355x", "-Wl,-rpath," + lib])
    G = htfx.load(os.path.join(HERE, "golden", "fullframe320.htfx"))
    n = len(G["rows"])
    w, h = (int(x) for x in G["dims"])
    depth = np.stack([G["f%d/depth" % f] for f in range(n)])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", n, w, h, 17))
        for k in range(n):
            f.write(np.ascontiguousarray(depth[k], np.uint16).tobytes()); f.write(np.ascontiguousarray(G["f%d/cam" % k], np.float32).tobytes())
            f.write(np.ascontiguousarray(G["f%d/startpose" % k], np.float32).tobytes()); f.write(np.ascontiguousarray(G["f%d/gtpose" % k], np.float32).tobytes())
    assert all(np.array_equal(G["f%d/cam" % k], G["f0/cam"]) for k in range(n))      # one camera for the batch
    out = subprocess.check_output([exe, ol.MODEL, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=300).decode()
    assert "render_depth: %d frames of %dx%d" % (n, w, h) in out
    got = np.fromfile(tmp_path / "out.bin", np.uint16).reshape(depth.shape)
    assert np.array_equal(got, depth)
