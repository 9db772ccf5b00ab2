"""HandTracker::render_scene (include/ht_handtrack.hpp, an addition to the reference-named C++ surface) through tests/cxx_scene_example.cpp: it compiles and links with
plain g++; on the device three hands at 48x36 over a background equal the C call ht_raster_scene_depth, and both equal the host's definition."""
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL = os.path.join(HERE, "golden", "model_hand17.htfx")


def _build(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    lib = os.path.dirname(native.lib_path())
    exe = str(tmp_path / "scene_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cxx_scene_example.cpp"), "-o", exe, "-L" + lib, "-lht_mi355x", "-Wl,-rpath," + lib])
    return exe


def test_cxx_scene_example_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("with_bg", [0, 1])
def test_cxx_render_scene_equals_the_c_call(tmp_path, with_bg):
    from hand_tracking_samples_amd import native
    exe = _build(tmp_path)
    w, h, far, off, H = 48, 36, 0.85, 0.5, 3
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    poses = z["gtpose"][[11, 640, 300]].astype(np.float32)
    left = np.array([0, 1, 1, 0], np.uint8)
    cam = np.array([305 * w / 320.0, 305 * w / 320.0, w / 2.0 + 1.25, h / 2.0, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)
    bg = np.full((h, w), 420, np.uint16); bg[::3] = 0
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<5i2f", H, w, h, 17, with_bg, far, off)); f.write(cam.tobytes()); f.write(left.tobytes()); f.write(np.ascontiguousarray(poses).tobytes())
        if with_bg:
            f.write(bg.tobytes())
    out = subprocess.check_output([exe, MODEL, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=300).decode()
    assert "render_scene: 3 hands in %dx%d" % (w, h) in out
    raw = open(tmp_path / "out.bin", "rb").read()
    n = w * h; one = 4 * n + 4 * H
    assert len(raw) == 2 * one and raw[:one] == raw[one:]
    m = native.HostModel(MODEL)
    try:
        depth, hand, body, visible = m.raster_scene(poses, cam, w, h, left[:H], far, off, bg=bg if with_bg else None)
    finally:
        m.close()
    assert (hand == 0).any() and (hand > 0).any() and (not with_bg or (depth == 420).any())
    assert raw[:one] == depth.tobytes() + hand.tobytes() + body.tobytes() + visible.tobytes()
