"""HandTracker::EstimateHandSize (include/ht_handtrack.hpp) through a headless example (tests/cxx_size_example.cpp), the way tests/test_cxx_joints.py drives its
members: the C++ form on a tracker of one slot against ht_estimate_scale on a context of its own, bit for bit, and both against the Python binding."""
import os
import subprocess

import numpy as np
import pytest

import joints_inputs as ji

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "size_example")
    lib = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cxx_size_example.cpp"), "-o", exe, "-L" + lib, "-lht_mi355x", "-Wl,-rpath," + lib])
    return exe


def test_example_compiles_and_states_its_usage(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("free_pose", [1, 0])
def test_cxx_form_equals_the_c_call_and_the_binding(tmp_path, free_pose):
    from hand_tracking_samples_amd import native
    import test_gpu_size as tg
    name, B = "hand17", 3
    depth, cams, truth = tg.scene(name, B)
    exe = _build(tmp_path)
    files = {k: str(tmp_path / k) for k in ("frames.u16", "cams.f32", "poses.f32")}
    depth.tofile(files["frames.u16"]); cams.tofile(files["cams.f32"]); truth.tofile(files["poses.f32"])
    r = subprocess.run([exe, ji.model_path(name), str(tg.W), str(tg.H), files["frames.u16"], files["cams.f32"], files["poses.f32"], "4", "2", str(free_pose)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    assert lines[0] == "frames=3 rows=5 degenerate=0 equal=1"
    ctx = native.Context(ji.model_path(name), 1)
    try:
        s, T, st = ctx.estimate_scale(depth, cams, truth, 0, ctx.size_default(iterations=4, fraction=2, free_pose=free_pose))
    finally:
        ctx.close()
    assert np.float32(float.fromhex(lines[1].split()[1])) == s[0] and s[0] != np.float32(1.0)
    got = np.array([float.fromhex(x) for x in lines[2].split()[1:]], np.float32)
    assert np.array_equal(got.view(np.uint32), T[0].view(np.uint32))
    assert [float.fromhex(x) for x in lines[3].split()[1:]] == [st[0, 2], st[-1, 2]]
