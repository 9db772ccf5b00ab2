"""The joint-coordinate additions of the C++ surface (HandTracker::handmodel.GetJointCoords / JointAngles / GetJointGaps / SetJointCoords, include/ht_handtrack.hpp)
through a headless driver (tests/cxx_joints_driver.cpp), the way tests/test_cxx_driver.py drives the reference-named members."""
import os
import struct
import subprocess

import numpy as np
import pytest

import joints_inputs as ji
import joints_ref as jr
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "joints_driver")
    lib = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cxx_joints_driver.cpp"), "-o", exe, "-L" + lib, "-lht_mi355x", "-Wl,-rpath," + lib])
    return exe


def test_driver_compiles_and_fails_loudly_without_a_device(tmp_path):
    import torch
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    if not torch.cuda.is_available():
        (tmp_path / "in.bin").write_bytes(struct.pack("<4i", 0, 64, 64, 17))
        r = subprocess.run([exe, ol.MODEL, "none.cnnb", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_set_joint_coords_of_get_joint_coords_reproduces_the_tracked_hand(tmp_path, golden, weights):
    """A tracked hand read out and rebuilt from its own coordinates: the coordinates come back within tol_c, every orientation within 2 tol_c per joint of its
    chain (depth <= 4: 8 tol_c, either quaternion sign), every position within that rotation's reach (< 1 m) plus the gaps the rebuild closes, and the joints
    end closed to the forward kinematics' own rounding."""
    from hand_tracking_samples_amd import weights as W
    exe = _build(tmp_path)
    nf, nb, nj, tol = 4, 17, 16, ji.tol_c()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", nf, 64, 64, nb))
        for k in range(nf):
            f.write(np.ascontiguousarray(golden["f%d/depth" % k], np.uint16).tobytes()); f.write(np.ascontiguousarray(golden["f%d/cam" % k], np.float32).tobytes())
            f.write(np.ascontiguousarray(golden["f%d/startpose" % k], np.float32).tobytes()); f.write(np.ascontiguousarray(golden["f%d/gtpose" % k], np.float32).tobytes())
    cnnb = str(tmp_path / "w.cnnb")
    W.save_cnnb(cnnb, weights)
    r = subprocess.run([exe, ol.MODEL, cnnb, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "joints: 4 frames, 17 bones, 16 joints" in r.stdout
    rec = np.fromfile(tmp_path / "out.bin", np.float32).reshape(nf, -1)
    cuts = np.cumsum([nb * 7, nj * 3, nj * 3, nj, nb * 7, nj * 3, nj])
    assert rec.shape[1] == cuts[-1]
    m = ji.model("hand17")
    A = float(max(np.linalg.norm(m.p0, axis=1).max(), np.linalg.norm(m.p1, axis=1).max(), np.linalg.norm(m.com, axis=1).max(),
                  np.linalg.norm(m.p0 - m.com[m.rb0], axis=1).max(), np.linalg.norm(m.p1 - m.com[m.rb1], axis=1).max()))
    for k in range(nf):
        before, c, deg, gaps, after, c2, gaps2 = np.split(rec[k], cuts[:-1])
        before, after, c, c2, deg = before.reshape(nb, 7), after.reshape(nb, 7), c.reshape(nj, 3), c2.reshape(nj, 3), deg.reshape(nj, 3)
        want_c, want_g = jr.coords(m, before[None], np.float32, com_poses=True)
        assert np.array_equal(c, want_c[0]) and np.array_equal(gaps, want_g[0])
        assert np.allclose(deg, 2 * np.arcsin(c.astype(np.float64)) * 180 / 3.14, rtol=1e-5, atol=1e-4)
        assert np.array_equal(after[0], before[0])      # body 0 stays where it is
        dq = np.minimum(np.abs(after[:, 3:] - before[:, 3:]).max(axis=1), np.abs(after[:, 3:] + before[:, 3:]).max(axis=1)).max()
        dp = np.abs(after[:, :3] - before[:, :3]).max()
        print("frame %d: |dc| %.2e, |dq| %.2e, |dp| %.2e with %.2e of gaps closed, gaps left %.2e" % (k, np.abs(c2 - c).max(), dq, dp, gaps.sum(), gaps2.max()))
        assert np.abs(c2 - c).max() <= tol and dq <= 8 * tol and dp <= 8 * tol + gaps.sum()
        assert gaps2.max() <= np.sqrt(3.0) * 2.0 ** -24 * (8 * float(np.abs(after[:, :3]).max()) + 48 * A)      # tests/test_joints_ref.py: K_POS, K_ROT
