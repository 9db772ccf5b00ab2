"""HandTracker::left_hand and PhysModel::Mirror of the C++ surface (include/ht_handtrack.hpp) through a headless driver (tests/cxx_hands_driver.cpp), the way
tests/test_cxx_joints.py drives the joint additions: two trackers on one golden full frame, one of them a left hand's, fed the flipped frame with the mirrored camera."""
import os
import struct
import subprocess

import numpy as np
import pytest

import htfx
import mirror_ref
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NB = 17


def _build(tmp_path):
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "hands_driver")
    lib = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cxx_hands_driver.cpp"), "-o", exe, "-L" + lib, "-lht_mi355x", "-Wl,-rpath," + lib])
    return exe


def test_driver_compiles_and_fails_loudly_without_a_device(tmp_path):
    import torch
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    if not torch.cuda.is_available():
        (tmp_path / "in.bin").write_bytes(struct.pack("<3i", 64, 64, NB))
        r = subprocess.run([exe, ol.MODEL, "none.cnnb", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout


class _Reader:
    def __init__(self, path):
        self.b = open(path, "rb").read(); self.at = 0

    def take(self, dtype, *shape):
        n = int(np.prod(shape)) * 4
        a = np.frombuffer(self.b, dtype, int(np.prod(shape)), self.at).reshape(shape); self.at += n
        return a

    def meshes(self):
        out = []
        for _ in range(NB):
            nv, nt = self.take(np.int32, 2)
            out.append(dict(pose=self.take(np.float32, 7), verts=self.take(np.float32, nv, 3), tris=self.take(np.int32, nt, 3)))
        return out


def _x_negated(v):
    return v * np.array([-1, 1, 1], np.float32)


def _is_mirror_mesh(left, right, pose_bytes=True):
    """the left mesh is the right one mirrored: the same triangles over x-negated corners, first corner kept and the other two swapped, at the mirrored pose
    (pose_bytes False: value for value -- a PositionUser computed from a mirrored pose, not mirrored after it was computed, may give +0.0 where the flip gives -0.0)"""
    for l, r in zip(left, right):
        assert l["verts"].shape == r["verts"].shape and l["tris"].shape == r["tris"].shape and len(r["tris"]) > 0
        assert l["verts"][l["tris"]].tobytes() == _x_negated(r["verts"])[r["tris"][:, [0, 2, 1]]].tobytes()
        want = mirror_ref.poses(r["pose"][None])[0]
        assert l["pose"].tobytes() == want.tobytes() if pose_bytes else np.array_equal(l["pose"], want)


@pytest.mark.gpu
def test_a_left_hand_tracker_is_the_mirror_image_of_a_right_hand_tracker(tmp_path, weights):
    from hand_tracking_samples_amd import weights as W
    exe = _build(tmp_path)
    G = htfx.load(os.path.join(HERE, "golden", "fullframe320.htfx"))
    depth = np.ascontiguousarray(G["f0/depth"], np.uint16); cam = G["f0/cam"].astype(np.float32); start = G["f0/startpose"].astype(np.float32)
    h, w = depth.shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3i", w, h, NB))
        f.write(depth.tobytes()); f.write(cam.tobytes()); f.write(start.tobytes())
        f.write(mirror_ref.frames(depth[None])[0].tobytes()); f.write(mirror_ref.cams(cam[None], w)[0].tobytes()); f.write(mirror_ref.poses(start[None])[0].tobytes())
    cnnb = str(tmp_path / "w.cnnb")
    W.save_cnnb(cnnb, weights)
    r = subprocess.run([exe, ol.MODEL, cnnb, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "hands: 320 x 240, 17 bones, cnn_input 64 x 64" in r.stdout
    rd = _Reader(tmp_path / "out.bin")
    side = []
    for _ in range(2):
        side.append(dict(update=rd.take(np.float32, NB, 7), pose=rd.take(np.float32, NB, 7), user=rd.take(np.float32, NB, 7), hulls=rd.meshes(), sd=rd.meshes()))
    right, left = side
    assert np.isfinite(right["update"]).all() and right["update"].tobytes() != start.tobytes()      # the tracker moved
    for k in ("update", "pose", "user"):
        assert left[k].tobytes() == mirror_ref.poses(right[k][None])[0].tobytes(), k
    # GetMeshes: the left tracker's hull vertices are the other's x-negated with each triangle's last two indices swapped, at the mirrored poses
    for l, r in zip(left["hulls"], right["hulls"]):
        assert l["verts"].tobytes() == _x_negated(r["verts"]).tobytes() and np.array_equal(l["tris"], r["tris"][:, [0, 2, 1]])
    _is_mirror_mesh(left["hulls"], right["hulls"]); _is_mirror_mesh(left["sd"], right["sd"])
    for b in range(NB):
        assert left["hulls"][b]["pose"].tobytes() == left["pose"][b].tobytes() and left["sd"][b]["pose"].tobytes() == left["user"][b].tobytes()
    # PhysModel::Mirror on the untracked model: the same meshes, and twice is the identity (poses: the rest poses, mirrored with the model)
    fake = [dict(hulls=rd.meshes(), sd=rd.meshes()) for _ in range(3)]
    assert rd.at == len(rd.b)
    _is_mirror_mesh(fake[1]["hulls"], fake[0]["hulls"]); _is_mirror_mesh(fake[1]["sd"], fake[0]["sd"], pose_bytes=False)
    for kind in ("hulls", "sd"):
        for a, b in zip(fake[0][kind], fake[2][kind]):
            assert all(a[k].tobytes() == b[k].tobytes() for k in ("verts", "tris")) and np.array_equal(a["pose"], b["pose"])
