"""CPU-only checks of the training-sample entry points (ht_expected_cnn_batch / _dev, ht_cnn_input_dev, ht_cnn_train_dev, include/ht_mi355x.h): they
are exported and declared, bad arguments are refused before any device work, and the numpy restatement of train-cnn's compress (tests/pose_frame.py)
that is the oracle of HT_LABELS_SEGMENT_FRAME behaves as the pose algebra it restates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import pose_frame as pf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("ht_expected_cnn_batch", "ht_expected_cnn_dev", "ht_cnn_input_dev", "ht_cnn_train_dev")


def test_label_and_pool_symbols_exported_and_declared():
    from hand_tracking_samples_amd import native
    L = native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    header = open(os.path.join(ROOT, "include", "ht_mi355x.h")).read()
    for s in NEW:
        assert s in native.SYMBOLS and s in exported and hasattr(L, s)
        assert re.search(r"\bint %s\(" % s, header)
    assert re.search(r"#define HT_LABELS_SEGMENT_FRAME 1\b", header) and native.LABELS_SEGMENT_FRAME == 1


def test_label_and_pool_calls_refuse_null_contexts_and_bad_arguments():
    from hand_tracking_samples_amd import native
    L = native.load()
    poses = np.zeros((1, 17, 7), np.float32); cams = np.zeros((1, 12), np.float32); out = np.zeros((1, 2304), np.float32)
    tiles = np.zeros((2, 4096), np.uint16); cnn_in = np.zeros((1, 4096), np.float32); order = np.zeros(1, np.int32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = order.ctypes.data_as(C.POINTER(C.c_int))
    misaligned = tiles.ctypes.data + 2
    # a NULL context is refused whatever else is given
    assert L.ht_expected_cnn_batch(None, fp(poses), fp(cams), 1, 0, fp(out), None, None) != 0
    assert L.ht_expected_cnn_dev(None, poses.ctypes.data, cams.ctypes.data, 1, 0, out.ctypes.data, None, None, None) != 0
    assert L.ht_cnn_input_dev(None, tiles.ctypes.data, cams.ctypes.data, 1, cnn_in.ctypes.data, None) != 0
    assert L.ht_cnn_train_dev(None, cnn_in.ctypes.data, out.ctypes.data, 1, ip, 1, 0.001, None, None) != 0
    # a context that never came up (no device here, or a missing model) is refused as well: the calls below must fail, not crash
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    try:
        for args in ((None, fp(cams), 1, 0, fp(out)), (fp(poses), None, 1, 0, fp(out)), (fp(poses), fp(cams), 1, 0, None), (fp(poses), fp(cams), -1, 0, fp(out)),
                     (fp(poses), fp(cams), 1, 2, fp(out))):
            assert L.ht_expected_cnn_batch(h, *args, None, None) != 0
            dev = [a if not hasattr(a, "contents") else C.cast(a, C.c_void_p) for a in args]
            assert L.ht_expected_cnn_dev(h, *dev, None, None, None) != 0
        for args in ((None, cams.ctypes.data, 1, cnn_in.ctypes.data), (tiles.ctypes.data, None, 1, cnn_in.ctypes.data), (tiles.ctypes.data, cams.ctypes.data, 1, None),
                     (tiles.ctypes.data, cams.ctypes.data, -1, cnn_in.ctypes.data), (misaligned, cams.ctypes.data, 1, cnn_in.ctypes.data)):
            assert L.ht_cnn_input_dev(h, *args, None) != 0
        bad = np.array([0, 5], np.int32)
        for args in ((None, out.ctypes.data, 1, ip, 1), (cnn_in.ctypes.data, None, 1, ip, 1), (cnn_in.ctypes.data, out.ctypes.data, 0, ip, 1),
                     (cnn_in.ctypes.data, out.ctypes.data, 1, ip, -1), (cnn_in.ctypes.data, out.ctypes.data, 1, None, 2),
                     (cnn_in.ctypes.data, out.ctypes.data, 1, bad.ctypes.data_as(C.POINTER(C.c_int)), 2)):
            assert L.ht_cnn_train_dev(h, *args, 0.001, None, None) != 0
    finally:
        if h:
            L.ht_destroy(h)


def _unit(q):
    q = np.asarray(q, np.float64)
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)


def test_compress_restatement_inverts_and_composes():
    rng = np.random.default_rng(7)
    a = np.concatenate([rng.uniform(-1, 1, (64, 3)), _unit(rng.normal(size=(64, 4)))], -1).astype(np.float32)
    b = np.concatenate([rng.uniform(-1, 1, (64, 3)), _unit(rng.normal(size=(64, 4)))], -1).astype(np.float32)
    ident = pf.mul(pf.inverse(a), a)
    assert np.abs(ident[:, :3]).max() < 1e-5 and np.abs(np.abs(ident[:, 6]) - 1).max() < 1e-5
    # the identity pose changes no bit of a pose it multiplies (the segment-frame camera)
    one = np.tile(np.array([0, 0, 0, 0, 0, 0, 1], np.float32), (64, 1))
    assert np.array_equal(pf.mul(one, b), b)
    ab = pf.mul(a, b)
    assert np.allclose(pf.mul(pf.inverse(a), ab), b, atol=1e-5)


def test_compressed_labels_see_the_hand_where_the_camera_did():
    """the host labels of the compressed frames (identity camera) and of the raw frames (camera posed) agree to rounding: the restatement is the
    frame change the camera applies (bench ground truths, their cameras with a rotated and shifted pose)"""
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    rng = np.random.default_rng(3)
    idx = rng.choice(len(z["gtpose"]), 64, replace=False)
    poses = z["gtpose"][idx].copy(); cams = z["cam"][idx].copy()
    cams[:, 5:8] = rng.uniform(-0.05, 0.05, (64, 3)); cams[:, 8:12] = _unit(np.concatenate([rng.normal(0, 0.05, (64, 3)), np.ones((64, 1))], -1))
    # move the hand with the camera so that it stays in view
    poses = pf.mul(np.broadcast_to(cams[:, None, 5:12], poses.shape), poses)
    e0, ip0, v0 = pf.host_labels(poses, cams)
    pc, cc = pf.compress(poses, cams)
    e1, ip1, v1 = pf.host_labels(pc, cc)
    assert np.abs(ip0 - ip1).max() < 1e-3 and np.abs(v0 - v1).max() < 1e-4
    assert (np.abs(e0 - e1) > 0).mean() < 0.01
