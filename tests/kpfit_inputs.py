"""Inputs shared by tests/test_kpfit_ref.py, tests/test_gpu_kpfit.py and tools/eval_keypoint_fit.py: start states and keypoint targets made from the bench's ground truths
(a frame's targets are its own ground truth's keypoints; the start is another frame's ground truth), cameras, weights.  Test infrastructure only."""
import functools
import os

import numpy as np

import joints_inputs as ji
import quality_ref as Q

ROOT = ji.ROOT


@functools.lru_cache(None)
def truths(name):
    """centre-of-mass poses [n,nb,7] of the model's bench frames"""
    if name == "hand17":
        return np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))["gtpose"].astype(np.float32)
    return np.load(os.path.join(ROOT, "bench_data", "frames5_256.npz"))["startpose"].astype(np.float32)


def states_of(poses):
    """centre-of-mass poses [B,nb,7] -> solver states [B,nb,13] at rest"""
    s = np.zeros(poses.shape[:2] + (13,), np.float32)
    s[:, :, :7] = poses
    return s


def camera(B, away=False, seed=5):
    """cameras [B,12] of a 64x64 tile; away: each with a pose of its own, centimetres off the origin and a few degrees round"""
    cams = np.zeros((B, 12), np.float32)
    cams[:, 0] = cams[:, 1] = 60.0; cams[:, 2] = cams[:, 3] = 31.5; cams[:, 4] = 0.001; cams[:, 11] = 1.0
    if away:
        rng = np.random.default_rng(seed)
        q = np.array([0, 0, 0, 1.0]) + rng.standard_normal((B, 4)) * 0.05
        cams[:, 8:12] = q / np.linalg.norm(q, axis=1, keepdims=True); cams[:, 5:8] = rng.uniform(-0.05, 0.05, (B, 3))
    return cams


def table_of(name, which):
    m = ji.model(name)
    return Q.feature8() if which == "feature8" else Q.skeleton(m)


def scene(name, B, table, lag=1, first=0, away=False):
    """dict(model, state [B,nb,13] = the ground truth of frame first + i + lag at rest, xyz [B,K,3] and pix [B,K,2] = the keypoints of frame first + i's ground truth, cams)"""
    m, P = ji.model(name), truths(name)
    idx = first + np.arange(B)
    cams = camera(B, away)
    kp = Q.keypoints(m, P[idx % len(P)], table, np.float32, com_poses=True, cams=cams)
    return dict(model=m, state=states_of(P[(idx + lag) % len(P)]), xyz=kp["xyz"], pix=kp["pix"], cams=cams, truth=P[idx % len(P)])


def mixed_kind(K):
    """every third keypoint a pixel target"""
    return (np.arange(K) % 3 == 1).astype(np.int32)


def ragged_weights(B, K, seed=3):
    """weights in (0, 1] with frame i's first 2 i keypoints absent (weight 0) and the last frame without any, so that every frame has another row count"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 1.0, (B, K)).astype(np.float32)
    for i in range(B):
        w[i, :min(K, 2 * i)] = 0
    if B > 1:
        w[B - 1] = 0
    return w
