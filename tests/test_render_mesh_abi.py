"""CPU-only checks of the mesh ray cast (ht_model_hitcheck_mesh / ht_model_render_mesh, the definition ht_render_mesh_depth is held to; include/ht_mi355x.h):
the mesh table, an independent numpy float32 restatement (tests/mesh_ray.py) bit for bit, the same definition evaluated in float64 as the geometric
yardstick, consistency with the bodies' bounds and the background, and the device entry points' refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_ray

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODELS = {17: os.path.join(HERE, "golden", "model_hand17.htfx"), 26: os.path.join(HERE, "golden", "model_hand26.htfx")}
W, H = 24, 18
CAM = np.array([305 * W / 320.0, 305 * W / 320.0, 160 * W / 320.0, 120 * W / 320.0, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)      # the application's camera scaled by 24/320
OFFSETS = ((0.0, 4.0), (0.5, 0.85))
# Share of pixels whose float32 winner differs from the float64 winner (rays within rounding of an edge or silhouette), measured on the 24 frames below:
# 0 of 10368 pixels.  The bound is twice the measured share.
MEASURED_WINNER_SHARE = 0.0


def _poses(nb):
    """six seeded ground truths of the bench recording; the 26-bone hand takes the poses of the reference's 26-bone frames, moved to the recorded palms"""
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    rng = np.random.default_rng(19)
    out = z["gtpose"][rng.choice(len(z["gtpose"]), 6, replace=False)].astype(np.float32)
    if nb == out.shape[1]:
        return out
    import htfx
    G = htfx.load(os.path.join(HERE, "golden", "fullframe5.htfx"))      # the reference's own 26-bone poses, brought to the recorded hands' places
    own = np.stack([G["f%d/gtpose" % (i % len(G["rows"]))] for i in range(len(out))]).astype(np.float32)
    own[:, :, :3] += out[:, :1, :3] - own[:, :1, :3]
    return own


@pytest.fixture(scope="module", params=[17, 26])
def frames(request):
    """host frames, the numpy float32 restatement and the float64 evaluation of the same poses: computed once, shared and left unchanged"""
    from hand_tracking_samples_amd import native
    nb = request.param
    m = native.HostModel(MODELS[nb])
    corners = [m.sdmesh(b).reshape(-1, 3, 3) for b in range(nb)]
    com = np.stack([m.com(b) for b in range(nb)])
    m32, m64 = mesh_ray.Mesh(corners, com, np.float32), mesh_ray.Mesh(corners, com, np.float64)
    poses = _poses(nb)
    rec = []
    for p in poses:
        for off, far in OFFSETS:
            rec.append(dict(pose=p, off=off, far=far, host=m.render_mesh(p, CAM, W, H, far, off), f32=mesh_ray.render(m32, p, CAM, W, H, far, off), f64=mesh_ray.render(m64, p, CAM, W, H, far, off)))
    yield dict(nb=nb, model=m, corners=corners, com=com, rec=rec)
    m.close()


def test_mesh_table_counts():
    from hand_tracking_samples_amd import native
    m = native.HostModel(MODELS[17])
    try:
        counts = [len(m.sdmesh(b)) // 3 for b in range(m.nb)]
    finally:
        m.close()
    assert counts == [512] * 3 + [320] * 14 and sum(counts) == 6016


def test_host_equals_the_numpy_restatement_bit_for_bit(frames):
    m = frames["model"]
    rng = np.random.default_rng(5)
    hand = 0
    for r in frames["rec"]:
        depth, body = r["host"]
        d32, b32, t32, _ = r["f32"]
        assert np.array_equal(depth, d32)
        assert np.array_equal(body, b32)
        hand += int((body >= 0).sum())
        # the winning triangle through ht_model_hitcheck_mesh on sampled pixels, hand and background
        ys, xs = np.nonzero(body >= 0)
        pick = [(ys[i], xs[i]) for i in rng.choice(len(ys), min(12, len(ys)), replace=False)] + [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(4)]
        off, far = np.float32(r["off"]), np.float32(r["far"])
        for y, x in pick:
            v1 = np.array([((np.float32(x) + off) - CAM[2]) / CAM[0] * far, ((np.float32(y) + off) - CAM[3]) / CAM[1] * far, far], np.float32)
            imp, nrm, b, t = m.hitcheck_mesh(r["pose"], np.zeros(3, np.float32), v1)
            assert (b, t) == (b32[y, x], t32[y, x]), (y, x)
            assert (b >= 0) == (abs(float(np.linalg.norm(nrm)) - 1.0) < 1e-4)
            assert np.uint16(int(imp[2] / CAM[4])) == depth[y, x]
    assert hand > 40 * len(frames["rec"]) // 2      # the hand is in the frames


def test_float32_definition_against_the_float64_evaluation(frames):
    same = differ = 0
    worst = 0
    for r in frames["rec"]:
        d32, b32, t32, _ = r["f32"]
        d64, b64, t64, _ = r["f64"]
        eq = (b32 == b64) & (t32 == t64)
        same += int(eq.sum()); differ += int((~eq).sum())
        if eq.any():
            worst = max(worst, int(np.abs(d32[eq].astype(np.int64) - d64[eq].astype(np.int64)).max()))
    share = differ / float(same + differ)
    print("bones %d: winners differ on %d of %d pixels (share %.3e); worst depth difference where they agree: %d counts" % (frames["nb"], differ, same + differ, share, worst))
    assert worst <= 1
    assert share <= 2 * MEASURED_WINNER_SHARE


def test_hits_lie_in_their_bodys_bound_and_background_is_the_far_point(frames):
    m, nb = frames["model"], frames["nb"]
    rad = [float(np.linalg.norm(frames["corners"][b].reshape(-1, 3).astype(np.float64) - frames["com"][b], axis=1).max()) for b in range(nb)]
    ys, xs = np.mgrid[0:H, 0:W]
    for r in frames["rec"]:
        depth, body = r["host"]
        bg = np.uint16(int(np.float32(r["far"]) / CAM[4]))
        assert np.array_equal(depth[body < 0], np.full(int((body < 0).sum()), bg))
        if r["off"] != 0.0:
            continue
        d = np.stack([(xs - float(CAM[2])) / float(CAM[0]), (ys - float(CAM[3])) / float(CAM[1]), np.ones_like(xs, float)], -1)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        for b in range(nb):
            c = r["pose"][b, :3].astype(np.float64)      # the centre of mass in the poses' frame
            dist = np.linalg.norm(c - (d @ c)[..., None] * d, axis=-1)
            assert (dist[body == b] <= rad[b] + 1e-5).all(), b
    # the hand behind the camera, and a far point short of the hand: all background
    p = frames["rec"][0]["pose"].copy()
    behind = p.copy(); behind[:, 2] = -behind[:, 2]; behind[:, 0] = -behind[:, 0]
    for pose, far in ((behind, 4.0), (p, 0.5 * float(p[:, 2].min()) - 0.05)):
        depth, body = m.render_mesh(pose, CAM, W, H, far, 0.0)
        assert (body == -1).all() and (depth == np.uint16(int(np.float32(far) / CAM[4]))).all()


def test_render_mesh_symbols_exported():
    from hand_tracking_samples_amd import native
    L = native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    for s in ("ht_render_mesh_depth", "ht_render_mesh_depth_dev", "ht_model_hitcheck_mesh", "ht_model_render_mesh", "ht_model_scale"):
        assert s in native.SYMBOLS and s in exported and hasattr(L, s)


def test_render_mesh_rejects_null_context_and_bad_arguments():
    from hand_tracking_samples_amd import native
    L = native.load()
    poses = np.zeros((1, 17, 7), np.float32); cams = np.zeros((1, 12), np.float32); depth = np.zeros((1, 8, 8), np.uint16)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dp = depth.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.ht_render_mesh_depth(None, fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, dp, None) != 0
    assert L.ht_render_mesh_depth_dev(None, poses.ctypes.data, cams.ctypes.data, 8, 8, 4.0, 0.0, 1, depth.ctypes.data, None, None) != 0
    assert L.ht_render_mesh_depth(None, fp(poses), fp(cams), 8, 8, 4.0, 0.0, 0, dp, None) != 0
    # a context that never came up (no device here, or a missing model): the calls below must fail, not crash
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    nan = float("nan")
    try:
        for args in ((None, fp(cams), 8, 8, 4.0, 0.0, 1, dp), (fp(poses), None, 8, 8, 4.0, 0.0, 1, dp), (fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, None),
                     (fp(poses), fp(cams), 0, 8, 4.0, 0.0, 1, dp), (fp(poses), fp(cams), 8, 0, 4.0, 0.0, 1, dp), (fp(poses), fp(cams), 4097, 8, 4.0, 0.0, 1, dp),
                     (fp(poses), fp(cams), 8, 8, 0.0, 0.0, 1, dp), (fp(poses), fp(cams), 8, 8, -1.0, 0.0, 1, dp), (fp(poses), fp(cams), 8, 8, 4.0, nan, 1, dp),
                     (fp(poses), fp(cams), 8, 8, 4.0, 1.5, 1, dp), (fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, dp)):
            assert L.ht_render_mesh_depth(h, *args, None) != 0
            dev = [a if not hasattr(a, "contents") else C.cast(a, C.c_void_p) for a in args]
            assert L.ht_render_mesh_depth_dev(h, *dev, None, None) != 0
    finally:
        if h:
            L.ht_destroy(h)
    # the host definition refuses the same, and a model scales only by a positive factor
    m = native.HostModel(MODELS[17])
    try:
        p = np.zeros((17, 7), np.float32); p[:, 6] = 1; d = np.zeros((8, 8), np.uint16)
        d16 = d.ctypes.data_as(C.POINTER(C.c_uint16))
        for args in ((None, fp(CAM), 8, 8, 4.0, 0.0, d16), (fp(p), None, 8, 8, 4.0, 0.0, d16), (fp(p), fp(CAM), 8, 8, 4.0, 0.0, None), (fp(p), fp(CAM), 0, 8, 4.0, 0.0, d16),
                     (fp(p), fp(CAM), 8, 8, 0.0, 0.0, d16), (fp(p), fp(CAM), 8, 8, 4.0, nan, d16), (fp(p), fp(CAM), 8, 8, 4.0, -0.25, d16)):
            assert L.ht_model_render_mesh(m.m, *args, None) != 0
        assert L.ht_model_render_mesh(None, fp(p), fp(CAM), 8, 8, 4.0, 0.0, d16, None) != 0
        assert L.ht_model_hitcheck_mesh(m.m, None, fp(p), fp(p), None, None, None, None) != 0
        assert L.ht_model_scale(m.m, 0.0) != 0 and L.ht_model_scale(None, 1.0) != 0
    finally:
        m.close()
