"""CPU-only checks of the mesh rasteriser's definition (ht_model_raster_mesh, include/ht_mi355x.h): the host equals the numpy float32
restatement (tests/mesh_raster_ref.py) bit for bit, the definition measured against the mesh ray cast evaluated in float64 (tests/mesh_ray.py), degenerate
frames, a cropped frame, a scaled model and the entry points' refusals."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mesh_ray
import mesh_raster_ref
from test_render_mesh_abi import CAM, H, MODELS, OFFSETS, W, _poses      # the ray cast's own frames: 24x18, six seeded poses, both (offset, far) conventions

W80, H80 = 80, 60
CAM80 = np.array([305 * W80 / 320.0, 305 * W80 / 320.0, 160 * W80 / 320.0, 120 * W80 / 320.0, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)
SIZES = {(W, H): CAM, (W80, H80): CAM80}
# Measured here against mesh_ray.render in float64, per hand and frame width: on the twelve 24x18 frames (six poses, both conventions) and on four 80x60 frames (the
# first four poses, the conventions in turn).  Each bound below is
# twice the measured share; a measured 0 is bound by 0, the inputs being fixed.
#   coverage: pixels that one renderer covers and the other does not, of all pixels
#   winner:   pixels that both cover with different (body, triangle), of the pixels both cover
#   on a triangle both pick, the counts were equal on every pixel measured (the definition allows 1)
MEASURED_COVERAGE_SHARE = {(17, 24): 1 / 5184.0, (17, 80): 1 / 19200.0, (26, 24): 0.0, (26, 80): 0.0}
MEASURED_WINNER_SHARE = {(17, 24): 5 / 441.0, (17, 80): 8 / 1588.0, (26, 24): 4 / 428.0, (26, 80): 8 / 1639.0}


CLOSE_W, CLOSE_H = 64, 48
CLOSE_CAM = np.array([61, 61, 32, 24, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)


def close_up(pose, z):
    """the hand centred on the optical axis, its bodies' mean at distance z: at 0.06 to 0.10 m it fills CLOSE_CAM's 64x48 frame and single triangles cover hundreds of pixels"""
    q = pose.copy(); q[:, :3] -= q[:, :3].mean(0); q[:, 2] += np.float32(z)
    return q


def _bg(far, cam=CAM):
    return np.uint16(int(np.float32(far) / cam[4]))


@pytest.fixture(scope="module", params=[17, 26])
def frames(request):
    """per size: the host's frames, the float32 restatement and the float64 ray cast of the same poses; computed once, shared and left unchanged"""
    from hand_tracking_samples_amd import native
    nb = request.param
    m = native.HostModel(MODELS[nb])
    corners = [m.sdmesh(b).reshape(-1, 3, 3) for b in range(nb)]
    com = np.stack([m.com(b) for b in range(nb)])
    m32, m64 = mesh_ray.Mesh(corners, com, np.float32), mesh_ray.Mesh(corners, com, np.float64)
    poses = _poses(nb)
    rec = []
    for (w, h), cam in SIZES.items():
        for i, p in enumerate(poses):
            for j, (off, far) in enumerate(OFFSETS):
                if w == W80 and (i >= 4 or j != i % 2):      # the float64 ray cast of an 80x60 frame takes seconds: four frames, the conventions in turn
                    continue
                rec.append(dict(w=w, h=h, cam=cam, pose=p, off=off, far=far, host=m.raster_mesh(p, cam, w, h, far, off), f32=mesh_raster_ref.render(m32, p, cam, w, h, far, off),
                                ray64=mesh_ray.render(m64, p, cam, w, h, far, off)))
    yield dict(nb=nb, model=m, m32=m32, rec=rec)
    m.close()


def test_host_equals_the_numpy_restatement_bit_for_bit(frames):
    hand = 0
    for r in frames["rec"]:
        depth, body = r["host"]
        d32, b32, _ = r["f32"]
        assert np.array_equal(depth, d32), (r["w"], r["off"])
        assert np.array_equal(body, b32), (r["w"], r["off"])
        assert np.array_equal(depth[body < 0], np.full(int((body < 0).sum()), _bg(r["far"])))
        hand += int((body >= 0).sum())
    assert hand > 40 * len(frames["rec"]) // 2      # the hand is in the frames
    # a hand that straddles the near distance (its crossing triangles are dropped) and one close to the camera, whose triangles cover many pixels
    m, p = frames["model"], frames["rec"][0]["pose"]
    for dz in (0.02, 0.08):
        q = close_up(p, dz)
        host = m.raster_mesh(q, CLOSE_CAM, CLOSE_W, CLOSE_H, 4.0, 0.0)
        ref = mesh_raster_ref.render(frames["m32"], q, CLOSE_CAM, CLOSE_W, CLOSE_H, 4.0, 0.0)
        assert np.array_equal(host[0], ref[0]) and np.array_equal(host[1], ref[1])
        assert (host[1] >= 0).sum() > CLOSE_W * CLOSE_H // 2


@pytest.mark.parametrize("w", [W, W80])
def test_against_the_float64_ray_cast(frames, w):
    total = cover = both = winners = 0
    worst_same = 0
    for r in frames["rec"]:
        if r["w"] != w:
            continue
        depth, body = r["host"]
        _, _, tri = r["f32"]
        d64, b64, t64, _ = r["ray64"]
        hit_r, hit_c = body >= 0, b64 >= 0
        total += depth.size; cover += int((hit_r != hit_c).sum())
        bo = hit_r & hit_c
        same = bo & (body == b64) & (tri == t64)
        diff = np.abs(depth.astype(np.int64) - d64.astype(np.int64))
        both += int(bo.sum()); winners += int((bo & ~same).sum())
        if same.any():
            worst_same = max(worst_same, int(diff[same].max()))
        assert not (bo & same & (diff > 1)).any()      # no pixel both cover differs by more than a count unless the winners differ
        # no hole: a pixel whose whole 3x3 neighbourhood the ray cast hits is covered
        full = hit_c.copy(); full[0, :] = full[-1, :] = False; full[:, 0] = full[:, -1] = False
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                full[1:-1, 1:-1] &= hit_c[1 + dy:hit_c.shape[0] - 1 + dy, 1 + dx:hit_c.shape[1] - 1 + dx]
        assert not (full & ~hit_r).any()
    cs, ws = cover / float(total), winners / float(both)
    print("bones %d, width %d: coverage differs on %d of %d pixels (share %.3e); winners differ on %d of %d pixels both cover (share %.3e); worst difference on the same triangle: %d counts"
          % (frames["nb"], w, cover, total, cs, winners, both, ws, worst_same))
    assert worst_same <= 1
    assert cs <= 2 * MEASURED_COVERAGE_SHARE[(frames["nb"], w)]
    assert ws <= 2 * MEASURED_WINNER_SHARE[(frames["nb"], w)]


def test_degenerate_frames_are_background(frames):
    m, p = frames["model"], frames["rec"][0]["pose"]
    behind = p.copy(); behind[:, 2] = -behind[:, 2]; behind[:, 0] = -behind[:, 0]
    near = p.copy(); near[:, 2] -= float(p[:, 2].max()) + 0.15      # every corner of the hand at z < HT_RASTER_NEAR (a body's mesh reaches less than 0.15 m from its centre of mass)
    away = CAM.copy(); away[2] = -1000.0                          # the hand wholly to the left of the image
    for pose, cam, far in ((behind, CAM, 4.0), (p, CAM, 0.5 * float(p[:, 2].min()) - 0.05), (near, CAM, 4.0), (p, away, 4.0)):
        depth, body = m.raster_mesh(pose, cam, W, H, far, 0.0)
        assert (body == -1).all() and (depth == _bg(far)).all()


def test_a_hand_half_outside_is_the_crop_of_a_wider_frame(frames):
    m = frames["model"]
    for r in frames["rec"][:4]:
        if r["w"] != W:
            continue
        body = r["host"][1]
        xs = np.nonzero((body >= 0).any(0))[0]
        cut = int(xs[0] + xs[-1] + 1) // 2                  # the column through the middle of the hand becomes the narrow frame's first
        narrow = CAM.copy(); narrow[2] = CAM[2] - cut        # pixel x of the narrow frame is pixel x + cut of the wide one
        d, b = m.raster_mesh(r["pose"], narrow, W - cut, H, r["far"], r["off"])
        assert (b[:, 0] >= 0).any() and np.array_equal(d, r["host"][0][:, cut:]) and np.array_equal(b, body[:, cut:])


def test_scaled_model_equals_the_restatement_on_the_scaled_corners(frames):
    from hand_tracking_samples_amd import native
    nb = frames["nb"]
    m = native.HostModel(MODELS[nb])
    try:
        m.scale(1.15)
        corners = [m.sdmesh(b).reshape(-1, 3, 3) for b in range(nb)]
        com = np.stack([m.com(b) for b in range(nb)])
        assert np.array_equal(corners[0], frames["m32"].corners[0] * np.float32(1.15))
        m32 = mesh_ray.Mesh(corners, com, np.float32)
        for r in frames["rec"][:2]:
            host = m.raster_mesh(r["pose"], CAM, W, H, r["far"], r["off"])
            ref = mesh_raster_ref.render(m32, r["pose"], CAM, W, H, r["far"], r["off"])
            assert np.array_equal(host[0], ref[0]) and np.array_equal(host[1], ref[1])
            assert not np.array_equal(host[0], r["host"][0])
    finally:
        m.close()


def test_raster_kernel_resources():
    """one kernel, no scratch, no spills; a band's z-buffer leaves room for two blocks in a CU's 160 KiB of LDS, at two waves a SIMD or more"""
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not any("k_raster_mesh" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    k = {n: v for n, v in u.items() if "k_raster_mesh" in n}
    assert len(k) == 1
    for n, v in k.items():
        print("%s VGPRs %d LDS %d scratch %d" % (n, v["VGPRs"], v["LDS Size"], v["ScratchSize"]))
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and 2 * v["LDS Size"] <= 163840 and v["Occupancy"] >= 2, (n, v)


def test_raster_mesh_symbols_exported():
    from hand_tracking_samples_amd import native
    L = native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    for s in ("ht_raster_mesh_depth", "ht_raster_mesh_depth_dev", "ht_model_raster_mesh"):
        assert s in native.SYMBOLS and s in exported and hasattr(L, s)


def test_raster_mesh_rejects_null_context_and_bad_arguments():
    from hand_tracking_samples_amd import native
    L = native.load()
    poses = np.zeros((1, 17, 7), np.float32); cams = np.zeros((1, 12), np.float32); depth = np.zeros((1, 8, 8), np.uint16)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dp = depth.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.ht_raster_mesh_depth(None, fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, dp, None) != 0
    assert L.ht_raster_mesh_depth_dev(None, poses.ctypes.data, cams.ctypes.data, 8, 8, 4.0, 0.0, 1, depth.ctypes.data, None, None) != 0
    assert L.ht_raster_mesh_depth(None, fp(poses), fp(cams), 8, 8, 4.0, 0.0, 0, dp, None) != 0
    # a context that never came up (no device here, or a missing model): every call must fail as the ray cast's does, not crash
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    nan = float("nan")
    try:
        for args in ((None, fp(cams), 8, 8, 4.0, 0.0, 1, dp), (fp(poses), None, 8, 8, 4.0, 0.0, 1, dp), (fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, None),
                     (fp(poses), fp(cams), 0, 8, 4.0, 0.0, 1, dp), (fp(poses), fp(cams), 8, 0, 4.0, 0.0, 1, dp), (fp(poses), fp(cams), 4097, 8, 4.0, 0.0, 1, dp),
                     (fp(poses), fp(cams), 8, 8, 0.0, 0.0, 1, dp), (fp(poses), fp(cams), 8, 8, -1.0, 0.0, 1, dp), (fp(poses), fp(cams), 8, 8, 4.0, nan, 1, dp),
                     (fp(poses), fp(cams), 8, 8, 4.0, 1.5, 1, dp), (fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, dp)):
            rc = L.ht_raster_mesh_depth(h, *args, None)
            assert rc != 0 and rc == L.ht_render_mesh_depth(h, *args, None)
            dev = [a if not hasattr(a, "contents") else C.cast(a, C.c_void_p) for a in args]
            rc = L.ht_raster_mesh_depth_dev(h, *dev, None, None)
            assert rc != 0 and rc == L.ht_render_mesh_depth_dev(h, *dev, None, None)
    finally:
        if h:
            L.ht_destroy(h)
    m = native.HostModel(MODELS[17])
    try:
        p = np.zeros((17, 7), np.float32); p[:, 6] = 1; d = np.zeros((8, 8), np.uint16)
        d16 = d.ctypes.data_as(C.POINTER(C.c_uint16))
        for args in ((None, fp(CAM), 8, 8, 4.0, 0.0, d16), (fp(p), None, 8, 8, 4.0, 0.0, d16), (fp(p), fp(CAM), 8, 8, 4.0, 0.0, None), (fp(p), fp(CAM), 0, 8, 4.0, 0.0, d16),
                     (fp(p), fp(CAM), 8, 4097, 4.0, 0.0, d16), (fp(p), fp(CAM), 8, 8, 0.0, 0.0, d16), (fp(p), fp(CAM), 8, 8, 4.0, nan, d16), (fp(p), fp(CAM), 8, 8, 4.0, -0.25, d16),
                     (fp(p), fp(CAM), 8, 8, 4.0, 1.25, d16)):
            rc = L.ht_model_raster_mesh(m.m, *args, None)
            assert rc != 0 and rc == L.ht_model_render_mesh(m.m, *args, None)
        assert L.ht_model_raster_mesh(None, fp(p), fp(CAM), 8, 8, 4.0, 0.0, d16, None) != 0
        assert L.ht_model_raster_mesh(m.m, fp(p), fp(CAM), 8, 8, 4.0, 0.0, d16, None) == 0      # the body image is optional
    finally:
        m.close()
