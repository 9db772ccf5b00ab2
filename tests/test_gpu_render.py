"""The device renderer (ht_render_depth, csrc/ht_render.hip): the application's software rasteriser FakeDepth (synthetic-tracker.cpp:69-76) for a batch
of frames, held bit for bit to

  - the reference's own renders (tests/golden/fullframe320.htfx, fullframe320close.htfx: 17 bones, 320x240; fullframe5.htfx: 26 bones, 128x128),
  - the host's HitCheck (tests/cxx_headless_driver.cpp `fakedepth`, the statement already pinned to the reference by tests/test_cxx_driver.py) on
    varied poses: the bench's ground truths at 320x240 and at their own tile cameras, and perturbations that put the hand across the border, very
    close to the camera, far away, around the camera (the origin inside a body's bounding sphere, outside its hull), turned edge-on,
  - and ht_model_hitcheck's body index on a sample of pixels.
Then the closed loop (render -> ht_update_frames_dev on one stream) against update_frames_sync on the stored frames, and no interference with tracking."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import htfx
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL26 = os.path.join(HERE, "golden", "model_hand26.htfx")
FIXTURES = {"fullframe320": ol.MODEL, "fullframe320close": ol.MODEL, "fullframe5": MODEL26}
QVGA_CAM = np.array([305, 305, 160, 120, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)      # the application's camera (synthetic-tracker.cpp:98)

pytestmark = pytest.mark.gpu


def _fixture(name):
    G = htfx.load(os.path.join(HERE, "golden", name + ".htfx"))
    n = len(G["rows"])
    return (np.stack([G["f%d/gtpose" % f] for f in range(n)]), np.stack([G["f%d/cam" % f] for f in range(n)]), np.stack([G["f%d/depth" % f] for f in range(n)]), G)


@pytest.fixture(scope="module")
def host_driver(tmp_path_factory):
    from hand_tracking_samples_amd import native
    native.load()
    d = tmp_path_factory.mktemp("render_drv")
    lib = os.path.dirname(native.lib_path())
    exe = str(d / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cxx_headless_driver.cpp"), "-o", exe, "-L" + lib, "-lht_mi355x", "-Wl,-rpath," + lib])
    return exe, d


def _host_render(host_driver, model, poses, cams, w, h):
    """FakeDepth on the host (PhysModel::HitCheck per pixel, 4 m far point) for frames of one size."""
    exe, d = host_driver
    n, nb = poses.shape[:2]
    with open(d / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", n, w, h, nb))
        for k in range(n):
            f.write(np.zeros(w * h, np.uint16).tobytes()); f.write(np.ascontiguousarray(cams[k], np.float32).tobytes())
            f.write(np.ascontiguousarray(poses[k], np.float32).tobytes()); f.write(np.ascontiguousarray(poses[k], np.float32).tobytes())
    subprocess.check_output([exe, "fakedepth", model, str(d / "in.bin"), str(d / "out.bin")], timeout=600)
    return np.fromfile(d / "out.bin", np.uint16).reshape(n, h, w)


def _qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([ax * bw + aw * bx + ay * bz - az * by, ay * bw + aw * by + az * bx - ax * bz, az * bw + aw * bz + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _qrot(q, v):
    x, y, z, w = q
    m = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - z * w), 2 * (z * x + y * w)],
                  [2 * (x * y + z * w), w * w - x * x + y * y - z * z, 2 * (y * z - x * w)],
                  [2 * (z * x - y * w), 2 * (y * z + x * w), w * w - x * x - y * y + z * z]])
    return m @ v


def _rigid(poses, q, t, about):
    """the whole hand moved rigidly: rotation q about the point `about`, then translation t"""
    out = poses.astype(np.float64).copy()
    for b in range(len(out)):
        out[b, :3] = _qrot(q, out[b, :3] - about) + about + t
        out[b, 3:] = _qmul(q, out[b, 3:])
        out[b, 3:] /= np.linalg.norm(out[b, 3:])
    return out.astype(np.float32)


def _axis_angle(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]])


def _varied_qvga(model):
    """ground-truth hands of the bench recording at the application's camera, and seeded perturbations of them"""
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    M = htfx.load(model)
    pl0 = M["b0/planes"]; hmin = int(np.argmin(-pl0[:, 3]))
    rng = np.random.default_rng(7)
    out, kinds = [], []
    for i, k in enumerate(rng.choice(len(z["gtpose"]), 12, replace=False)):
        p = z["gtpose"][k]
        c = p[:, :3].mean(0)
        out.append(p); kinds.append("truth")
        edge = np.array([(0.0 - 160.0) / 305.0 * c[2], c[1], c[2]]) if i % 2 else np.array([c[0], (239.0 - 120.0) / 305.0 * c[2], c[2]])
        out.append(_rigid(p, np.array([0, 0, 0, 1.0]), edge - c, c)); kinds.append("border")
        out.append(_rigid(p, _axis_angle(rng.normal(size=3), rng.uniform(0, np.pi)), np.array([0, 0, 0.12]) - c, c)); kinds.append("close")
        out.append(_rigid(p, _axis_angle(rng.normal(size=3), rng.uniform(0, np.pi)), np.array([0.1, -0.05, 2.6]) - c, c)); kinds.append("far")
        # the origin just outside the palm's thinnest face: inside its bounding sphere, outside its hull
        n = pl0[hmin, :3].astype(np.float64); local = n * (-pl0[hmin, 3] * (1.2 + 0.3 * rng.uniform()))
        want0 = -_qrot(p[0, 3:].astype(np.float64), local)
        out.append(_rigid(p, np.array([0, 0, 0, 1.0]), want0 - p[0, :3], c)); kinds.append("origin_in_sphere")
        out.append(_rigid(p, _axis_angle([1, 0, 0], np.pi / 2 * (1 if i % 2 else -1)), np.zeros(3), c)); kinds.append("edge_on")      # fingers along the rays: bodies behind bodies
    return np.stack(out), kinds


def _ctx(model, B=1):
    from hand_tracking_samples_amd import native
    return native.Context(model, B)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_render_equals_the_references_own_frames(name):
    poses, cams, depth, G = _fixture(name)
    w, h = (int(x) for x in G["dims"])
    ctx = _ctx(FIXTURES[name])
    try:
        got = ctx.render_depth(poses, cams, w, h)
    finally:
        ctx.close()
    assert got.shape == depth.shape
    assert (depth < 3999).any()      # there is a hand in every fixture
    assert np.array_equal(got, depth)


def test_render_equals_the_host_hitcheck_on_varied_poses(host_driver):
    poses, kinds = _varied_qvga(ol.MODEL)
    cams = np.tile(QVGA_CAM, (len(poses), 1))
    ctx = _ctx(ol.MODEL)
    try:
        got, body = ctx.render_depth(poses, cams, 320, 240, want_body=True)
        want = _host_render(host_driver, ol.MODEL, poses, cams, 320, 240)
        # the bench's own tiles: 64x64 frames with their recorded cameras
        z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
        tp, tc = z["gtpose"][:64], z["cam"][:64]
        got_t = ctx.render_depth(tp, tc, 64, 64)
        want_t = _host_render(host_driver, ol.MODEL, tp, tc, 64, 64)
        for k in range(len(tp)):
            assert np.array_equal(got_t[k], want_t[k]), "tile %d: %d pixels differ" % (k, int((got_t[k] != want_t[k]).sum()))
    finally:
        ctx.close()
    kinds = np.array(kinds)
    assert len(poses) >= 64
    hand = want < 3999
    assert hand[kinds == "border"][:, :, 0].any() or hand[kinds == "border"][:, -1, :].any()      # the hand crosses the border
    assert (want[kinds == "close"][hand[kinds == "close"]] < 150).any()                            # ... comes within 15 cm
    assert (want[kinds == "far"][hand[kinds == "far"]] > 2400).any()                               # ... is far out
    assert hand[kinds == "origin_in_sphere"].any()
    for k in range(len(poses)):
        assert np.array_equal(got[k], want[k]), "frame %d (%s): %d pixels differ" % (k, kinds[k], int((got[k] != want[k]).sum()))
    assert np.array_equal(body >= 0, got < 3999)      # every hand pixel names its body, the background none
    # the body index against ht_model_hitcheck on a sample of pixels (hand and background)
    from hand_tracking_samples_amd import native
    L = native.load()
    m = C.c_void_p()
    assert L.ht_model_open(ol.MODEL.encode(), 1, C.byref(m)) == 0
    try:
        rng = np.random.default_rng(3)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        checked = 0
        for k in range(0, len(poses), 3):
            ys, xs = np.nonzero(hand[k])
            pick = [(ys[i], xs[i]) for i in rng.choice(len(ys), min(40, len(ys)), replace=False)] if len(ys) else []
            pick += [(rng.integers(240), rng.integers(320)) for _ in range(10)]
            pk = np.ascontiguousarray(poses[k], np.float32)
            for y, x in pick:
                far = np.array([(np.float32(x) - np.float32(160)) / np.float32(305) * np.float32(4), (np.float32(y) - np.float32(120)) / np.float32(305) * np.float32(4), 4], np.float32)
                v0 = np.zeros(3, np.float32); imp = np.zeros(3, np.float32); nrm = np.zeros(3, np.float32); rb = C.c_int(-2)
                assert L.ht_model_hitcheck(m, fp(pk), fp(v0), fp(far), fp(imp), fp(nrm), C.byref(rb)) == 0
                assert body[k, y, x] == rb.value, (k, y, x)
                checked += 1
        assert checked > 500
    finally:
        L.ht_model_close(m)


def test_render_odd_shapes_and_batches(host_driver):
    poses, cams, _, _ = _fixture("fullframe320")
    ctx = _ctx(ol.MODEL)
    try:
        for (w, h) in ((100, 75), (1, 1), (321, 17)):
            cam = QVGA_CAM.copy(); cam[2], cam[3] = w / 2.0, h / 2.0
            if w == 1:
                cam[0] = cam[1] = 2.0      # a 1x1 frame looking straight at the hand
            for B in (1, 37):
                p = np.stack([poses[i % len(poses)] for i in range(B)])
                c = np.tile(cam, (B, 1))
                got = ctx.render_depth(p, c, w, h)
                want = _host_render(host_driver, ol.MODEL, p[:2], c[:2], w, h)
                assert got.shape == (B, h, w)
                for i in range(B):
                    assert np.array_equal(got[i], want[i % 2]), (w, h, B, i)
        empty = ctx.render_depth(np.zeros((0, 17, 7), np.float32), np.zeros((0, 12), np.float32), 320, 240)
        assert empty.shape == (0, 240, 320)
    finally:
        ctx.close()


def test_render_dev_on_a_side_stream_equals_sync():
    poses, _ = _varied_qvga(ol.MODEL)
    poses = poses[:16]
    cams = np.tile(QVGA_CAM, (len(poses), 1))
    ctx = _ctx(ol.MODEL)
    try:
        want, wbody = ctx.render_depth(poses, cams, 320, 240, want_body=True)
        dev = torch.device("cuda:0")
        tp = torch.from_numpy(poses).to(dev); tc = torch.from_numpy(cams).to(dev)
        td = torch.full((len(poses), 240, 320), 7, dtype=torch.int16, device=dev); tb = torch.full((len(poses), 240, 320), 5, dtype=torch.int8, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            ctx.render_depth_dev(tp.data_ptr(), tc.data_ptr(), 320, 240, 4.0, len(poses), td.data_ptr(), tb.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert np.array_equal(td.cpu().numpy().view(np.uint16), want)
        assert np.array_equal(tb.cpu().numpy(), wbody)
    finally:
        ctx.close()


def test_render_argument_errors_on_a_live_context():
    from hand_tracking_samples_amd import native
    ctx = _ctx(ol.MODEL)
    L = ctx.L
    p = np.zeros((1, 17, 7), np.float32); c = np.tile(QVGA_CAM, (1, 1)); d = np.zeros((1, 8, 8), np.uint16)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); dp = d.ctypes.data_as(C.POINTER(C.c_uint16))
    try:
        assert L.ht_render_depth(ctx.h, None, fp(c), 8, 8, 4.0, 1, dp, None) == 1
        assert L.ht_render_depth(ctx.h, fp(p), None, 8, 8, 4.0, 1, dp, None) == 1
        assert L.ht_render_depth(ctx.h, fp(p), fp(c), 8, 8, 4.0, 1, None, None) == 1
        for w, h, far in ((0, 8, 4.0), (8, 0, 4.0), (4097, 8, 4.0), (8, 4097, 4.0), (8, 8, 0.0), (8, 8, -2.0)):
            assert L.ht_render_depth(ctx.h, fp(p), fp(c), w, h, far, 1, dp, None) == 1
        assert L.ht_render_depth(ctx.h, fp(p), fp(c), 8, 8, 4.0, 0, dp, None) == 0      # B = 0: nothing to do
        assert L.ht_render_depth(ctx.h, fp(p), fp(c), 8, 8, 4.0, 1, dp, None) == 0
    finally:
        ctx.close()
    cnn_only = native.Context(None, 1)
    try:
        assert cnn_only.L.ht_render_depth(cnn_only.h, fp(p), fp(c), 8, 8, 4.0, 1, dp, None) == 4      # HT_ERR_STATE: no hand model
    finally:
        cnn_only.close()


def test_render_then_track_on_one_stream_equals_tracking_the_stored_frames(weights):
    """closed loop: the reference's fullframe320 poses rendered on the device feed ht_update_frames_dev on the same stream; the poses equal those
    update_frames_sync gives on the fixture's stored frames (same weights, start poses and parameters)"""
    import torch
    poses, cams, depth, G = _fixture("fullframe320")
    n = len(poses)
    start = np.stack([G["f%d/startpose" % f] for f in range(n)])
    ctx = _ctx(ol.MODEL, n)
    try:
        ctx.load_weights(weights)
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        ctx.tracker_reset(start)
        want = ctx.update_frames_sync(depth, cams, 0.17)
        dev = torch.device("cuda:0")
        tp = torch.from_numpy(poses).to(dev); tc = torch.from_numpy(cams).to(dev); ts = torch.from_numpy(start).to(dev)
        td = torch.empty((n, 240, 320), dtype=torch.int16, device=dev); out = torch.empty((n, 17, 7), dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        ctx.render_depth_dev(tp.data_ptr(), tc.data_ptr(), 320, 240, 4.0, n, td.data_ptr(), None, s.cuda_stream)
        ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), 320, 240, 0.17, ts.data_ptr(), n, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert np.array_equal(td.cpu().numpy().view(np.uint16), depth)
        assert np.array_equal(out.cpu().numpy(), want)
    finally:
        ctx.close()


def test_render_between_updates_does_not_disturb_tracking(weights):
    poses, cams, depth, G = _fixture("fullframe320")
    n = len(poses)
    start = np.stack([G["f%d/startpose" % f] for f in range(n)])
    res = []
    for render in (False, True):
        ctx = _ctx(ol.MODEL, n)
        try:
            ctx.load_weights(weights)
            ctx.set_params(microforce=3.0, mainthreadpasses=3)
            ctx.tracker_reset(start)
            a = ctx.update_frames_sync(depth, cams, 0.17)
            if render:
                v, _ = _varied_qvga(ol.MODEL)
                ctx.render_depth(v[:40], np.tile(QVGA_CAM, (40, 1)), 320, 240, want_body=True)      # more frames than the context's max_batch
            b = ctx.update_frames_sync(depth, cams, 0.17)
            res.append((a, b, ctx.get_state(0, n)))
        finally:
            ctx.close()
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(x, y)
