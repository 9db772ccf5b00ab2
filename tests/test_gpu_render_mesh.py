"""The device mesh renderer (ht_render_mesh_depth, csrc/ht_render_mesh.hip) held bit for bit, depth and body map, to the host's definition
(ht_model_render_mesh: a plain loop over pixels, bodies and triangles with no culling): small frames that are no multiple of the 16x4 tile with six
cameras and poses per call (truth, across the border, very close, far, the camera origin inside a body's bound, edge-on), both pixel offsets and far
points, 17 and 26 bones; two full 320x240 frames; the empty-tile path; after ht_scale; the _dev entry on a side stream; and render -> track on one stream."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import htfx

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODELS = {17: os.path.join(HERE, "golden", "model_hand17.htfx"), 26: os.path.join(HERE, "golden", "model_hand26.htfx")}
QVGA_CAM = np.array([305, 305, 160, 120, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)      # the application's camera (synthetic-tracker.cpp:98)

pytestmark = pytest.mark.gpu


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


def _truth(nb, k):
    if nb == 17:
        z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
        return z["gtpose"][(37 * k + 5) % len(z["gtpose"])].astype(np.float32)
    G = htfx.load(os.path.join(HERE, "golden", "fullframe5.htfx"))
    return G["f%d/gtpose" % (k % len(G["rows"]))].astype(np.float32)


def _six(nb, seed):
    """the six kinds of test_gpu_render.py, one each: truth, across the border, very close, far, origin inside a body's bound, edge-on"""
    rng = np.random.default_rng(seed)
    p = _truth(nb, seed)
    c = p[:, :3].mean(0).astype(np.float64)
    edge = np.array([(0.0 - 160.0) / 305.0 * c[2], c[1], c[2]])
    out = [p, _rigid(p, np.array([0, 0, 0, 1.0]), edge - c, c),
           _rigid(p, _axis_angle(rng.normal(size=3), rng.uniform(0, np.pi)), np.array([0, 0, 0.12]) - c, c),
           _rigid(p, _axis_angle(rng.normal(size=3), rng.uniform(0, np.pi)), np.array([0.1, -0.05, 2.6]) - c, c)]
    pl0 = htfx.load(MODELS[nb])["b0/planes"]; k = int(np.argmin(-pl0[:, 3]))      # the origin just outside the palm's thinnest side: inside its bound, outside its surface
    want0 = -_qrot(p[0, 3:].astype(np.float64), pl0[k, :3].astype(np.float64) * (-pl0[k, 3] * 1.6))
    out.append(_rigid(p, np.array([0, 0, 0, 1.0]), want0 - p[0, :3], c))
    out.append(_rigid(p, _axis_angle([1, 0, 0], np.pi / 2), np.zeros(3), c))     # fingers along the rays: bodies behind bodies
    return np.stack(out)


def _cams(w, h, n):
    """n different cameras for w x h frames: the application's, scaled to the frame, with varied focal lengths and principal points"""
    c = np.tile(QVGA_CAM, (n, 1))
    for i in range(n):
        f = 305.0 * w / 320.0 * (1.0 + 0.07 * i)
        c[i, :4] = [f, f * (1.0 - 0.02 * i), w / 2.0 + 0.75 * i, h / 2.0 - 0.5 * i]
    return c


def _host(model, poses, cams, w, h, far, off):
    d, b = zip(*[model.render_mesh(poses[i], cams[i], w, h, far, off) for i in range(len(poses))])
    return np.stack(d), np.stack(b)


@pytest.fixture(scope="module", params=[17, 26])
def pair(request):
    from hand_tracking_samples_amd import native
    nb = request.param
    ctx = native.Context(MODELS[nb], 4); m = native.HostModel(MODELS[nb])
    yield nb, ctx, m
    m.close(); ctx.close()


@pytest.mark.parametrize("w,h", [(33, 25), (64, 48)])
@pytest.mark.parametrize("off,far", [(0.0, 4.0), (0.5, 0.85), (0.5, 4.0)])
def test_device_equals_host_on_six_cameras_and_poses(pair, w, h, off, far):
    nb, ctx, m = pair
    poses = _six(nb, 3); cams = _cams(w, h, 6)
    got, gbody = ctx.render_mesh_depth(poses, cams, w, h, far, off, want_body=True)
    want, wbody = _host(m, poses, cams, w, h, far, off)
    if far == 4.0:
        assert (wbody[0] >= 0).any() and (wbody[2] >= 0).any() and (wbody[4] >= 0).any()      # truth, close and origin-inside frames see the hand
    for k in range(6):
        assert np.array_equal(got[k], want[k]), "frame %d: %d pixels differ" % (k, int((got[k] != want[k]).sum()))
        assert np.array_equal(gbody[k], wbody[k]), "frame %d: %d labels differ" % (k, int((gbody[k] != wbody[k]).sum()))


def test_two_full_frames_equal_host():
    from hand_tracking_samples_amd import native
    ctx = native.Context(MODELS[17], 1); m = native.HostModel(MODELS[17])
    try:
        poses = _six(17, 9)[[0, 2]]; cams = np.tile(QVGA_CAM, (2, 1))
        got, gbody = ctx.render_mesh_depth(poses, cams, 320, 240, 4.0, 0.5, want_body=True)
        want, wbody = _host(m, poses, cams, 320, 240, 4.0, 0.5)
    finally:
        m.close(); ctx.close()
    assert (wbody[0] >= 0).mean() > 0.02 and (want[1][wbody[1] >= 0] < 200).any()
    assert np.array_equal(got, want) and np.array_equal(gbody, wbody)


def test_no_body_in_view_is_all_background_and_b0_does_nothing(pair):
    nb, ctx, m = pair
    p = _truth(nb, 1)[None].copy(); p[:, :, 2] -= 10.0
    got, body = ctx.render_mesh_depth(p, QVGA_CAM[None], 100, 75, 0.85, 0.5, want_body=True)
    assert (got == np.uint16(int(np.float32(0.85) / np.float32(0.001)))).all() and (body == -1).all()
    empty = ctx.render_mesh_depth(np.zeros((0, nb, 7), np.float32), np.zeros((0, 12), np.float32), 320, 240)
    assert empty.shape == (0, 240, 320)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    d = np.zeros((1, 8, 8), np.uint16); dp = d.ctypes.data_as(C.POINTER(C.c_uint16)); c = QVGA_CAM[None].copy()
    for w, h, far, off in ((0, 8, 4.0, 0.0), (8, 4097, 4.0, 0.0), (8, 8, -2.0, 0.0), (8, 8, 4.0, float("nan")), (8, 8, 4.0, 1.25)):
        assert ctx.L.ht_render_mesh_depth(ctx.h, fp(p), fp(c), w, h, far, off, 1, dp, None) == 1
    assert ctx.L.ht_render_mesh_depth(ctx.h, None, fp(c), 8, 8, 4.0, 0.0, 1, dp, None) == 1


def test_cnn_only_context_is_refused():
    from hand_tracking_samples_amd import native
    ctx = native.Context(None, 1)
    try:
        p = np.zeros((1, 17, 7), np.float32); d = np.zeros((1, 8, 8), np.uint16); c = QVGA_CAM[None].copy()
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        assert ctx.L.ht_render_mesh_depth(ctx.h, fp(p), fp(c), 8, 8, 4.0, 0.0, 1, d.ctypes.data_as(C.POINTER(C.c_uint16)), None) == 4      # HT_ERR_STATE
    finally:
        ctx.close()


def test_after_scale_device_equals_a_host_model_scaled_alike():
    from hand_tracking_samples_amd import native
    ctx = native.Context(MODELS[17], 1); m = native.HostModel(MODELS[17])
    try:
        ctx.scale(1.15); m.scale(1.15)
        p = _six(17, 6)[[0]]; cams = _cams(64, 48, 1)
        got, gbody = ctx.render_mesh_depth(p, cams, 64, 48, 4.0, 0.5, want_body=True)
        want, wbody = _host(m, p, cams, 64, 48, 4.0, 0.5)
        assert (wbody >= 0).any()
        assert np.array_equal(got, want) and np.array_equal(gbody, wbody)
    finally:
        m.close(); ctx.close()


def test_render_mesh_dev_on_a_side_stream_equals_sync(pair):
    """ht_render_mesh_depth_dev on a non-default stream, into tensors pre-filled with a sentinel: frames and labels equal the synchronous entry's exactly"""
    nb, ctx, m = pair
    w, h, off, far = 33, 25, 0.5, 0.85
    poses = _six(nb, 3); cams = _cams(w, h, 6)
    want, wbody = ctx.render_mesh_depth(poses, cams, w, h, far, off, want_body=True)
    dev = torch.device("cuda:0")
    tp = torch.from_numpy(poses).to(dev); tc = torch.from_numpy(cams).to(dev)
    td = torch.full((6, h, w), 7, dtype=torch.int16, device=dev); tb = torch.full((6, h, w), 5, dtype=torch.int8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        ctx.render_mesh_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, far, off, 6, td.data_ptr(), tb.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(td.cpu().numpy().view(np.uint16), want)
    assert np.array_equal(tb.cpu().numpy(), wbody)


def test_render_mesh_then_track_on_one_stream(weights):
    """ht_render_mesh_depth_dev then ht_update_frames_dev on one stream equals update_frames_sync on the downloaded frames; the hull renderer is undisturbed"""
    from hand_tracking_samples_amd import native
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    n = 4
    poses = z["gtpose"][[3, 200, 470, 900]].astype(np.float32); start = z["startpose"][[3, 200, 470, 900]].astype(np.float32)
    cams = np.tile(QVGA_CAM, (n, 1))
    ctx = native.Context(MODELS[17], n)
    try:
        ctx.load_weights(weights)
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        hull_before = ctx.render_depth(poses, cams, 320, 240)
        dev = torch.device("cuda:0")
        tp = torch.from_numpy(poses).to(dev); tc = torch.from_numpy(cams).to(dev); ts = torch.from_numpy(start).to(dev)
        td = torch.empty((n, 240, 320), dtype=torch.int16, device=dev); out = torch.empty((n, 17, 7), dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        ctx.render_mesh_depth_dev(tp.data_ptr(), tc.data_ptr(), 320, 240, 4.0, 0.0, n, td.data_ptr(), None, s.cuda_stream)
        ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), 320, 240, 0.17, ts.data_ptr(), n, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        frames = td.cpu().numpy().view(np.uint16)
        got = out.cpu().numpy()
        assert (frames < 3999).any()
        assert np.array_equal(frames, ctx.render_mesh_depth(poses, cams, 320, 240, 4.0, 0.0))
        ctx.tracker_reset(start)
        want = ctx.update_frames_sync(frames, cams, 0.17)
        assert np.array_equal(got, want)
        assert np.array_equal(ctx.render_depth(poses, cams, 320, 240), hull_before)
    finally:
        ctx.close()
