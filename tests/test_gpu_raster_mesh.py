"""The device mesh rasteriser (ht_raster_mesh_depth, csrc/ht_raster_mesh.hip) held bit for bit, depth and body map, to the host's definition
(ht_model_raster_mesh: a plain loop over bodies, triangles and pixels): small frames, frames that cross the kernel's band and write-out group edges, a
hand close to the camera (triangles walked by a whole wave) and half outside the frame, determinism, the _dev entry on a side stream, raster -> track on
one stream, after ht_scale, and the refusals.

The kernel's tiling (csrc/ht_raster_mesh.hip): one block per band of rows of at most RZ_PIX = 19200 pixels, bands of equal height (the last one shorter); the
band is written out in groups of four pixels aligned in the batch; a triangle whose pixel rectangle has RZ_BIG = 64 pixels or more is walked by its wave."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mesh_ray import _qmat
from test_gpu_render_mesh import MODELS, QVGA_CAM, ROOT, _cams, _six
from test_raster_mesh_ref import CLOSE_CAM, CLOSE_H, CLOSE_W, close_up

pytestmark = pytest.mark.gpu
CONVENTIONS = ((0.0, 4.0), (0.5, 0.85))


def _host(model, poses, cams, w, h, far, off):
    d, b = zip(*[model.raster_mesh(poses[i], cams[i], w, h, far, off) for i in range(len(poses))])
    return np.stack(d), np.stack(b)


def _equal(ctx, m, poses, cams, w, h, far, off):
    got, gbody = ctx.raster_mesh_depth(poses, cams, w, h, far, off, want_body=True)
    want, wbody = _host(m, poses, cams, w, h, far, off)
    for k in range(len(poses)):
        assert np.array_equal(got[k], want[k]), "frame %d: %d pixels differ" % (k, int((got[k] != want[k]).sum()))
        assert np.array_equal(gbody[k], wbody[k]), "frame %d: %d labels differ" % (k, int((gbody[k] != wbody[k]).sum()))
    return want, wbody


def _largest_rectangle(m, nb, pose, cam, w, h):
    """the most pixels in the rectangle of one triangle in front of the near distance (in double: a size, not a definition)"""
    best = 0
    for b in range(nb):
        T = m.sdmesh(b).reshape(-1, 3, 3).astype(np.float64)
        R = np.array(_qmat(list(pose[b, 3:].astype(np.float64)))).T
        Wc = T @ R.T + (pose[b, :3] - R @ m.com(b).astype(np.float64))
        sx = cam[0] * Wc[:, :, 0] / Wc[:, :, 2] + cam[2]; sy = cam[1] * Wc[:, :, 1] / Wc[:, :, 2] + cam[3]
        x0 = np.clip(np.ceil(sx.min(1)), 0, w - 1); x1 = np.clip(np.floor(sx.max(1)), 0, w - 1); y0 = np.clip(np.ceil(sy.min(1)), 0, h - 1); y1 = np.clip(np.floor(sy.max(1)), 0, h - 1)
        a = (x1 - x0 + 1) * (y1 - y0 + 1)
        a[(Wc[:, :, 2] < 0.011).any(1) | (x1 < x0) | (y1 < y0)] = 0
        best = max(best, int(a.max()))
    return best


@pytest.fixture(scope="module", params=[17, 26])
def pair(request):
    from hand_tracking_samples_amd import native
    nb = request.param
    ctx = native.Context(MODELS[nb], 4); m = native.HostModel(MODELS[nb])
    yield nb, ctx, m
    m.close(); ctx.close()


@pytest.mark.parametrize("w,h", [(24, 18), (37, 29), (100, 75)])
@pytest.mark.parametrize("off,far", CONVENTIONS)
def test_device_equals_host_on_six_cameras_and_poses(pair, w, h, off, far):
    nb, ctx, m = pair
    poses = _six(nb, 3); cams = _cams(w, h, 6)
    want, wbody = _equal(ctx, m, poses, cams, w, h, far, off)
    if far == 4.0:
        assert (wbody[0] >= 0).any() and (wbody[2] >= 0).any() and (wbody[3] >= 0).any()      # the truth, close and far frames see the hand


def test_two_full_frames_equal_host(pair):
    """320x240: four bands of 60 rows per frame"""
    nb, ctx, m = pair
    poses = _six(nb, 9)[[0, 2]]; cams = np.tile(QVGA_CAM, (2, 1))
    want, wbody = _equal(ctx, m, poses, cams, 320, 240, 4.0, 0.5)
    assert (wbody[0] >= 0).mean() > 0.02 and (want[1][wbody[1] >= 0] < 200).any()


@pytest.mark.parametrize("w,h", [(333, 61),      # 57 rows fit a band: two bands of 31 and 30 rows, and odd band starts, so the write-out groups straddle band and frame edges
                                 (7, 251),       # one band of 1757 pixels, no multiple of four, the second frame starting at an odd pixel
                                 (4096, 5)])     # the widest frame: four rows fit a band, bands of 3 and 2 rows
def test_frames_across_band_and_group_edges(pair, w, h):
    nb, ctx, m = pair
    p = _six(nb, 3)[[0, 2]]
    f = 305.0 * min(w / 320.0, h / 240.0) * 3.0      # the hand about as large as the frame's short side
    cams = np.tile(QVGA_CAM, (2, 1)); cams[:, :4] = [f, f, w / 2.0, h / 2.0]
    c = p[0, :, :3].mean(0); p[0, :, :2] -= c[:2]      # the first frame's hand on the axis
    want, wbody = _equal(ctx, m, p, cams, w, h, 4.0, 0.5)
    assert (wbody[0] >= 0).any(1).sum() >= min(h, 4) and (wbody >= 0).sum() > 40


def test_close_up_and_half_outside(pair):
    nb, ctx, m = pair
    from test_render_mesh_abi import _poses
    base = _poses(nb)
    poses = np.stack([close_up(base[0], 0.06), close_up(base[1], 0.08), close_up(base[2], 0.10)])
    cams = np.tile(CLOSE_CAM, (3, 1))
    assert _largest_rectangle(m, nb, poses[0], CLOSE_CAM, CLOSE_W, CLOSE_H) >= 128      # well past RZ_BIG: the wave's walk runs
    for off, far in CONVENTIONS:
        want, wbody = _equal(ctx, m, poses, cams, CLOSE_W, CLOSE_H, far, off)
        assert (wbody[0] >= 0).mean() > 0.5
    # half outside: the frame starts at the column through the middle of the hand
    p = _six(nb, 3)[[0]]; cam = _cams(100, 75, 1)
    _, b = _host(m, p, cam, 100, 75, 4.0, 0.0)
    xs = np.nonzero((b[0] >= 0).any(0))[0]; cut = int(xs[0] + xs[-1] + 1) // 2
    cam[0, 2] -= cut
    want, wbody = _equal(ctx, m, p, cam, 100 - cut, 75, 4.0, 0.0)
    assert (wbody[0][:, 0] >= 0).any()


def test_two_calls_give_the_same_bits(pair):
    nb, ctx, m = pair
    poses = np.concatenate([_six(nb, 3), close_up(_six(nb, 3)[0], 0.07)[None]]); cams = np.tile(CLOSE_CAM, (7, 1))
    a = ctx.raster_mesh_depth(poses, cams, CLOSE_W, CLOSE_H, 4.0, 0.5, want_body=True)
    b = ctx.raster_mesh_depth(poses, cams, CLOSE_W, CLOSE_H, 4.0, 0.5, want_body=True)
    assert (a[1] >= 0).any() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(ctx.raster_mesh_depth(poses, cams, CLOSE_W, CLOSE_H, 4.0, 0.5), a[0])      # without the body image


def test_raster_mesh_dev_on_a_side_stream_equals_sync(pair):
    """ht_raster_mesh_depth_dev on a non-default stream, into tensors pre-filled with a sentinel: frames and labels equal the synchronous entry's exactly"""
    nb, ctx, m = pair
    w, h, off, far = 37, 29, 0.5, 0.85
    poses = _six(nb, 3); cams = _cams(w, h, 6)
    want, wbody = ctx.raster_mesh_depth(poses, cams, w, h, far, off, want_body=True)
    dev = torch.device("cuda:0")
    tp = torch.from_numpy(poses).to(dev); tc = torch.from_numpy(cams).to(dev)
    td = torch.full((6 * h * w + 1,), 7, dtype=torch.int16, device=dev); tb = torch.full((6 * h * w + 1,), 5, dtype=torch.int8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        ctx.raster_mesh_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, far, off, 6, td.data_ptr(), tb.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(td[:-1].cpu().numpy().view(np.uint16).reshape(6, h, w), want) and int(td[-1]) == 7
    assert np.array_equal(tb[:-1].cpu().numpy().reshape(6, h, w), wbody) and int(tb[-1]) == 5
    # buffers that start at an odd pixel: the write-out goes pixel by pixel
    td.fill_(7); tb.fill_(5)
    ctx.raster_mesh_depth_dev(tp.data_ptr(), tc.data_ptr(), w, h, far, off, 6, td.data_ptr() + 2, tb.data_ptr() + 1, s.cuda_stream)
    s.synchronize()
    assert np.array_equal(td[1:].cpu().numpy().view(np.uint16).reshape(6, h, w), want) and int(td[0]) == 7
    assert np.array_equal(tb[1:].cpu().numpy().reshape(6, h, w), wbody) and int(tb[0]) == 5


def test_raster_mesh_then_track_on_one_stream(weights):
    """ht_raster_mesh_depth_dev then ht_update_frames_dev on one stream equals update_frames_sync on the downloaded frames"""
    from hand_tracking_samples_amd import native
    z = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
    n = 4
    poses = z["gtpose"][[3, 200, 470, 900]].astype(np.float32); start = z["startpose"][[3, 200, 470, 900]].astype(np.float32)
    cams = np.tile(QVGA_CAM, (n, 1))
    ctx = native.Context(MODELS[17], n)
    try:
        ctx.load_weights(weights)
        ctx.set_params(microforce=3.0, mainthreadpasses=3)
        dev = torch.device("cuda:0")
        tp = torch.from_numpy(poses).to(dev); tc = torch.from_numpy(cams).to(dev); ts = torch.from_numpy(start).to(dev)
        td = torch.empty((n, 240, 320), dtype=torch.int16, device=dev); out = torch.empty((n, 17, 7), dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        ctx.raster_mesh_depth_dev(tp.data_ptr(), tc.data_ptr(), 320, 240, 4.0, 0.0, n, td.data_ptr(), None, s.cuda_stream)
        ctx.update_frames_dev(td.data_ptr(), tc.data_ptr(), 320, 240, 0.17, ts.data_ptr(), n, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        frames = td.cpu().numpy().view(np.uint16)
        got = out.cpu().numpy()
        assert (frames < 3999).any()
        assert np.array_equal(frames, ctx.raster_mesh_depth(poses, cams, 320, 240, 4.0, 0.0))
        ctx.tracker_reset(start)
        want = ctx.update_frames_sync(frames, cams, 0.17)
        assert np.array_equal(got, want)
    finally:
        ctx.close()


def test_after_scale_device_equals_a_host_model_scaled_alike():
    from hand_tracking_samples_amd import native
    ctx = native.Context(MODELS[17], 1); m = native.HostModel(MODELS[17])
    try:
        ctx.scale(1.15); m.scale(1.15)
        p = _six(17, 6)[[0]]; cams = _cams(64, 48, 1)
        want, wbody = _equal(ctx, m, p, cams, 64, 48, 4.0, 0.5)
        assert (wbody >= 0).any()
    finally:
        m.close(); ctx.close()


def test_refusals_and_b0(pair):
    nb, ctx, m = pair
    p = _six(nb, 3)[[0]].copy(); p[:, :, 2] -= 10.0
    got, body = ctx.raster_mesh_depth(p, QVGA_CAM[None], 100, 75, 0.85, 0.5, want_body=True)
    assert (got == np.uint16(int(np.float32(0.85) / np.float32(0.001)))).all() and (body == -1).all()
    empty = ctx.raster_mesh_depth(np.zeros((0, nb, 7), np.float32), np.zeros((0, 12), np.float32), 320, 240)
    assert empty.shape == (0, 240, 320)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    d = np.full((1, 8, 8), 9, np.uint16); dp = d.ctypes.data_as(C.POINTER(C.c_uint16)); c = QVGA_CAM[None].copy()
    assert ctx.L.ht_raster_mesh_depth(ctx.h, fp(p), fp(c), 8, 8, 4.0, 0.0, 0, dp, None) == 0 and (d == 9).all()      # B = 0 does nothing
    assert ctx.L.ht_raster_mesh_depth_dev(ctx.h, 256, 256, 8, 8, 4.0, 0.0, 0, 256, None, None) == 0
    for w, h, far, off, B in ((0, 8, 4.0, 0.0, 1), (8, 4097, 4.0, 0.0, 1), (8, 8, -2.0, 0.0, 1), (8, 8, 4.0, float("nan"), 1), (8, 8, 4.0, 1.25, 1), (8, 8, 4.0, 0.0, -1)):
        rc = ctx.L.ht_raster_mesh_depth(ctx.h, fp(p), fp(c), w, h, far, off, B, dp, None)
        assert rc == 1 and rc == ctx.L.ht_render_mesh_depth(ctx.h, fp(p), fp(c), w, h, far, off, B, dp, None)
        assert ctx.L.ht_raster_mesh_depth_dev(ctx.h, 256, 256, w, h, far, off, B, 256, None, None) == 1
    assert ctx.L.ht_raster_mesh_depth(ctx.h, None, fp(c), 8, 8, 4.0, 0.0, 1, dp, None) == 1
    assert ctx.L.ht_raster_mesh_depth(ctx.h, fp(p), None, 8, 8, 4.0, 0.0, 1, dp, None) == 1
    assert ctx.L.ht_raster_mesh_depth(ctx.h, fp(p), fp(c), 8, 8, 4.0, 0.0, 1, None, None) == 1
    assert (d == 9).all()


def test_pose_mesh_residual_is_raster_then_depth_compare(pair):
    """ht_pose_mesh_residual on four 64x48 frames: the rendered frames are the rasteriser's at pixel offset 0, the figures ht_depth_compare's on them; the _dev form agrees"""
    nb, ctx, m = pair
    w, h, far, lo, hi, tol = 64, 48, 4.0, 1, 3999, 12
    poses = _six(nb, 3)[[0, 1, 2, 5]]; cams = _cams(w, h, 4)
    observed = ctx.render_depth(poses, cams, w, h, far)      # the hulls' frames stand for a camera's
    got = ctx.pose_mesh_residual(poses, cams, observed, lo, hi, tol, far, com_poses=True, want_rendered=True)
    frames = ctx.raster_mesh_depth(poses, cams, w, h, far, 0.0)
    assert (frames < 3999).any() and np.array_equal(got["rendered"], frames)
    want = ctx.depth_compare(observed, frames, lo, hi, tol, cams[:, 4])
    assert np.array_equal(got["info"], want["info"]) and (got["info"][:, 2] > 0).any() and (got["info"][:, 6] > 0).any()
    assert np.array_equal(ctx.pose_mesh_residual(poses, cams, observed, lo, hi, tol, far, com_poses=True)["info"], want["info"])      # rendered into the context's own buffer
    assert not np.array_equal(ctx.pose_depth_residual(poses, cams, observed, lo, hi, tol, far, com_poses=True)["info"], want["info"])      # the hull form is another renderer
    dev = torch.device("cuda:0")
    tp = torch.from_numpy(poses).to(dev); tc = torch.from_numpy(cams).to(dev); to = torch.from_numpy(observed.view(np.int16)).to(dev)
    ti = torch.full((4, 8), -1, dtype=torch.int64, device=dev); tr = torch.full((4, h, w), 7, dtype=torch.int16, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    ctx.pose_mesh_residual_dev(tp.data_ptr(), tc.data_ptr(), to.data_ptr(), w, h, 4, lo, hi, tol, ti.data_ptr(), tr.data_ptr(), far, True, s.cuda_stream)
    s.synchronize()
    assert np.array_equal(ti.cpu().numpy(), want["info"]) and np.array_equal(tr.cpu().numpy().view(np.uint16), frames)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    info = np.zeros((4, 8), np.int64)
    args = (w, h, 4, 0, far, lo, hi, tol, info.ctypes.data_as(C.POINTER(C.c_int64)), None)
    assert ctx.L.ht_pose_mesh_residual(ctx.h, None, fp(cams), observed.ctypes.data_as(C.POINTER(C.c_uint16)), *args) == 1
    assert ctx.L.ht_pose_mesh_residual(ctx.h, fp(poses), fp(cams), observed.ctypes.data_as(C.POINTER(C.c_uint16)), w, h, 4, 2, far, lo, hi, tol, info.ctypes.data_as(C.POINTER(C.c_int64)), None) == 1


def test_cnn_only_context_is_refused():
    from hand_tracking_samples_amd import native
    ctx = native.Context(None, 1)
    try:
        p = np.zeros((1, 17, 7), np.float32); d = np.zeros((1, 8, 8), np.uint16); c = QVGA_CAM[None].copy()
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        assert ctx.L.ht_raster_mesh_depth(ctx.h, fp(p), fp(c), 8, 8, 4.0, 0.0, 1, d.ctypes.data_as(C.POINTER(C.c_uint16)), None) == 4      # HT_ERR_STATE
        assert ctx.L.ht_raster_mesh_depth_dev(ctx.h, 256, 256, 8, 8, 4.0, 0.0, 1, 256, None, None) == 4
    finally:
        ctx.close()
