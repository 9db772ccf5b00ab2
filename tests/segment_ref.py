"""SampleD (misc_image.h:154-162) through a segment camera of side S, restated in float32 numpy: what HandSegmentVR (handtrack.h:342) does with the camera it has
built, for the 64x64 tile of the reference and for the 128x128 tile of the sized calls (ht_segment_vr_sized).

Every operation is a separate float32 numpy operation, so it rounds once, as the reference's build without contraction does; the order of the operations is that of
oracle/ho_math.h's qrot (the three rotated axes scaled and added left to right) and dot3 ((x*x + y*y) + z*z); the projections truncate like the C cast; a
pixel that falls outside the source gets the background (uint16)(4 / depth_scale).

The camera is the 12 floats of the C ABI: focal (2), principal (2), depth_scale, position (3), orientation quaternion xyzw (4).
"""
import numpy as np

F = np.float32


def side128_camera(cam64):
    """The side-128 segment camera of a side-64 one: dstcam = ({S,S}, avgdepth*S/diam, {S/2,S/2}) (handtrack.h:338-340) and S a power of two, so the focal
    doubles exactly, the principal point becomes (64,64) and the pose stays."""
    c = np.array(cam64, np.float32).copy()
    c[..., 0] = c[..., 0] * F(2); c[..., 1] = c[..., 1] * F(2); c[..., 2] = F(64); c[..., 3] = F(64)
    return c


def _qrot(q, vx, vy, vz):
    x, y, z, w = (F(v) for v in q)
    two = F(2)
    xd = (w * w + x * x - y * y - z * z, (x * y + z * w) * two, (z * x - y * w) * two)
    yd = ((x * y - z * w) * two, w * w - x * x + y * y - z * z, (y * z + x * w) * two)
    zd = ((z * x + y * w) * two, (y * z - x * w) * two, w * w - x * x - y * y + z * z)
    return tuple((xd[k] * vx + yd[k] * vy) + zd[k] * vz for k in range(3))


def sample_d(depth, cam, segcam, side):
    """depth u16[h,w] seen by `cam` [12] -> (tile u16[side,side] seen by `segcam` [12], the mask of tile pixels that fall outside the source)."""
    depth = np.ascontiguousarray(depth, np.uint16); h, w = depth.shape
    cam = np.asarray(cam, np.float32); segcam = np.asarray(segcam, np.float32)
    fx, fy, px, py, dscale = (F(v) for v in cam[:5])
    dfx, dfy, dpx, dpy = (F(v) for v in segcam[:4])
    q = segcam[8:12]
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        # ppdir = dstcam.pose * dstcam.deprojectz(dstcam.principal(), 1)
        pp = _qrot(q, ((dpx - dpx) / dfx) * one, ((dpy - dpy) / dfy) * one, one * one)
        pp = tuple(zero + v for v in pp)
        yy, xx = np.mgrid[0:side, 0:side]
        xx = xx.astype(np.float32); yy = yy.astype(np.float32)
        d = _qrot(q, ((xx - dpx) / dfx) * one, ((yy - dpy) / dfy) * one, np.full_like(xx, one) * one)
        d = tuple(zero + v for v in d)
        u = d[0] / d[2] * fx + px
        v = d[1] / d[2] * fy + py
        ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < F(2.0e9)) & (np.abs(v) < F(2.0e9))
        sx = np.where(ok, np.trunc(np.where(ok, u, zero)), -1).astype(np.int64)
        sy = np.where(ok, np.trunc(np.where(ok, v, zero)), -1).astype(np.int64)
        inside = ok & (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
        cx = np.clip(sx, 0, w - 1); cy = np.clip(sy, 0, h - 1)
        dd = depth[cy, cx].astype(np.float32)
        rx = ((cx.astype(np.float32) - px) / fx) * dd
        ry = ((cy.astype(np.float32) - py) / fy) * dd
        rz = one * dd
        val = (pp[0] * rx + pp[1] * ry) + pp[2] * rz
        background = np.uint16(int(F(4.0) / dscale))
        tile = np.where(inside, np.trunc(val).astype(np.int64) & 0xFFFF, background).astype(np.uint16)
    return tile, ~inside
