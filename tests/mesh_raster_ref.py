"""The mesh rasteriser's definition (ht_model_raster_mesh, include/ht_mi355x.h) restated in numpy: every float operation is a separate numpy operation in one
dtype, in the host's order (csrc/ht_raster.hpp); the snapped screen coordinates, the facing and the coverage are exact int64.  With dtype float32 it must equal the
host bit for bit.  The mesh is a mesh_ray.Mesh, whose helpers this reuses."""
import numpy as np

from mesh_ray import _cross, _dot3, _mul, _qmat, _sub

NEAR = 0.01      # HT_RASTER_NEAR


def render(mesh, poses, cam, w, h, far, off):
    """one frame: (depth u16 [h,w], body [h,w], tri [h,w] -- the winner's index within its body, -1 for background)"""
    dt = mesh.dtype
    poses = np.asarray(poses).astype(dt)
    cam = np.asarray(cam, np.float32).astype(dt)
    fx, fy, px, py, ds = (cam[k] for k in range(5))
    F, o, near, snap = dt(np.float32(far)), dt(np.float32(off)), dt(np.float32(NEAR)), dt(256)
    cand = []      # per body: (pixel, count, body, triangle) of every candidate
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(len(mesh.corners)):
            pos = [poses[b, k] for k in range(3)]; q = [poses[b, 3 + k] for k in range(4)]
            R = _qmat(q)
            up = _sub(pos, _mul(R, [mesh.com[b, k] for k in range(3)]))
            T = mesh.corners[b]
            keep = np.ones(len(T), bool)
            W, X, Y = [], [], []
            for i in range(3):
                rv = _mul(R, [T[:, i, k] for k in range(3)])
                wi = [up[k] + rv[k] for k in range(3)]
                keep &= (wi[2] >= near) & np.isfinite(wi[0]) & np.isfinite(wi[1]) & np.isfinite(wi[2])
                sx = (fx * (wi[0] / wi[2]) + px) - o
                sy = (fy * (wi[1] / wi[2]) + py) - o
                keep &= (np.abs(sx) < 2.0 ** 20) & (np.abs(sy) < 2.0 ** 20)      # false for NaN
                W.append(wi)
                X.append(np.rint(np.where(keep, sx, 0) * snap).astype(np.int64)); Y.append(np.rint(np.where(keep, sy, 0) * snap).astype(np.int64))
            A2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
            keep &= A2 < 0
            N = _cross(_sub(W[1], W[0]), _sub(W[2], W[0]))
            k = _dot3(N, W[0])
            # the pixels whose samples lie in the corners' rectangle, clipped to the frame: the only ones the inclusive edge tests can pass
            x0 = np.maximum(-((-np.minimum(np.minimum(X[0], X[1]), X[2])) // 256), 0); x1 = np.minimum(np.maximum(np.maximum(X[0], X[1]), X[2]) // 256, w - 1)
            y0 = np.maximum(-((-np.minimum(np.minimum(Y[0], Y[1]), Y[2])) // 256), 0); y1 = np.minimum(np.maximum(np.maximum(Y[0], Y[1]), Y[2]) // 256, h - 1)
            keep &= (x0 <= x1) & (y0 <= y1)
            t = np.nonzero(keep)[0]
            if not len(t):
                continue
            bw = (x1 - x0 + 1)[t]; n = bw * (y1 - y0 + 1)[t]
            j = np.repeat(np.arange(len(t)), n)                       # one entry per (triangle, pixel of its rectangle)
            loc = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
            tj = t[j]
            x = x0[tj] + loc % bw[j]; y = y0[tj] + loc // bw[j]
            inside = np.ones(len(tj), bool)
            for i in range(3):
                i1 = (i + 1) % 3
                inside &= (X[i1][tj] - X[i][tj]) * (256 * y - Y[i][tj]) - (Y[i1][tj] - Y[i][tj]) * (256 * x - X[i][tj]) <= 0
            tj, x, y = tj[inside], x[inside], y[inside]
            rx = ((x.astype(dt) + o) - px) / fx; ry = ((y.astype(dt) + o) - py) / fy
            den = (N[0][tj] * rx + N[1][tj] * ry) + N[2][tj]
            z = k[tj] / den
            c = z / ds
            ok = np.isfinite(c) & (z >= near) & (z < F) & (c >= 0) & (c < 65536)
            cand.append((y[ok] * w + x[ok], c[ok].astype(np.int64), np.full(int(ok.sum()), b, np.int64), tj[ok]))
        bg = np.uint16(int(F / ds))
    depth = np.full(h * w, bg, np.uint16); body = np.full(h * w, -1, np.int64); tri = np.full(h * w, -1, np.int64)
    if cand:
        pix, cnt, bod, tr = (np.concatenate([c[i] for c in cand]) for i in range(4))
        order = np.lexsort((tr, bod, cnt, pix))      # by pixel, then count, then (body, triangle)
        first = order[np.concatenate([[True], pix[order][1:] != pix[order][:-1]])]
        depth[pix[first]] = cnt[first].astype(np.uint16); body[pix[first]] = bod[first]; tri[pix[first]] = tr[first]
    return depth.reshape(h, w), body.reshape(h, w), tri.reshape(h, w)
