"""The mesh ray cast's definition (ht_model_hitcheck_mesh / ht_model_render_mesh, include/ht_mi355x.h) restated in numpy: every operation is a separate
numpy operation in one dtype, in the host's order (csrc/ht_math.hpp, geometric.h:247-273).  With dtype float32 it must equal the host bit for bit; with
float64 it is the geometric yardstick the float32 definition is measured against (the inputs stay the float32 corners, poses and camera)."""
import numpy as np


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _qmat(q):
    x, y, z, w = q
    two = x.dtype.type(2)
    X = [w * w + x * x - y * y - z * z, (x * y + z * w) * two, (z * x - y * w) * two]
    Y = [(x * y - z * w) * two, w * w - x * x + y * y - z * z, (y * z + x * w) * two]
    Z = [(z * x + y * w) * two, (y * z - x * w) * two, w * w - x * x - y * y + z * z]
    return X, Y, Z


def _mul(m, v):
    X, Y, Z = m
    return [(X[i] * v[0] + Y[i] * v[1]) + Z[i] * v[2] for i in range(3)]


def _det(a, b, c):
    """determinant(float3x3(a, b, c)), linalg.h:326 (a, b, c are the columns)"""
    return a[0] * (b[1] * c[2] - c[1] * b[2]) + a[1] * (b[2] * c[0] - c[2] * b[0]) + a[2] * (b[0] * c[1] - c[0] * b[1])


def planes(corners, dtype):
    """PolyPlane of every triangle: corners [t,3,3] -> [t,4]"""
    v = [[corners[:, i, k].astype(dtype) for k in range(3)] for i in range(3)]
    inv = dtype(1) / dtype(3)
    c = [np.zeros(len(corners), dtype) for _ in range(3)]
    for i in range(3):
        c = [c[k] + v[i][k] * inv for k in range(3)]
    n = [np.zeros(len(corners), dtype) for _ in range(3)]
    for i in range(3):
        x = _cross(_sub(v[i], c), _sub(v[(i + 1) % 3], c))
        n = [n[k] + x[k] for k in range(3)]
    zero = (n[0] == 0) & (n[1] == 0) & (n[2] == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt(_dot3(n, n))
        n = [n[k] / ln for k in range(3)]
        w = -_dot3(c, n)
    P = np.stack(n + [w], 1)
    P[zero] = 0
    return P


class Mesh:
    """corners: per body [t,3,3] float32 (ht_model_body_sdmesh), com: [nb,3] float32"""

    def __init__(self, corners, com, dtype):
        self.dtype = dtype
        self.corners = [c.astype(dtype) for c in corners]
        self.com = np.asarray(com).astype(dtype)
        self.planes = [planes(c, dtype) for c in corners]


def cast(mesh, poses, v0, v1):
    """segments v0 [n,3] -> v1 [n,3] against the bodies at poses [nb,7]: (impact [n,3], body [n], tri [n])"""
    dt = mesh.dtype
    poses = np.asarray(poses).astype(dt); v0 = np.asarray(v0).astype(dt); v1 = np.asarray(v1).astype(dt)
    n = len(v1)
    best = np.full(n, np.inf, dt); body = np.full(n, -1, np.int64); tri = np.full(n, -1, np.int64)
    impact = v1.copy()
    for b in range(len(mesh.corners)):
        pos = [poses[b, k] for k in range(3)]; q = [poses[b, 3 + k] for k in range(4)]
        R = _qmat(q)
        up = _sub(pos, _mul(R, [mesh.com[b, k] for k in range(3)]))
        qc = [-q[0], -q[1], -q[2], q[3]]
        Ri = _qmat(qc)
        invp = _mul(Ri, [-up[0], -up[1], -up[2]])
        a = [(invp[k] + _mul(Ri, [v0[:, 0], v0[:, 1], v0[:, 2]])[k])[:, None] for k in range(3)]      # [n,1]
        c = [(invp[k] + _mul(Ri, [v1[:, 0], v1[:, 1], v1[:, 2]])[k])[:, None] for k in range(3)]
        P = mesh.planes[b]; T = mesh.corners[b]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            d0 = ((P[None, :, 0] * a[0] + P[None, :, 1] * a[1]) + P[None, :, 2] * a[2]) + P[None, :, 3]      # [n,t]
            d1 = ((P[None, :, 0] * c[0] + P[None, :, 1] * c[1]) + P[None, :, 2] * c[2]) + P[None, :, 3]
            hit = (d0 > 0) & (d1 < 0)
            D = _sub(c, a)
            e = [[T[None, :, i, k] - a[k] for k in range(3)] for i in range(3)]
            for i in range(3):
                hit &= _det(e[(i + 1) % 3], e[i], D) >= 0
            t = np.where(hit, d0 / (d0 - d1), np.inf)
        k = np.argmin(t, 1)      # the first of equal minima
        tk = t[np.arange(n), k]
        win = tk < best
        if not win.any():
            continue
        best = np.where(win, tk, best); body[win] = b; tri[win] = k[win]
        i = np.nonzero(win)[0]
        d0w, d1w = d0[i, k[i]], d1[i, k[i]]
        aw = [a[x][i, 0] for x in range(3)]; cw = [c[x][i, 0] for x in range(3)]
        loc = [aw[x] + ((cw[x] - aw[x]) * d0w) / (d0w - d1w) for x in range(3)]
        wl = _mul(R, loc)
        for x in range(3):
            impact[i, x] = up[x] + wl[x]
    return impact, body, tri


def render(mesh, poses, cam, w, h, far, off):
    """one frame: (depth u16 [h,w], body [h,w], tri [h,w], impact z [h,w] in the mesh's dtype)"""
    dt = mesh.dtype
    cam = np.asarray(cam, np.float32).astype(dt)
    fx, fy, px, py, ds = (cam[k] for k in range(5))
    F, o = dt(np.float32(far)), dt(np.float32(off))
    ys, xs = np.mgrid[0:h, 0:w]
    x = xs.ravel().astype(dt); y = ys.ravel().astype(dt)
    v1 = np.stack([((x + o) - px) / fx * F, ((y + o) - py) / fy * F, np.full(len(x), F, dt)], 1)
    impact, body, tri = cast(mesh, poses, np.zeros_like(v1), v1)
    z = impact[:, 2] / ds
    return z.astype(np.int64).astype(np.uint16).reshape(h, w), body.reshape(h, w), tri.reshape(h, w), z.reshape(h, w)
