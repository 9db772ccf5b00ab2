"""The input frames of the sensor-filter tests (tests/test_sensor_ref.py pins their properties, tests/test_gpu_sensor.py runs the device on them).

FilterDS4's flying-pixel pass rewrites the frame while it walks it, so these frames are made to let early verdicts decide late ones: on every one of them
a kernel that read all neighbours as pass 1 left them (`naive_ds4`) gets at least 5 % of the interior wrong, while at least 10 % of it survives."""
import numpy as np


def cascade_rows(w, h):
    """every row 1000 + (0, 12, 0)[x % 3], bright IR: pixel x survives or not depending on its two left neighbours' fates, all the way along the row"""
    row = np.array([1000 + (0, 12, 0)[x % 3] for x in range(w)], np.uint16)
    return np.tile(row, (h, 1)), np.full((h, w), 200, np.uint8)


def cascade_cols(w, h):
    """the transposed frame: every column 1000 + (0, 12, 0)[y % 3]"""
    d, ir = cascade_rows(h, w)
    return np.ascontiguousarray(d.T), np.ascontiguousarray(ir.T)


def _noise(rng, d, ir):
    """3 % random pixels, 5 % dark in IR"""
    h, w = d.shape
    hit = rng.random((h, w)) < 0.03
    d = np.where(hit, rng.integers(0, 4200, (h, w)), d).astype(np.uint16)
    ir = np.where(rng.random((h, w)) < 0.05, rng.integers(0, 8, (h, w)), ir).astype(np.uint8)
    return d, ir


def _trigger(ir):
    """a dark pixel at x = 2 of every other row: where a row's cascade starts"""
    ir[::2, 2] = 0
    return ir


def staircase(w, h, seed):
    """a staircase that climbs through 4096 (steps of 8 counts, six pixels wide, four rows high: a killed neighbour, 4096, counts as near for the values
    4087..4105) under one-pixel stripes 12 counts off, 3 % random pixels, 5 % dark IR"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    ph = int(rng.integers(0, 3))
    d = 4064 + 8 * (((x + int(rng.integers(0, 9))) // 6 + y // 4) % 8) + 12 * ((x + ph) % 3 == 1)
    d, ir = _noise(rng, d, np.full((h, w), 120, np.uint8))
    return d, _trigger(ir)


def blob(w, h, seed):
    """a blob with a steep rim and one-pixel stripes 12 counts off on a far wall, 3 % random pixels, 5 % dark IR: the stripes' neighbours live on their
    already-visited neighbours"""
    rng = np.random.default_rng(1000 + seed)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    cx, cy, r = w * (0.35 + 0.3 * rng.random()), h * (0.35 + 0.3 * rng.random()), 0.40 * max(w, h)
    rr = np.hypot(x - cx, (y - cy) * w / h)
    ph = int(rng.integers(0, 3))
    d = np.where(rr < r, 600 + (rr * rr * (7.0 / r)).astype(np.int64) + 12 * ((x + ph) % 3 == 1), 3000 + 3 * ((x + y) % 5))
    d, ir = _noise(rng, d, np.full((h, w), 90, np.uint8))
    return d, _trigger(ir)


FAMILIES = {"staircase": staircase, "blob": blob}
DIFFER_MIN, KEPT_MIN = 0.05, 0.10      # what every frame with an interior must show (tests/test_sensor_ref.py)


def judge(depth, ir):
    """(fraction of the interior the naive form gets wrong, fraction of the interior the restatement keeps)"""
    import sensor_ref
    h, w = depth.shape
    ref, nv = sensor_ref.filter_ds4(depth, ir, max_width=w), naive_ds4(depth, ir)
    n = (h - 4) * (w - 4)
    return float((ref[2:-2, 2:-2] != nv[2:-2, 2:-2]).sum()) / n, float((ref[2:-2, 2:-2] != 4096).sum()) / n


def batch(family, w, h, B, seed0=0):
    """B distinct frames of a family, (depth u16 [B, h, w], ir u8 [B, h, w]): the first B seeds from seed0 on whose frame meets the condition with a margin
    (a frame without an interior is taken as it comes)"""
    D, I, seed = [], [], seed0
    while len(D) < B:
        if seed - seed0 > 8 * B + 64:
            raise ValueError("the %s family does not meet the condition at %dx%d" % (family, w, h))
        d, ir = FAMILIES[family](w, h, seed)
        seed += 1
        if h > 4 and w > 4:
            differ, kept = judge(d, ir)
            if differ < DIFFER_MIN + 0.01 or kept < KEPT_MIN + 0.02:
                continue
        D.append(d); I.append(ir)
    return np.stack(D), np.stack(I)


def background_for(depth, seed):
    """a background model near the frames' own values, so that pass 3 drops some pixels and keeps others"""
    rng = np.random.default_rng(77 + seed)
    return (depth.astype(np.int64) + rng.integers(-6, 20, depth.shape)).clip(0, 65535).astype(np.uint16)


def naive_ds4(depth, ir):
    """the WRONG parallel form: pass 2 with every neighbour read as pass 1 left it (vectorised).  Only the inputs are judged with it."""
    h, w = depth.shape
    p = np.where((depth < 30) | (ir < 8), 4096, depth).astype(np.int64)
    out = p.copy()
    if h > 4 and w > 4:
        c = p[2:-2, 2:-2]

        def has(a, b):
            return (np.abs(a - c) < 10) | (np.abs(b - c) < 10)

        ok = has(p[2:-2, 3:-1], p[2:-2, 1:-3]) & has(p[3:-1, 2:-2], p[1:-3, 2:-2]) & has(p[2:-2, 4:], p[2:-2, :-4]) & has(p[4:, 2:-2], p[:-4, 2:-2])
        out[2:-2, 2:-2] = np.where(ok, c, 4096)
    return out.astype(np.uint16)
