"""Two hands in one frame in numpy (include/ht_mi355x.h "two hands in one frame"): the definition ht_split_hands and ht_update_two_hands_* are held
to.  All integers; the flood fill is a plain breadth-first search in raster order, so a component's label is the index it was first reached from: its smallest.
Mirroring comes from mirror_ref.  No code is shared with the kernels."""
import os
from collections import deque

import numpy as np

import mirror_ref

HERE = os.path.dirname(os.path.abspath(__file__))
RIGHT_IS_LOW_X, MIRROR_LEFT = 1, 2
NONE = 0xFFFF


def quarter(depth):
    """depth u16 [h,w] -> Q [h/4,w/4]: the minimum of every 4x4 block"""
    h, w = depth.shape
    return depth.reshape(h // 4, 4, w // 4, 4).min(axis=(1, 3))


def labels_of(Q, range_lo, range_hi, max_step):
    """Q u16 [H4,W4] -> labels u16 [H4,W4]: the smallest raster index of a cell's component, 0xFFFF for background"""
    H4, W4 = Q.shape
    q = Q.astype(np.int64)
    fg = (q >= range_lo) & (q < range_hi)
    lab = np.full((H4, W4), NONE, np.int64)
    for Y in range(H4):
        for X in range(W4):
            if not fg[Y, X] or lab[Y, X] != NONE:
                continue
            root = Y * W4 + X
            lab[Y, X] = root
            todo = deque([(Y, X)])
            while todo:
                y, x = todo.popleft()
                for v, u in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= v < H4 and 0 <= u < W4 and fg[v, u] and lab[v, u] == NONE and abs(int(q[y, x]) - int(q[v, u])) <= max_step:
                        lab[v, u] = root
                        todo.append((v, u))
    return lab.astype(np.uint16)


def components(lab):
    """{label: dict(count, sum_x, sum_y, min_x, min_y, max_x, max_y)} of a label image"""
    out = {}
    for l in np.unique(lab):
        if l == NONE:
            continue
        ys, xs = np.nonzero(lab == l)
        out[int(l)] = dict(count=len(xs), sum_x=int(xs.sum()), sum_y=int(ys.sum()), min_x=int(xs.min()), min_y=int(ys.min()), max_x=int(xs.max()), max_y=int(ys.max()))
    return out


def choose(comps, W4, min_pixels, flags):
    """-> (right label or None, left label or None, n_components)"""
    elig = sorted((l for l, c in comps.items() if c["count"] >= min_pixels), key=lambda l: (-comps[l]["count"], l))
    low = high = None
    if len(elig) >= 2:
        a, b = elig[0], elig[1]
        lhs, rhs = comps[a]["sum_x"] * comps[b]["count"], comps[b]["sum_x"] * comps[a]["count"]      # Python integers: exact
        a_lower = lhs < rhs or (lhs == rhs and a < b)
        low, high = (a, b) if a_lower else (b, a)
    elif len(elig) == 1:
        a = elig[0]
        if 2 * comps[a]["sum_x"] < comps[a]["count"] * (W4 - 1):
            low = a
        else:
            high = a
    right, left = (low, high) if flags & RIGHT_IS_LOW_X else (high, low)
    return right, left, len(elig)


def split(depth, range_lo, range_hi, far, max_step=65535, min_pixels=1, flags=0, cams=None):
    """depth u16 [B,h,w] -> dict(frames u16 [B,2,h,w], info i32 [B,2,8], n_components i32 [B], labels u16 [B,h/4,w/4], cams f32 [B,2,12] if cams is given)"""
    depth = np.asarray(depth, np.uint16)
    B, h, w = depth.shape
    assert w >= 8 and h >= 8 and w % 4 == 0 and h % 4 == 0 and (w // 4) * (h // 4) <= 19200
    assert range_lo < range_hi <= far and min_pixels >= 1 and not flags & ~3
    frames = np.full((B, 2, h, w), far, np.uint16); info = np.zeros((B, 2, 8), np.int32); n = np.zeros(B, np.int32); labels = np.empty((B, h // 4, w // 4), np.uint16)
    for b in range(B):
        lab = labels_of(quarter(depth[b]), range_lo, range_hi, max_step)
        labels[b] = lab
        comps = components(lab)
        right, left, n[b] = choose(comps, w // 4, min_pixels, flags)
        big = np.repeat(np.repeat(lab, 4, axis=0), 4, axis=1)
        for k, l in enumerate((right, left)):
            if l is None:
                info[b, k, 1] = NONE
                continue
            c = comps[l]
            info[b, k] = (c["count"], l, c["sum_x"], c["sum_y"], c["min_x"], c["min_y"], c["max_x"], c["max_y"])
            frames[b, k] = np.where(big == l, depth[b], np.uint16(far))
    out = dict(frames=frames, info=info, n_components=n, labels=labels)
    if flags & MIRROR_LEFT:
        frames[:, 1] = mirror_ref.frames(frames[:, 1])
    if cams is not None:
        c = np.repeat(np.asarray(cams, np.float32).reshape(B, 1, 12), 2, axis=1).copy()
        if flags & MIRROR_LEFT:
            c[:, 1] = mirror_ref.cams(c[:, 1], w)
        out["cams"] = c
    return out


# ---- the shapes the tests draw, as quarter images of 0 (background) and 1 (foreground), blown up to frames --------------------------------------------------------
def serpentine(W4, H4):
    """one component through every cell it has: full even rows joined alternately at the right and the left end"""
    m = np.zeros((H4, W4), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, H4 - 1, 2)):
        m[y, W4 - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(W4, H4):
    """one component: a path winding inwards, one background cell between its turns"""
    m = np.zeros((H4, W4), bool)
    inside = lambda x, y: 0 <= x < W4 and 0 <= y < H4
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = True
    while True:
        for _ in range(2):      # straight on while the cell after the next is free, else one turn to the right
            free = inside(x + dx, y + dy) and not m[y + dy, x + dx] and not (inside(x + 2 * dx, y + 2 * dy) and m[y + 2 * dy, x + 2 * dx])
            if free:
                break
            dx, dy = -dy, dx
        if not free:
            return m
        x, y = x + dx, y + dy
        m[y, x] = True


def frame_of(cells, far, rng=None):
    """a quarter image of depths (0 = background) -> a frame [4 H4, 4 W4] whose 4x4 blocks have their cell's depth as minimum: one pixel of a block holds it, the
    others (with rng) up to 2 units more"""
    cells = np.asarray(cells)
    H4, W4 = cells.shape
    out = np.repeat(np.repeat(np.where(cells > 0, cells, far).astype(np.uint16), 4, axis=0), 4, axis=1)
    if rng is not None:
        keep = np.zeros((H4, 4, W4, 4), bool)
        yy, xx = np.divmod(rng.integers(0, 16, (H4, W4)), 4)
        Y, X = np.indices((H4, W4))
        keep[Y, yy, X, xx] = True
        bumped = np.minimum(out.astype(np.int64) + rng.integers(0, 3, out.shape), far).astype(np.uint16)
        out = np.where(keep.reshape(out.shape), out, bumped)
    return out


# ---- the rendered two-hand scene of tests/test_gpu_split.py: its separation condition is checked on the host by tests/test_split_ref.py ----------------------------
SCENE_W, SCENE_H, SCENE_SHIFT = 320, 240, 0.09
SCENE_HI, SCENE_MIN_PIXELS = 650, 50      # foreground nearer than 0.65 m (HandSegmentVR's wrange.y); blobs of at least 50 cells
SCENES = (0, 300)      # the poses the scenes are made of
SCENE_FAR = 3999       # what both renderers write where nothing is hit: (uint16)(4.0f / 0.001f) in fp32
SCENE_CAM = np.array([305, 305, 160, 120, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)


def scene_poses(k):
    """centre-of-mass poses [2][nb][7] of scene k: a tracked hand of tests/golden/poses1024.htfx moved to the high-x side, and the mirror image of another moved to the low-x side"""
    import htfx
    P = htfx.load(os.path.join(HERE, "golden", "poses1024.htfx"))["other_pose"].astype(np.float32)
    right = P[k].copy(); left = mirror_ref.poses(P[(k + 341) % 1024][None])[0]
    right[:, 0] += np.float32(SCENE_SHIFT); left[:, 0] -= np.float32(SCENE_SHIFT)
    return np.stack([right, left])


def separable(solo_right, solo_left):
    """no foreground cell of one solo frame within one cell of a foreground cell of the other"""
    a = quarter(solo_right) < SCENE_HI; b = quarter(solo_left) < SCENE_HI
    grown = np.zeros_like(a)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            grown[max(dy, 0):a.shape[0] + min(dy, 0), max(dx, 0):a.shape[1] + min(dx, 0)] |= a[max(-dy, 0):a.shape[0] + min(-dy, 0), max(-dx, 0):a.shape[1] + min(-dx, 0)]
    return a.any() and b.any() and not (grown & b).any()
