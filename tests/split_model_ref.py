"""Two hands that touch or cross in numpy (include/ht_mi355x.h "two hands that touch or cross"): the definition ht_split_hands_model and
ht_update_two_hands_model_* are held to.  The distances come from the oracle's ho_closest (independent C, pinned to the reference) on an oracle model set to the prior
poses; the blob part and the frame writer are split_ref's, mirroring is mirror_ref's.  No code is shared with the kernels."""
import ctypes as C
import os

import numpy as np

import mirror_ref
import oracle_lib as ol
import split_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
ALWAYS, MERGED = 0, 1
RIGHT_IS_LOW_X, MIRROR_LEFT, USER_POSES = 1, 2, 4
NONE = 0xFFFF
MODEL17 = os.path.join(HERE, "golden", "model_hand17.htfx")
F = np.float32


def first_min(depth):
    """depth u16 [h,w] -> (Q [H4,W4], x* [H4,W4], y* [H4,W4]): the minimum of every 4x4 block and the first pixel of the block, in raster order, that attains it"""
    h, w = depth.shape
    blocks = depth.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(h // 4, w // 4, 16)
    at = blocks.argmin(axis=2)      # numpy's argmin returns the first occurrence
    Y, X = np.indices(at.shape)
    return blocks.min(axis=2), 4 * X + at % 4, 4 * Y + at // 4


def cell_point(x, y, Q, cam):
    """deprojectz((x, y), (float)Q * depth_scale) in the expression order of misc_image.h:48, one float32 operation after another"""
    fx, fy, cx, cy, ds = (F(c) for c in cam[:5])
    d = F(Q) * ds
    return np.array([((F(x) - cx) / fx) * d, ((F(y) - cy) / fy) * d, F(1.0) * d], F)


def _qrot(q, v):
    """linalg.h:284-288: qxdir(q) * v.x + qydir(q) * v.y + qzdir(q) * v.z in float32"""
    x, y, z, w = (F(c) for c in q)
    two = F(2)
    xd = np.array([w * w + x * x - y * y - z * z, (x * y + z * w) * two, (z * x - y * w) * two], F)
    yd = np.array([(x * y - z * w) * two, w * w - x * x + y * y - z * z, (y * z + x * w) * two], F)
    zd = np.array([(z * x + y * w) * two, (y * z - x * w) * two, w * w - x * x - y * y + z * z], F)
    return (xd * F(v[0]) + yd * F(v[1])) + zd * F(v[2])


def prior_poses(poses2, com, flags, left_canonical=False):
    """poses2 [2][nb][7] (right; left in real space) -> the centre-of-mass poses both oracle models are set to: the left one mirrored into canonical space, then,
    with USER_POSES, pos += qrot(q, com[b])"""
    out = np.array(poses2, F, copy=True)
    if not left_canonical:
        out[1] = mirror_ref.poses(out[1][None])[0]
    if flags & USER_POSES:
        for k in range(2):
            for b in range(out.shape[1]):
                out[k, b, :3] = out[k, b, :3] + _qrot(out[k, b, 3:], com[b])
    return out


class Closest:
    """ho_closest against two oracle models (0: the right prior, 1: the canonical left prior)"""

    def __init__(self, model=None):
        import htfx
        self.path = model or MODEL17
        self.o = ol.Oracle(model=self.path)
        self.com = htfx.load(self.path)["body_f"][:, 7:10].astype(F)
        self.nb = self.o.nb

    def close(self):
        self.o.close()

    def set(self, canon2):
        for k in range(2):
            self.o.L.ho_set_pose(self.o.h, k, ol.fptr(np.ascontiguousarray(canon2[k], F)))

    def dist(self, k, v):
        """dot(closest(model k, v), (v, 1)) in float32, the order of linalg.h:262"""
        p = ol.F4()
        self.o.L.ho_closest(self.o.model(k), ol.v3(v), C.byref(p))
        return ((F(p.x) * v[0] + F(p.y) * v[1]) + F(p.z) * v[2]) + F(p.w) * F(1)


def assign(depth, cam, canon2, closest, range_lo, range_hi, max_dist):
    """one frame -> (labels u16 [H4,W4] of 0 / 1 / 0xFFFF, dist f32 [H4,W4,2])"""
    Q, xs, ys = first_min(depth)
    H4, W4 = Q.shape
    lab = np.full((H4, W4), NONE, np.uint16); dist = np.full((H4, W4, 2), np.inf, F)
    closest.set(canon2)
    md = F(max_dist)
    for Y in range(H4):
        for X in range(W4):
            q = int(Q[Y, X])
            if not range_lo <= q < range_hi:
                continue
            v = cell_point(xs[Y, X], ys[Y, X], q, cam)
            dR = closest.dist(0, v)
            dL = closest.dist(1, np.array([-v[0], v[1], v[2]], F))
            dist[Y, X] = (dR, dL)
            if (dL if dL < dR else dR) > md:
                continue
            lab[Y, X] = 0 if dR <= dL else 1
    return lab, dist


def split(depth, cams, poses, range_lo, range_hi, far, closest, max_dist=np.inf, mode=ALWAYS, max_step=65535, min_pixels=1, flags=0, left_canonical=False):
    """depth u16 [B,h,w], cams [B,12], poses [B,2,nb,7] -> dict(frames, cams, info, n_components, source, dist, labels) as ht_split_hands_model writes them"""
    depth = np.asarray(depth, np.uint16); cams = np.asarray(cams, F).reshape(-1, 12); poses = np.asarray(poses, F)
    B, h, w = depth.shape
    assert not (max_dist != max_dist) and max_dist >= 0 and mode in (ALWAYS, MERGED) and not flags & ~7 and not (mode == ALWAYS and flags & RIGHT_IS_LOW_X)
    blob = S.split(depth, range_lo, range_hi, far, max_step=max_step, min_pixels=min_pixels, flags=flags & 3, cams=cams)
    frames = blob["frames"].copy(); info = blob["info"].copy(); n = blob["n_components"].copy(); labels = blob["labels"].copy()
    source = np.zeros(B, np.int32); dist = np.full((B, h // 4, w // 4, 2), np.inf, F)
    for b in range(B):
        if mode == MERGED and n[b] >= 2:
            continue
        lab, dist[b] = assign(depth[b], cams[b], prior_poses(poses[b], closest.com, flags, left_canonical), closest, range_lo, range_hi, max_dist)
        comps = S.components(lab)
        present = [k in comps and comps[k]["count"] >= min_pixels for k in (0, 1)]
        if mode == MERGED and not all(present):
            continue
        source[b] = 1; labels[b] = lab
        if mode == ALWAYS:
            n[b] = sum(present)
        big = np.repeat(np.repeat(lab, 4, axis=0), 4, axis=1)
        for k in (0, 1):
            frame = np.full((h, w), far, np.uint16)
            info[b, k] = 0; info[b, k, 1] = NONE
            if present[k]:
                c = comps[k]
                info[b, k] = (c["count"], k, c["sum_x"], c["sum_y"], c["min_x"], c["min_y"], c["max_x"], c["max_y"])
                frame = np.where(big == k, depth[b], np.uint16(far))
            frames[b, k] = mirror_ref.frames(frame[None])[0] if k == 1 and flags & MIRROR_LEFT else frame
    return dict(frames=frames, cams=blob["cams"], info=info, n_components=n, source=source, dist=dist, labels=labels)


# ---- the touching scene: section 27's scene with the hands' lateral offset reduced in 5 mm steps until the blob split first reports one component ------------------
def scene_poses_at(k, shift):
    P = S.scene_poses(k)
    P[0, :, 0] += F(shift) - F(S.SCENE_SHIFT); P[1, :, 0] -= F(shift) - F(S.SCENE_SHIFT)
    return P


def compose(solo_right, solo_left):
    """the nearer of two solo frames per pixel, and per cell which solo frame supplied Q (0 right, 1 left, 0xFFFF background; a tie to the right)"""
    both = np.minimum(solo_right, solo_left)
    qr, ql = S.quarter(solo_right), S.quarter(solo_left)
    truth = np.where(np.minimum(qr, ql) >= S.SCENE_HI, NONE, np.where(qr <= ql, 0, 1)).astype(np.uint16)
    return both, truth


def mislabelled(labels, truth):
    """(wrong, foreground): cells whose label differs from the truth among the truth's foreground cells"""
    fg = truth != NONE
    return int((labels[fg] != truth[fg]).sum()), int(fg.sum())
