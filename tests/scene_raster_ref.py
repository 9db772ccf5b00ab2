"""The scene rasteriser's definition (ht_model_raster_scene, include/ht_mi355x.h) restated in numpy on top of mesh_raster_ref.render and
mirror_ref: the layer of every instance, a left one from its mirrored pose through the mirrored principal point and read at the flipped column, the smallest
count per pixel with the lowest instance on equal counts, over the background frame.  With a float32 mesh it must equal the host bit for bit."""
import numpy as np

import mesh_raster_ref
import mirror_ref

RIGHT, LEFT, ABSENT, MAX_HANDS = 0, 1, 255, 4


def mirror_px(cx, w, off):
    """cx' = ((float)(w-1) - cx) + (off + off) in float32, the second addition skipped at off 0 (then ht_mirror_cams' bits)"""
    m = np.float32(w - 1) - np.float32(cx)
    o = np.float32(off)
    return m if o == 0 else np.float32(m + np.float32(o + o))


def layer(mesh, pose, flag, cam, w, h, far, off):
    """(count [h,w] int64, body [h,w]) of one instance, in the scene's columns; body -1 where the layer does not cover"""
    cam = np.array(cam, np.float32)
    left = flag != RIGHT
    if left:
        pose = mirror_ref.poses(pose)
        cam[2] = mirror_px(cam[2], w, off)
    d, b, _ = mesh_raster_ref.render(mesh, pose, cam, w, h, far, off)
    if left:
        d, b = d[:, ::-1], b[:, ::-1]
    return d.astype(np.int64), b


def render(mesh, poses, hands, cam, w, h, far, off, bg=None):
    """one frame: dict of depth u16 [h,w], hand int8 [h,w], body int8 [h,w], visible int32 [H], and `layers` (the per-instance (count, body), None for an absent one)"""
    H = len(poses)
    assert 1 <= H <= MAX_HANDS
    flags = [RIGHT] * H if hands is None else [int(f) for f in hands]
    cnt = np.full((h, w), 65536, np.int64); inst = np.full((h, w), -1, np.int64); bod = np.full((h, w), -1, np.int64)
    layers = []
    for i in range(H):
        if flags[i] == ABSENT:
            layers.append(None)
            continue
        c, b = layer(mesh, poses[i], flags[i], cam, w, h, far, off)
        layers.append((c, b))
        better = (b >= 0) & (c < cnt)      # strictly: the lowest instance keeps a pixel on equal counts
        cnt[better] = c[better]; inst[better] = i; bod[better] = b[better]
    camf = np.asarray(cam, np.float32)
    none = np.uint16(int(np.float32(far) / camf[4]))
    under = np.full((h, w), none, np.uint16) if bg is None else np.asarray(bg, np.uint16).reshape(h, w)
    on = inst >= 0
    if bg is not None:
        on &= (under == 0) | (cnt <= under.astype(np.int64))
    depth = np.where(on, cnt, under.astype(np.int64)).astype(np.uint16)
    hand = np.where(on, inst, -1).astype(np.int8); body = np.where(on, bod, -1).astype(np.int8)
    visible = np.array([int((hand == i).sum()) for i in range(H)], np.int32)
    return dict(depth=depth, hand=hand, body=body, visible=visible, layers=layers)
