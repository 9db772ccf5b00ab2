"""Two hands that touch or cross on the device: ht_split_hands_model against tests/split_model_ref.py bit for bit, ht_update_two_hands_model_*
against the calls it is defined by, and the touching scene, where the blob split loses a hand and the model split tracks both.

A model update is: split the frame by the tracked models (left hand mirrored), run the existing update on the 2B hand frames, mirror the odd slots' poses back.  So
ht_update_two_hands_model_sync must equal  ht_split_hands_model(HT_SPLIT_MIRROR_LEFT, priors = the slots' state) -> ht_update_frames_sized_sync -> mirror_ref  bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import htfx
import mirror_ref
import oracle_lib as ol
import split_model_ref as R
import split_model_scene as SC
import split_ref as S
from hand_tracking_samples_amd import native, weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAR, HI = 4000, 650
F = np.float32
KEYS = ("frames", "cams", "info", "n_components", "source", "dist", "labels")
# (mode, flags, max_dist, max_step, min_pixels): both modes, the mirror and the user-pose bit on and off, max_dist on and off
SETTINGS = [(R.ALWAYS, 0, np.inf, 65535, 1), (R.ALWAYS, R.MIRROR_LEFT | R.USER_POSES, 0.03, 65535, 3), (R.MERGED, R.MIRROR_LEFT | R.RIGHT_IS_LOW_X, np.inf, 65535, 2),
            (R.MERGED, R.USER_POSES, 0.05, 40, 1)]
W_, H_ = S.SCENE_W, S.SCENE_H
SPLIT = dict(range_lo=0, range_hi=S.SCENE_HI, far=S.SCENE_FAR, min_pixels=S.SCENE_MIN_PIXELS)


@pytest.fixture(scope="module")
def tracker():
    c = native.Context(ol.MODEL, 4)
    c.load_weights(W.make_cnnb()); c.set_params(microforce=3.0, mainthreadpasses=3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def closest():
    c = R.Closest()
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _same(got, want, what, keys=KEYS):
    for k in keys:
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k)


def _cam(w, h):
    """a camera whose frame spans about 0.5 m at 0.45 m: the blobs' cells land on and around the priors"""
    return np.array([0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0, 0.001, 0, 0, 0, 0, 0, 0, 1], F)


def _priors(rng, n, com=None):
    """n pairs of tracked hands of tests/golden/poses1024.htfx: one moved to the high-x side, the mirror image of another to the low-x side; with com: as user poses"""
    P = htfx.load(os.path.join(HERE, "golden", "poses1024.htfx"))["other_pose"].astype(F)
    out = []
    for _ in range(n):
        right = P[rng.integers(0, 1024)].copy(); left = P[rng.integers(0, 1024)].copy()
        right[:, 0] += F(rng.uniform(0.03, 0.07)); left[:, 0] += F(rng.uniform(0.03, 0.07))
        if com is not None:      # user pose = pose * (-com), physics.h:142, in canonical space; then the left one goes to real space
            for p in (right, left):
                for b in range(len(p)):
                    p[b, :3] = p[b, :3] - R._qrot(p[b, 3:], com[b])
        out.append(np.stack([right, mirror_ref.poses(left[None])[0]]))
    return np.stack(out)


def _frames(w, h, n, rng):
    """n distinct frames: the first one blob over the whole frame (depths 380 .. 520: the blob split sees one component, the models two hands), the others random blobs
    in and just out of range"""
    W4, H4 = w // 4, h // 4
    out = [S.frame_of(rng.integers(380, 520, (H4, W4)), FAR, rng)]
    for i in range(1, n):
        coarse = rng.random((H4 // 3 + 2, W4 // 3 + 2)) < 0.4 + 0.1 * i
        m = np.repeat(np.repeat(coarse, 3, axis=0), 3, axis=1)[:H4, :W4] ^ (rng.random((H4, W4)) < 0.08)
        out.append(S.frame_of(np.where(m, rng.integers(300, 700, (H4, W4)), 0), FAR, rng))
    return np.stack(out)


def _model_dev(ctx, d_in, in_off, d_cams, d_poses, w, h, B, mode, flags, max_dist, step, minpx, out_off, leave_out=()):
    """the device form into guarded buffers -> dict of host arrays; every output sits some bytes into an allocation filled with 0xA5; twice"""
    n = B * w * h; cells = B * (w // 4) * (h // 4)
    sizes = dict(frames=4 * n, cams=B * 96, info=B * 64, n_components=B * 4, source=B * 4, dist=8 * cells, labels=2 * cells)
    off = dict(frames=out_off, cams=16, info=16, n_components=16, source=16, dist=16, labels=16)
    buf = {k: torch.full((sizes[k] + 32,), 0xA5, dtype=torch.uint8, device=DEV) for k in sizes}
    torch.cuda.synchronize()
    ptr = lambda k: None if k in leave_out else buf[k].data_ptr() + off[k]
    got = None
    for _ in range(2):
        ctx.split_hands_model_dev(d_in.data_ptr() + in_off, d_cams.data_ptr(), d_poses.data_ptr(), w, h, B, 0, HI, step, minpx, FAR, max_dist, mode, flags, ptr("frames"), ptr("cams"), ptr("info"),
                                  ptr("n_components"), ptr("source"), ptr("dist"), ptr("labels"), None)
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in buf.items()}
        for k, v in host.items():
            used = 0 if k in leave_out else sizes[k]
            assert np.all(v[:off[k]] == 0xA5) and np.all(v[off[k] + used:] == 0xA5), ("written beside", k, in_off, out_off, leave_out)
        now = {k: v[off[k]:off[k] + sizes[k]] for k, v in host.items() if k not in leave_out}
        assert got is None or all(now[k].tobytes() == got[k].tobytes() for k in now)
        got = now
    return got


@pytest.mark.parametrize("w,h,B", [(8, 8, 1), (36, 20, 3), (76, 20, 3), (320, 240, 1), (320, 240, 3)])
def test_model_split_equals_the_restatement(tracker, closest, w, h, B):
    """Seeded blobs in front of seeded priors; the host form, the device form on aligned buffers and on views one pixel into an allocation, every optional output left
    out in turn."""
    rng = np.random.default_rng(w * 1000 + h * 10 + B)
    depth = _frames(w, h, B, rng)
    cams = np.repeat(_cam(w, h)[None], B, axis=0); cams[:, 2] += rng.integers(-2, 3, B).astype(F) / 4
    com_poses, user_poses = _priors(rng, B), _priors(rng, B, closest.com)
    n = depth.size
    d_in = torch.zeros(2 * n + 32, dtype=torch.uint8, device=DEV); d_in[:2 * n] = _dev(depth)
    d_in2 = torch.zeros(2 * n + 32, dtype=torch.uint8, device=DEV); d_in2[2:2 + 2 * n] = _dev(depth)
    d_cams = _dev(cams)
    sources = set()
    for mode, flags, max_dist, step, minpx in SETTINGS:
        poses = user_poses if flags & R.USER_POSES else com_poses
        want = R.split(depth, cams, poses, 0, HI, FAR, closest, max_dist=max_dist, mode=mode, max_step=step, min_pixels=minpx, flags=flags)
        sources |= set(want["source"].tolist())
        if mode == R.ALWAYS and max_dist == np.inf and w * h >= 100:
            assert (want["info"][:, :, 0] > 0).all()      # both hands take cells
        got = tracker.split_hands_model(depth, cams, poses, 0, HI, FAR, max_dist=max_dist, mode=mode, max_step=step, min_pixels=minpx, flags=flags, want_dist=True, want_labels=True)
        _same(got, want, ("host form", mode, flags))
        d_poses = _dev(poses)
        for src, in_off, out_off in ((d_in, 0, 0), (d_in, 0, 2), (d_in2, 2, 0)):
            raw = _model_dev(tracker, src, in_off, d_cams, d_poses, w, h, B, mode, flags, max_dist, step, minpx, out_off)
            for k in KEYS:
                assert raw[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), ("device form", k, in_off, out_off, mode, flags)
    assert (1 in sources or w * h < 100) and (0 in sources or B == 1)      # MERGED took the model for the one blob and left the blob split for the others
    # every optional output left out in turn: the others unchanged, nothing written into it
    mode, flags, max_dist, step, minpx = SETTINGS[2]
    want = R.split(depth, cams, com_poses, 0, HI, FAR, closest, max_dist=max_dist, mode=mode, max_step=step, min_pixels=minpx, flags=flags)
    d_poses = _dev(com_poses)
    for leave in (("cams",), ("n_components",), ("source",), ("dist",), ("labels",), ("cams", "n_components", "source", "dist", "labels")):
        raw = _model_dev(tracker, d_in, 0, d_cams, d_poses, w, h, B, mode, flags, max_dist, step, minpx, 0, leave_out=leave)
        for k in raw:
            assert raw[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), ("left out", leave, k)
    got = tracker.split_hands_model(depth, cams, com_poses, 0, HI, FAR, max_dist=max_dist, mode=mode, max_step=step, min_pixels=minpx, flags=flags, want_cams=False, want_n=False, want_source=False)
    assert sorted(got) == ["frames", "info"] and got["frames"].tobytes() == want["frames"].tobytes() and got["info"].tobytes() == want["info"].tobytes()


def test_the_26_bone_model():
    model = os.path.join(HERE, "golden", "model_hand26.htfx")
    c = native.Context(model, 2); cl = R.Closest(model)
    try:
        rest = htfx.load(model)["rest_state"][:, :7].astype(F)      # the hand along z, 0.12 .. 0.41 m
        right = rest.copy(); right[:, 0] += F(0.05)
        poses = np.stack([right, mirror_ref.poses(right[None])[0]])[None]
        rng = np.random.default_rng(26)
        depth = _frames(76, 20, 1, rng); cams = _cam(76, 20)[None]
        want = R.split(depth, cams, poses, 0, HI, FAR, cl, min_pixels=2, flags=R.MIRROR_LEFT)
        assert (want["info"][0, :, 0] > 20).all()
        _same(c.split_hands_model(depth, cams, poses, 0, HI, FAR, min_pixels=2, flags=R.MIRROR_LEFT, want_dist=True, want_labels=True), want, "26 bones")
    finally:
        c.close(); cl.close()


def test_the_hand_made_cases_on_the_device(tracker, closest):
    """the tie, max_dist at and one ulp below a cell's distance, the fallback of MERGED: the restatement's answers are written out in tests/test_split_model_ref.py"""
    P = SC.hand_made_priors()[None]; cam = SC.SMALL_CAM[None]

    def both(frame, cam=cam, **kw):
        kw.setdefault("mode", R.ALWAYS)
        want = R.split(frame[None], cam, P, 0, HI, FAR, closest, **kw)
        _same(tracker.split_hands_model(frame[None], cam, P, 0, HI, FAR, want_dist=True, want_labels=True, **kw), want, kw)
        return want

    tie_cam = cam.copy(); tie_cam[0, 2] = 4
    out = both(SC.small_frame({(4, 1): 430, (4, 6): 455, (1, 1): 430}), cam=tie_cam)
    assert out["dist"][0, 0, 1, 0] == out["dist"][0, 0, 1, 1] and out["labels"][0].tolist() == [[1, 0], [0xFFFF, 0]]
    frame = SC.small_frame({(1, 1): 380, (6, 2): 431})
    D = both(frame)["dist"][0, 0, 0].min()
    assert both(frame, max_dist=D)["labels"][0, 0].tolist() == [1, 0] and both(frame, max_dist=np.nextafter(D, F(0)))["labels"][0, 0].tolist() == [0xFFFF, 0]
    assert both(frame, max_dist=np.finfo(F).max)["labels"][0, 0].tolist() == [1, 0]
    full = np.full((8, 8), 430, np.uint16)
    assert both(full, mode=R.MERGED, min_pixels=2)["source"].tolist() == [1] and both(full, mode=R.MERGED, min_pixels=3)["source"].tolist() == [0]
    assert both(SC.small_frame({(6, 2): 431, (6, 6): 433}), mode=R.MERGED)["source"].tolist() == [0]
    assert both(SC.small_frame(SC.FOUR), min_pixels=3)["n_components"].tolist() == [0]
    swapped = tracker.split_hands_model(SC.small_frame(SC.FOUR)[None], cam, P[:, ::-1], 0, HI, FAR)
    assert swapped["frames"][0, ::-1].tobytes() == both(SC.small_frame(SC.FOUR))["frames"][0].tobytes()


# ---- the rendered scenes --------------------------------------------------------------------------------------------------------------------------------------
def _hull_solo(c, poses, cams):
    """[B][2][h][w] hull frames (ht_render_depth) of poses [B][2][nb][7]: the left hands' canonical poses through the mirrored camera, flipped"""
    B = len(poses)
    right = c.render_depth(poses[:, 0], cams, W_, H_, far=4.0)
    left = c.render_depth(mirror_ref.poses(poses[:, 1]), mirror_ref.cams(cams, W_), W_, H_, far=4.0)[:, :, ::-1]
    return np.ascontiguousarray(np.stack([right.reshape(B, H_, W_), left.reshape(B, H_, W_)], axis=1))


@pytest.fixture(scope="module")
def touching(tracker):
    """(b) B = 2: both scenes at the first 5 mm step at which the blob split of the composed hull frames reports one component (the premise, asserted here for the
    frames the device renders; tests/test_split_model_ref.py finds the same offset on the host)"""
    cams = np.repeat(S.SCENE_CAM[None], 2, axis=0)
    out = None
    for shift in (SC.TOUCH_SHIFT + SC.STEP, SC.TOUCH_SHIFT):
        poses = np.stack([R.scene_poses_at(k, shift) for k in S.SCENES])
        solo = _hull_solo(tracker, poses, cams)
        frames = np.minimum(solo[:, 0], solo[:, 1])
        n = tracker.split_hands(frames, **SPLIT)["n_components"]
        assert n.tolist() == ([2, 2] if shift > SC.TOUCH_SHIFT else [1, 1]), (shift, n)
        out = dict(poses=poses, solo=solo, frames=frames, cams=cams, truth=np.stack([R.compose(*s)[1] for s in solo]))
    return out


@pytest.fixture(scope="module")
def separable(tracker):
    """(a) section 27's scenes, mesh frames"""
    poses = np.stack([S.scene_poses(k) for k in S.SCENES])
    cams = np.repeat(S.SCENE_CAM[None], 2, axis=0)
    right = tracker.render_mesh_depth(poses[:, 0], cams, W_, H_, far=4.0).reshape(2, H_, W_)
    left = tracker.render_mesh_depth(mirror_ref.poses(poses[:, 1]), mirror_ref.cams(cams, W_), W_, H_, far=4.0).reshape(2, H_, W_)[:, :, ::-1]
    solo = np.ascontiguousarray(np.stack([right, left], axis=1))
    return dict(poses=poses, solo=solo, frames=np.minimum(solo[:, 0], solo[:, 1]), cams=cams)


def test_separable_scenes_split_into_their_solo_frames_also_with_crossed_priors(tracker, closest, separable):
    s = separable
    assert all(S.separable(*x) for x in s["solo"])
    for mode in (R.ALWAYS, R.MERGED):
        got = tracker.split_hands_model(s["frames"], s["cams"], s["poses"], mode=mode, want_dist=True, want_labels=True, **SPLIT)
        assert got["frames"].tobytes() == s["solo"].tobytes() and got["source"].tolist() == [1 - mode] * 2
        _same(got, R.split(s["frames"], s["cams"], s["poses"], 0, S.SCENE_HI, S.SCENE_FAR, closest, mode=mode, min_pixels=S.SCENE_MIN_PIXELS), ("separable", mode))
    crossed = tracker.split_hands_model(s["frames"], s["cams"], s["poses"][:, ::-1], **SPLIT)
    assert crossed["frames"].tobytes() == np.ascontiguousarray(s["solo"][:, ::-1]).tobytes()


def test_the_touching_scene_is_split_with_at_most_two_percent_of_its_cells_mislabelled(tracker, closest, touching):
    t = touching
    for mode in (R.ALWAYS, R.MERGED):
        got = tracker.split_hands_model(t["frames"], t["cams"], t["poses"], mode=mode, want_dist=True, want_labels=True, **SPLIT)
        _same(got, R.split(t["frames"], t["cams"], t["poses"], 0, S.SCENE_HI, S.SCENE_FAR, closest, mode=mode, min_pixels=S.SCENE_MIN_PIXELS), ("touching", mode))
        assert got["source"].tolist() == [1, 1] and (got["info"][:, :, 0] > 300).all()
        for b in range(2):
            wrong, fg = R.mislabelled(got["labels"][b], t["truth"][b])
            print("touching scene %d, mode %d: %d of %d foreground cells mislabelled (%.2f %%)" % (b, mode, wrong, fg, 100.0 * wrong / fg))
            assert fg > 800 and wrong <= 0.02 * fg


# ---- the update -----------------------------------------------------------------------------------------------------------------------------------------------
def _seed(poses):
    """the slots' starting poses [2B][nb][7]: canonical, so the left hands' mirrored"""
    B = len(poses)
    return mirror_ref.poses(poses.reshape(2 * B, -1, 7), np.arange(2 * B) % 2)


def _snapshot(c, n, poses, cnn):
    return dict(poses=poses.reshape(n, c.nb, 7), cnn=cnn, hand=c.get_state(0, n), other=c.get_state(1, n), err=c.tracker_flags(n)[0], init=c.tracker_flags(n)[1])


def _same_track(a, b, what):
    for k in a:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (what, k)


def _carried(c, B):
    """the slots' hand-model poses as the split call takes them: [B][2][nb][7], the left ones brought to real space (the mirror twice is the identity, bit for bit)"""
    st = np.ascontiguousarray(c.get_state(0, 2 * B)[:, :, :7])
    return mirror_ref.poses(st, np.arange(2 * B) % 2).reshape(B, 2, c.nb, 7)


@pytest.mark.parametrize("mode", [R.ALWAYS, R.MERGED])
def test_model_update_is_split_update_mirror(tracker, touching, mode):
    c, t = tracker, touching
    frames, cams, poses = t["frames"], t["cams"], t["poses"]
    B, n = 2, 4
    seed = _seed(poses)
    odd = (np.arange(n) % 2).astype(np.uint8)
    want, infos = [], []
    c.tracker_reset(seed)
    for _ in range(2):
        sp = c.split_hands_model(frames, cams, _carried(c, B), mode=mode, flags=R.MIRROR_LEFT, **SPLIT)
        assert sp["source"].tolist() == [1, 1]
        p, cnn = c.update_frames_sized_sync(sp["frames"].reshape(n, H_, W_), sp["cams"].reshape(n, 12), 64, 0.17, want_cnn=True)
        assert c.frames_overflow() == 0
        want.append(_snapshot(c, n, mirror_ref.poses(p, odd), cnn)); infos.append(sp["info"])
    assert np.isfinite(want[1]["poses"]).all() and want[0]["poses"].tobytes() != want[1]["poses"].tobytes()
    c.tracker_reset(seed)
    for u in range(2):
        p, info, source, cnn = c.update_two_hands_model(frames, cams, mode=mode, want_cnn=True, **SPLIT)
        assert c.frames_overflow() == 0 and info.tobytes() == infos[u].tobytes() and source.tolist() == [1, 1]
        _same_track(want[u], _snapshot(c, n, p, cnn), ("fused, update %d" % u, mode))
    # the device form, re-seeded through d_start_poses (the camera's space: the left hands' own poses), which are then the priors too
    c.tracker_reset(np.zeros_like(seed) + np.array([0, 0, 0, 0, 0, 0, 1], F))
    d_frames, d_cams, d_start = _dev(frames), _dev(cams), _dev(poses)
    d_out = torch.zeros(n * c.nb * 7, dtype=torch.float32, device=DEV); d_info = torch.zeros(B * 16, dtype=torch.int32, device=DEV); d_src = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    c.update_two_hands_model_dev(64, d_frames.data_ptr(), d_cams.data_ptr(), W_, H_, 0.17, 0, S.SCENE_HI, 65535, S.SCENE_MIN_PIXELS, S.SCENE_FAR, float("inf"), mode, 0, d_start.data_ptr(), B, d_out.data_ptr(),
                                 d_info.data_ptr(), d_src.data_ptr(), None)
    assert c.frames_overflow() == 0
    _same_track(want[0], _snapshot(c, n, d_out.cpu().numpy(), c.cnn_results(n)[1]), ("device form", mode))
    assert d_info.cpu().numpy().tobytes() == infos[0].tobytes() and d_src.cpu().tolist() == [1, 1]
    c.tracker_reset(seed)      # and without d_info, d_source and d_start_poses
    c.update_two_hands_model_dev(64, d_frames.data_ptr(), d_cams.data_ptr(), W_, H_, 0.17, 0, S.SCENE_HI, 65535, S.SCENE_MIN_PIXELS, S.SCENE_FAR, float("inf"), mode, 0, None, B, d_out.data_ptr(), None, None, None)
    assert c.frames_overflow() == 0
    _same_track(want[0], _snapshot(c, n, d_out.cpu().numpy(), c.cnn_results(n)[1]), ("device form, optional arguments left out", mode))


def test_merged_update_on_separable_scenes_is_the_blob_update(tracker, separable):
    c, s = tracker, separable
    seed = _seed(s["poses"])
    for flags in (0, R.RIGHT_IS_LOW_X):
        c.tracker_reset(seed)
        p0, info0, cnn0 = c.update_two_hands_sync(s["frames"], s["cams"], flags=flags, want_cnn=True, **SPLIT)
        a = _snapshot(c, 4, p0, cnn0)
        c.tracker_reset(seed)
        p1, info1, source, cnn1 = c.update_two_hands_model(s["frames"], s["cams"], mode=R.MERGED, flags=flags, want_cnn=True, **SPLIT)
        _same_track(a, _snapshot(c, 4, p1, cnn1), ("merged on separable scenes", flags))
        assert info0.tobytes() == info1.tobytes() and source.tolist() == [0, 0]


def test_touching_hands_are_both_tracked_where_the_blob_update_loses_one(tracker, touching):
    """The test that fails without the feature.  Each hand's mean HT_KP_SKELETON error against the truth may be at most twice that of the existing one-hand update on
    that hand's solo frame from the same start pose (the same code on a perfect split); both figures are printed and recorded."""
    c, t = tracker, touching
    frames, cams, poses, solo = t["frames"], t["cams"], t["poses"], t["solo"]
    seed = _seed(poses)
    odd = (np.arange(4) % 2).astype(np.uint8)
    c.tracker_reset(seed)
    _, info = c.update_two_hands_sync(frames, cams, **SPLIT)
    assert ((info[:, :, 0] == 0).sum(axis=1) == 1).all()      # the premise: one hand absent in either scene
    c.tracker_reset(seed)
    p, info, source = c.update_two_hands_model(frames, cams, mode=R.MERGED, **SPLIT)
    assert (info[:, :, 0] > 300).all() and source.tolist() == [1, 1]
    c.tracker_reset(seed)
    q = c.update_hands_sync(solo.reshape(4, H_, W_), np.repeat(cams, 2, axis=0), odd, 64, 0.17)      # the yardstick: every hand alone in its frame
    truth = c.keypoints(poses.reshape(4, c.nb, 7), table=native.KP_SKELETON, com_poses=True, hands=odd)["xyz"]
    err = lambda x: c.keypoint_errors(c.keypoints(x.reshape(4, c.nb, 7), table=native.KP_SKELETON, hands=odd)["xyz"], truth)["frame"][:, 0]
    model, alone = err(p), err(q)
    rec = {"scene": "two rendered hands of tests/golden/poses1024.htfx (rows %s), lateral offset %.3f m, 320x240, hull frames" % (list(S.SCENES), SC.TOUCH_SHIFT),
           "mean_skeleton_error_m": {"model_split_update": [float(x) for x in model], "one_hand_update_on_solo_frames": [float(x) for x in alone]}, "slots": "2i right, 2i + 1 left"}
    print(json.dumps(rec))      # (profiles/r24_two_hands_accuracy.json, "test_gpu_split_model", holds one run's figures)
    assert np.isfinite(model).all() and (model <= 2.0 * alone).all(), (model, alone)


def test_refusals_and_no_side_effects(tracker, touching, separable):
    c, t, s = tracker, touching, separable
    frames, cams, poses = t["frames"], t["cams"], t["poses"]
    seed = _seed(s["poses"])
    odd = (np.arange(4) % 2).astype(np.uint8)

    def existing():
        c.tracker_reset(seed)
        a = c.update_two_hands_sync(s["frames"], s["cams"], want_cnn=True, **SPLIT)
        c.tracker_reset(seed)
        b = c.update_hands_sync(s["solo"].reshape(4, H_, W_), np.repeat(s["cams"], 2, axis=0), odd, 64, 0.17, want_cnn=True)
        sp = c.split_hands(s["frames"], cams=s["cams"], want_labels=True, **SPLIT)
        return [x.tobytes() for x in a + b] + [sp[k].tobytes() for k in sorted(sp)] + [c.get_state(0, 4).tobytes(), c.get_state(1, 4).tobytes()]

    before = existing()
    good = c.split_hands_model(frames, cams, poses, **SPLIT)
    split_bad = ((dict(range_lo=650), "range_lo"), (dict(far=600), "far"), (dict(min_pixels=0), "min_pixels"), (dict(max_dist=float("nan")), "max_dist"), (dict(max_dist=-0.01), "max_dist"),
                 (dict(mode=2), "mode is"), (dict(mode=-1), "mode is"), (dict(flags=8), "flag"), (dict(flags=R.RIGHT_IS_LOW_X), "HT_SPLIT_RIGHT_IS_LOW_X"))
    for kw, msg in split_bad:
        with pytest.raises(native.HTError, match=msg):
            c.split_hands_model(frames, cams, poses, **dict(SPLIT, **kw))
        with pytest.raises(native.HTError, match=msg):
            c.update_two_hands_model(frames, cams, **dict(dict(SPLIT, mode=R.ALWAYS), **kw))
    with pytest.raises(native.HTError, match="flag"):
        c.update_two_hands_model(frames, cams, flags=R.USER_POSES, **SPLIT)      # the start poses also seed the slots: centre-of-mass poses only
    with pytest.raises(native.HTError, match="frame size"):
        c.split_hands_model(np.zeros((2, 66, 66), np.uint16), cams, poses, **SPLIT)
    u16 = lambda a: a.ctypes.data_as(native.C.POINTER(native.C.c_uint16)); fp = lambda a: a.ctypes.data_as(native.C.POINTER(native.C.c_float)); i32 = lambda a: a.ctypes.data_as(native.C.POINTER(native.C.c_int32))
    out = np.zeros((2, 2, H_, W_), np.uint16); info = np.zeros((2, 2, 8), np.int32)
    assert c.L.ht_split_hands_model(c.h, u16(frames), None, fp(poses), W_, H_, 2, 0, S.SCENE_HI, 65535, 50, S.SCENE_FAR, float("inf"), 0, 0, u16(out), None, i32(info), None, None, None, None) == 1      # cams is required
    assert not out.any() and not info.any()
    assert c.L.ht_split_hands_model(c.h, u16(frames), fp(cams), fp(poses), W_, H_, 0, 0, S.SCENE_HI, 65535, 50, S.SCENE_FAR, float("inf"), 0, 0, u16(out), None, i32(info), None, None, None, None) == 0 and not out.any()      # B = 0 does nothing
    three = np.repeat(frames[:1], 3, axis=0); cams3 = np.repeat(cams[:1], 3, axis=0)
    with pytest.raises(native.HTError, match="2 \\* B exceeds"):
        c.update_two_hands_model(three, cams3, **SPLIT)
    with pytest.raises(native.HTError, match="2 \\* B exceeds"):
        c.update_two_hands_model(frames[:0], cams[:0], **SPLIT)      # B = 0
    assert c.split_hands_model(three, cams3, np.repeat(poses[:1], 3, axis=0), **SPLIT)["frames"][2].tobytes() == good["frames"][0].tobytes()      # the split is not bounded by max_batch
    assert c.split_hands_model(frames, cams, poses, **SPLIT)["frames"].tobytes() == good["frames"].tobytes()      # the context still works
    assert existing() == before      # and the existing calls give the bytes they gave before any model-split call
    net = native.Context(None, 4)
    try:
        with pytest.raises(native.HTError, match="without a hand model.*status 4"):
            net.split_hands_model(frames, cams, poses, **SPLIT)
        with pytest.raises(native.HTError, match="without a hand model"):
            net.update_two_hands_model(frames, cams, **SPLIT)
    finally:
        net.close()


def test_cxx_split_model_example_runs_on_the_device(tmp_path):
    """SplitHandsByModel and TwoHandTracker::split_mode of include/ht_handtrack.hpp on one blob across the optical axis: the blob split loses a hand, the model split
    cuts the blob in two halves of 48 cells"""
    exe = str(tmp_path / "split_model"); cnnb = str(tmp_path / "w.cnnb")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_split_model_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    W.save_cnnb(cnnb, W.make_cnnb())
    r = subprocess.run([exe, ol.MODEL, cnnb], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "model split source 1 right 48 cells from 8 left 48 cells to 7 mirrored pixel 450" in r.stdout and "blob split components 1" in r.stdout
    assert "refused:" in r.stdout and "merged: source 1 right 48 left 48; always: source 1 right 48 left 48" in r.stdout and "update blobs: source 0" in r.stdout
