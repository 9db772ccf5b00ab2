"""Two rendered hands approach, touch and part: tracking through the sequence with TwoHandTracker's three ways of splitting a frame -- by blobs
(ht_update_two_hands_sync), by the tracked models where the blobs have merged (HT_SPLIT_MODEL_MERGED) and always by the models (HT_SPLIT_MODEL_ALWAYS).

The scenes are section 27's (two hands of tests/golden/poses1024.htfx, one mirrored), hull frames at 320x240; the lateral offset goes from 0.09 m down to --closest
(default 0.04 m) and back in 5 mm steps, the poses otherwise unchanged, so the truth of every frame is known.  Per mode and frame: presence of both hands, the share
of foreground cells whose label differs from the composition's ground truth (which solo frame supplied the cell's depth), and the mean and worst HT_KP_SKELETON error
per hand against the truth (ht_keypoint_errors).  No figure is promised: the table is the result.  Writes profiles/r24_two_hands_accuracy.json (or --out).

With --scene-render the scenes are drawn by ht_raster_scene_depth instead: both hands of a frame in one z-buffer pass on the subdivision surface the application draws
(DESIGN section 36), and the ground truth of a cell is the call's own hand label at the cell's nearest pixel.  Writes profiles/r27_two_hands_scene_accuracy.json (or --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mirror_ref  # noqa: E402
import split_model_ref as R  # noqa: E402
import split_ref as S  # noqa: E402
from hand_tracking_samples_amd import native, weights as W  # noqa: E402

W_, H_ = S.SCENE_W, S.SCENE_H
SPLIT = dict(range_lo=0, range_hi=S.SCENE_HI, far=S.SCENE_FAR, min_pixels=S.SCENE_MIN_PIXELS)
MODES = {"Blobs": None, "ModelWhenMerged": R.MERGED, "ModelAlways": R.ALWAYS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--closest", type=float, default=0.04, help="the smallest lateral offset of the sequence, metres")
    ap.add_argument("--scene-render", action="store_true", help="draw the scenes with ht_raster_scene_depth on the mesh surface (the default stays the composed hull frames)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r27_two_hands_scene_accuracy.json" if a.scene_render else "r24_two_hands_accuracy.json")
    steps = int(round((S.SCENE_SHIFT - a.closest) / 0.005))
    shifts = [S.SCENE_SHIFT - 0.005 * i for i in range(steps + 1)]
    shifts = shifts + shifts[-2::-1]
    B = len(S.SCENES); n = 2 * B
    odd = (np.arange(n) % 2).astype(np.uint8)
    cams = np.repeat(S.SCENE_CAM[None], B, axis=0)
    c = native.Context(os.path.join(ROOT, "tests", "golden", "model_hand17.htfx"), n)
    res = {"scenes": list(S.SCENES), "frame": ("%dx%d mesh frames of ht_raster_scene_depth" if a.scene_render else "%dx%d hull frames") % (W_, H_), "lateral_offsets_m": [round(x, 3) for x in shifts], "modes": {}}
    try:
        c.load_weights(W.make_cnnb()); c.set_params(microforce=3.0, mainthreadpasses=3)
        seq = []
        for shift in shifts:
            poses = np.stack([R.scene_poses_at(k, shift) for k in S.SCENES])
            if a.scene_render:      # one call: the frame and, per pixel, which hand it shows
                sc = c.raster_scene_depth(poses, cams, W_, H_, hands=np.tile(np.array([native.SCENE_RIGHT, native.SCENE_LEFT], np.uint8), (B, 1)), far=4.0, pixel_offset=0.0, want_body=False, want_visible=False)
                truth = []
                for b in range(B):
                    Q, xs, ys = R.first_min(sc["depth"][b])
                    truth.append(np.where(Q >= S.SCENE_HI, R.NONE, sc["hand"][b][ys, xs].astype(np.int64)).astype(np.uint16))
                seq.append(dict(poses=poses, frames=sc["depth"], truth=np.stack(truth), kp=c.keypoints(poses.reshape(n, c.nb, 7), table=native.KP_SKELETON, com_poses=True, hands=odd)["xyz"]))
                continue
            right = c.render_depth(poses[:, 0], cams, W_, H_, far=4.0).reshape(B, H_, W_)
            left = c.render_depth(mirror_ref.poses(poses[:, 1]), mirror_ref.cams(cams, W_), W_, H_, far=4.0).reshape(B, H_, W_)[:, :, ::-1]
            truth = np.stack([R.compose(right[b], left[b])[1] for b in range(B)])
            seq.append(dict(poses=poses, frames=np.minimum(right, left), truth=truth, kp=c.keypoints(poses.reshape(n, c.nb, 7), table=native.KP_SKELETON, com_poses=True, hands=odd)["xyz"]))
        for name, mode in MODES.items():
            c.tracker_reset(mirror_ref.poses(seq[0]["poses"].reshape(n, c.nb, 7), odd))
            rows = []
            for shift, f in zip(shifts, seq):
                # the labels the update is about to cut along: the same split on the slots' carried poses
                if mode is None:
                    sp = c.split_hands(f["frames"], want_labels=True, **SPLIT)
                    hand_of = [{int(sp["info"][b, k, 1]): k for k in (0, 1) if sp["info"][b, k, 0] > 0} for b in range(B)]
                    labels = np.stack([np.vectorize(lambda l, b=b: hand_of[b].get(int(l), R.NONE))(sp["labels"][b]).astype(np.uint16) for b in range(B)])
                    source = [0] * B
                else:
                    carried = mirror_ref.poses(np.ascontiguousarray(c.get_state(0, n)[:, :, :7]), odd).reshape(B, 2, c.nb, 7)
                    sp = c.split_hands_model(f["frames"], cams, carried, mode=mode, want_labels=True, **SPLIT)
                    labels = sp["labels"].copy()
                    for b in range(B):
                        if sp["source"][b] == 0:      # the blob split's labels: name them by hand
                            hand_of = {int(sp["info"][b, k, 1]): k for k in (0, 1) if sp["info"][b, k, 0] > 0}
                            labels[b] = np.vectorize(lambda l: hand_of.get(int(l), R.NONE))(sp["labels"][b]).astype(np.uint16)
                        else:
                            for k in (0, 1):
                                if sp["info"][b, k, 0] == 0:
                                    labels[b][labels[b] == k] = R.NONE
                    source = sp["source"].tolist()
                if mode is None:
                    p, info = c.update_two_hands_sync(f["frames"], cams, **SPLIT)
                else:
                    p, info, src = c.update_two_hands_model(f["frames"], cams, mode=mode, **SPLIT)
                    assert src.tolist() == source and info.tobytes() == sp["info"].tobytes()
                err = c.keypoint_errors(c.keypoints(p.reshape(n, c.nb, 7), table=native.KP_SKELETON, hands=odd)["xyz"], f["kp"])["frame"].reshape(B, 2, 2)
                wrong = [R.mislabelled(labels[b], f["truth"][b]) for b in range(B)]
                rows.append({"offset_m": round(shift, 3), "present": (info[:, :, 0] > 0).astype(int).tolist(), "source": source, "mislabelled_share": [round(wr / fg, 5) for wr, fg in wrong],
                             "mean_error_m": np.round(err[:, :, 0], 5).tolist(), "worst_error_m": np.round(err[:, :, 1], 5).tolist()})
                print(name, json.dumps(rows[-1]), flush=True)
            res["modes"][name] = rows
    finally:
        c.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
