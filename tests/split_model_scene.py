"""The rendered scenes of the model split's tests, built on the host: hull frames of both hands of section 27's scene (ht_render_depth's geometry,
the hulls closest() measures) by ht_model_hitcheck per pixel, and the touching scene found from them.  The left hand's frame is the canonical (mirrored) pose rendered
through the mirrored camera and flipped: every operation of the ray cast is symmetric under the sign flips (tests/test_mirror_ref.py), so it is the frame of the
mirrored model at the real-space pose."""
import os

import numpy as np

import mirror_ref
import split_model_ref as R
import split_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
STEP = 0.005      # the lateral offset is reduced in 5 mm steps
TOUCH_SHIFT = 0.05      # where both scenes' hull frames first merge into one blob (asserted by tests/test_split_model_ref.py on the host and by the GPU test on the device)


def hull_frame(m, poses, cam, w, h, far=4.0):
    """FakeDepth (synthetic-tracker.cpp:69-76) of the hulls at centre-of-mass poses [nb,7]: only the pixels of the box around the bodies' projected outer spheres are
    cast (a hull lies inside its body's outer sphere), the others are background"""
    import htfx
    radius = htfx.load(R.MODEL17)["body_f"][:, 2].astype(np.float64)
    bg = int(F(F(far) / F(cam[4])))
    out = np.full((h, w), bg, np.uint16)
    p = np.asarray(poses, np.float64)[:, :3]
    z = p[:, 2] - radius
    assert (z > 0.05).all()
    x0 = int(np.floor(((p[:, 0] - radius) / z * cam[0] + cam[2]).min())) - 1; x1 = int(np.ceil(((p[:, 0] + radius) / z * cam[0] + cam[2]).max())) + 2
    y0 = int(np.floor(((p[:, 1] - radius) / z * cam[1] + cam[3]).min())) - 1; y1 = int(np.ceil(((p[:, 1] + radius) / z * cam[1] + cam[3]).max())) + 2
    o = np.zeros(3, F); fr = F(far)
    for y in range(max(y0, 0), min(y1, h)):
        for x in range(max(x0, 0), min(x1, w)):
            v1 = np.array([(F(x) - cam[2]) / cam[0] * fr, (F(y) - cam[3]) / cam[1] * fr, F(1.0) * fr], F)
            imp, _, b = m.hitcheck(poses, o, v1)
            out[y, x] = np.uint16(int(F(imp[2] / cam[4])))
    return out


def solo_frames(m, poses2, cam=S.SCENE_CAM, w=S.SCENE_W, h=S.SCENE_H):
    """[2][h][w]: the right hand's hull frame and the left hand's (poses2[1] in real space)"""
    right = hull_frame(m, poses2[0], cam, w, h)
    left = hull_frame(m, mirror_ref.poses(poses2[1][None])[0], mirror_ref.cams(cam[None], w)[0], w, h)[:, ::-1]
    return np.stack([right, np.ascontiguousarray(left)])



# ---- the hand-made cases (tests/test_split_model_ref.py writes their answers out; tests/test_gpu_split_model.py runs them on the device) -----------------------------
SMALL_FAR, SMALL_HI = 4000, 650
SMALL_CAM = np.array([20, 20, 3.5, 3.5, 0.001, 0, 0, 0, 0, 0, 0, 1], F)      # at 0.43 m pixel 1 is 0.054 m left of the axis, pixel 6 as far right
FOUR = {(1, 1): 430, (6, 2): 431, (2, 5): 432, (6, 6): 433}                  # one pixel in every cell of an 8x8 frame


def hand_made_priors():
    """a tracked hand of tests/golden/poses1024.htfx moved 0.08 m to the high-x side (bodies at x 0.025 .. 0.095, z 0.37 .. 0.49), and its mirror image as the left hand"""
    import htfx
    right = htfx.load(os.path.join(HERE, "golden", "poses1024.htfx"))["other_pose"][0].astype(F)
    right[:, 0] += F(0.08)
    return np.stack([right, mirror_ref.poses(right[None])[0]])


def small_frame(pixels):
    """an 8x8 frame of SMALL_FAR with the given {(x, y): depth}"""
    f = np.full((8, 8), SMALL_FAR, np.uint16)
    for (x, y), d in pixels.items():
        f[y, x] = d
    return f
