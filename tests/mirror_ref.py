"""The mirror x -> -x of the camera's space in numpy (include/ht_mi355x.h "left hands"): the definition the mirror kernels and ht_update_hands_* are held to.
hands: uint8 [B], nonzero = mirrored, None = every frame; everything else is copied.  Signs are flipped as bits, so -0.0 and NaNs follow."""
import numpy as np

SIGN = np.uint32(0x80000000)


def _sel(hands, B):
    return np.ones(B, bool) if hands is None else np.asarray(hands).reshape(B) != 0


def frames(depth, hands=None):
    """depth u16 [B,h,w]: F'[y][x] = F[y][w-1-x]"""
    out = np.array(depth, np.uint16, copy=True); m = _sel(hands, len(out))
    out[m] = out[m][:, :, ::-1]
    return out


def poses(p, hands=None):
    """p [B,...,7]: (px,py,pz, qx,qy,qz,qw) -> (-px,py,pz, qx,-qy,-qz,qw)"""
    out = np.array(p, np.float32, copy=True); bits = out.view(np.uint32); m = _sel(hands, len(out))
    for k in (0, 4, 5):
        bits[m, ..., k] ^= SIGN
    return out


def cams(c, w, hands=None):
    """c [B,12] (focal xy, principal xy, depth_scale, pose): cx' = float32(w-1) - cx, the pose as a pose"""
    out = np.array(c, np.float32, copy=True); m = _sel(hands, len(out))
    out[m, 2] = np.float32(w - 1) - out[m, 2]
    out[:, 5:] = poses(out[:, 5:], m)
    return out
