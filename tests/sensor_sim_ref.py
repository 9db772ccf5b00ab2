"""A numpy restatement of ht_sensor_simulate (include/ht_mi355x.h, "raw camera frames from rendered depth"), written from the header's
definition alone: Python integers for the per-frame key, int64 / uint64 arrays for the pixels.  `//` is floor division and `>>` on int64 is arithmetic, as the
definition asks.  It shares no code with csrc/ht_sensor.hip.

`variant` makes one of the wrong restatements tests/test_sensor_sim_ref.py tells apart from the right one:
  "wrap"      a neighbour is pixel i + dy*w + dx of the frame whenever that index exists, so rows wrap at their ends
  "last"      the far neighbour is the last neighbour with the largest difference, not the first
simulate(..., keyed_by_position=True) is the third: frame f's stream is f, whatever first_index says."""
import numpy as np

IVY, DS4 = 0, 1
M64 = (1 << 64) - 1
C_FRAME, C_PIXEL, C_IR = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93, 0xA0761D6478BD642F
FIELDS = ("seed", "first_index", "far_count", "sigma0_256", "sigma2", "edge_step", "slope_step", "p_edge_drop", "p_edge_fly", "p_slope_drop", "p_hole", "fly_bg_count",
          "disparity_k", "wall_count", "ir_floor", "ir_gain", "ir_noise")
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))      # (dy, dx) in raster order


class Noise:
    """ht_sensor_noise, field for field.  The defaults switch everything off: the simulation then only maps background to 0 (or to wall_count)."""

    def __init__(self, **kw):
        self.seed = 0; self.first_index = 0; self.far_count = 3999
        self.sigma0_256 = 0; self.sigma2 = 0; self.edge_step = 20; self.slope_step = 15
        self.p_edge_drop = 0; self.p_edge_fly = 0; self.p_slope_drop = 0; self.p_hole = 0
        self.fly_bg_count = 3999; self.disparity_k = 0; self.wall_count = 0
        self.ir_floor = 16; self.ir_gain = 0; self.ir_noise = 0
        for k, v in kw.items():
            if k not in FIELDS:
                raise TypeError(k)
            setattr(self, k, int(v))

    def but(self, **kw):
        return Noise(**dict({k: getattr(self, k) for k in FIELDS}, **kw))


def mix(x):
    x &= M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def _mix_np(x):
    x = x.astype(np.uint64)
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def frame_key(nz, index):
    return mix(nz.seed ^ (((index & M64) * C_FRAME) & M64))


def _bits(H, lo, n):
    return ((H >> np.uint64(lo)) & np.uint64((1 << n) - 1)).astype(np.int64)


def fields(nz, index, n):
    """The random fields of pixels 0 .. n-1 of stream `index`: ua, t, ub, g (of H), dark, gi (of H2), each int64[n]."""
    i = np.arange(1, n + 1, dtype=np.uint64)
    H = _mix_np(np.uint64(frame_key(nz, index)) ^ (i * np.uint64(C_PIXEL)))
    H2 = _mix_np(H ^ np.uint64(C_IR))
    g = _bits(H, 40, 6) + _bits(H, 46, 6) + _bits(H, 52, 6) + _bits(H, 58, 6) - 126
    return dict(ua=_bits(H, 0, 16), t=_bits(H, 16, 8), ub=_bits(H, 24, 16), g=g, dark=_bits(H2, 0, 3), gi=_bits(H2, 8, 6) + _bits(H2, 14, 6) - 63)


def sd256(nz, d):
    """the axial standard deviation in 1/256 count at depth d"""
    d = np.asarray(d, np.int64)
    return nz.sigma0_256 + ((nz.sigma2 * d * d) >> 20)


def noise(nz, d, g):
    d = np.asarray(d, np.int64)
    return np.clip(d + (sd256(nz, d) * g + 4736) // 9472, 1, 65535)


def disparity(K, d1):
    """step 9 on nonzero depths d1: (the depth after the round trip, or 0 where disp == 0)"""
    d1 = np.asarray(d1, np.int64)
    safe = np.maximum(d1, 1)
    disp = (2 * K + safe) // (2 * safe)
    back = np.minimum(65535, (2 * K + disp) // (2 * np.maximum(disp, 1)))
    return np.where(disp == 0, 0, back)


def simulate_frame(kind, frame, nz, index, variant=None):
    """One frame u16[h,w] of stream `index` -> (depth u16[h,w], ir u8[h,w], info).  info: the masks edge, edge_drop, fly, slope_drop, hole, disp_drop and the int64
    images far (v of the far neighbour, where edge) and base (the depth before the noise, where a foreground pixel survived steps 3-7)."""
    assert kind in (IVY, DS4) and variant in (None, "wrap", "last")
    frame = np.asarray(frame)
    h, w = frame.shape
    n = w * h
    p = frame.astype(np.int64)
    F = fields(nz, index, n)
    ua, t, ub, g = (F[k].reshape(h, w) for k in ("ua", "t", "ub", "g"))
    is_fg = lambda q: (q != 0) & (q < nz.far_count)
    fg = is_fg(p)

    pad = np.full((h + 2, w + 2), -1, np.int64)
    pad[1:-1, 1:-1] = p
    flat = p.reshape(-1)
    best = np.full((h, w), -1, np.int64); far = np.zeros((h, w), np.int64)
    for dy, dx in NEIGHBOURS:
        if variant == "wrap":
            idx = np.arange(n, dtype=np.int64) + dy * w + dx
            ok = (idx >= 0) & (idx < n)
            q = np.where(ok, flat[np.clip(idx, 0, n - 1)], -1).reshape(h, w)
        else:
            q = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        present = q >= 0
        v = np.where(is_fg(q), q, nz.fly_bg_count)
        diff = np.where(present, np.abs(v - p), -1)
        take = (diff >= best) if variant == "last" else (diff > best)
        take &= present
        far = np.where(take, v, far); best = np.where(take, diff, best)
    edge = fg & (best > nz.edge_step)

    def central(a, b):      # |a - b| where both are in the image and foreground, else 0
        return np.where((a >= 0) & (b >= 0) & is_fg(a) & is_fg(b), np.abs(a - b), 0)
    gx = central(pad[1:-1, 2:], pad[1:-1, :-2]); gy = central(pad[2:, 1:-1], pad[:-2, 1:-1])

    edge_drop = edge & (ua < nz.p_edge_drop)
    fly = edge & ~edge_drop & (ua < nz.p_edge_drop + nz.p_edge_fly)
    base = np.where(fly, p + (((far - p) * t) >> 8), p)
    slope_drop = fg & ~edge & (np.maximum(gx, gy) > nz.slope_step) & (ub < nz.p_slope_drop)
    hole = fg & (ub >= 65536 - nz.p_hole)
    live = fg & ~(edge_drop | slope_drop | hole)
    d1 = np.where(live, noise(nz, base, g), 0)
    if kind == DS4 and nz.wall_count > 0:
        d1 = np.where(fg, d1, noise(nz, np.full((h, w), nz.wall_count, np.int64), g))
    disp_drop = np.zeros((h, w), bool)
    if kind == DS4 and nz.disparity_k > 0:
        back = disparity(nz.disparity_k, d1)
        disp_drop = (d1 != 0) & (back == 0)
        d1 = np.where(d1 != 0, back, 0)
    dark, gi = F["dark"].reshape(h, w), F["gi"].reshape(h, w)
    lit = np.clip(nz.ir_floor + nz.ir_gain // (((d1 * d1) >> 8) + 1) + ((gi * nz.ir_noise) >> 6), 8, 255)
    ir = np.where(d1 != 0, lit, dark)
    info = dict(edge=edge, edge_drop=edge_drop, fly=fly & ~hole, slope_drop=slope_drop, hole=hole, disp_drop=disp_drop, far=np.where(edge, far, 0), base=np.where(live, base, 0))
    return d1.astype(np.uint16), ir.astype(np.uint8), info


def simulate(kind, frames, nz, variant=None, keyed_by_position=False):
    """frames u16[B,h,w] -> (depth u16[B,h,w], ir u8[B,h,w]); frame f is stream first_index + f"""
    frames = np.asarray(frames)
    out = [simulate_frame(kind, frames[f], nz, f if keyed_by_position else nz.first_index + f, variant)[:2] for f in range(len(frames))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def check(kind, nz, w, h, B, ir_given=True):
    """What the calls refuse on the noise set and sizes alone: None, or a word about the first refusal."""
    if kind not in (IVY, DS4): return "kind"
    if not (1 <= w <= 4096 and 1 <= h <= 4096): return "size"
    if B < 0: return "B"
    if kind == DS4 and not ir_given: return "ir"
    if not 1 <= nz.far_count <= 65536: return "far_count"
    for k in ("p_edge_drop", "p_edge_fly", "p_slope_drop", "p_hole"):
        if not 0 <= getattr(nz, k) <= 65536: return k
    if nz.p_edge_drop + nz.p_edge_fly > 65536: return "p_edge_drop + p_edge_fly"
    for k, hi in (("sigma0_256", 65536), ("sigma2", 4096), ("edge_step", 65535), ("slope_step", 65535), ("fly_bg_count", 65535), ("wall_count", 65535), ("disparity_k", 1 << 30),
                  ("ir_floor", 65536), ("ir_gain", (1 << 31) - 1), ("ir_noise", 65536)):
        if not 0 <= getattr(nz, k) <= hi: return k
    return None
