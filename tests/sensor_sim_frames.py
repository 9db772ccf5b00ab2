"""Clean input frames for the tests of ht_sensor_simulate: synthetic blobs in front of a far wall, from a seeded numpy generator, and the noise sets the tests
run them under.  A frame has tilted elliptical blobs (every other one steep enough for the grazing-angle rule, none so steep that its own pixels are edges), so
that at any size with an interior a batch takes every branch of the definition: edge drop, flying pixel, slope drop, hole, and disparity drop under NOISE_DS4
(whose K = 350 drops depths above 700 counts)."""
import numpy as np

import sensor_sim_ref as S

FAR = 3999
NOISE_IVY = S.Noise(seed=0x1234567, first_index=10, far_count=FAR, sigma0_256=128, sigma2=537, edge_step=20, slope_step=15, p_edge_drop=22938, p_edge_fly=16384, p_slope_drop=32768, p_hole=3000,
                    fly_bg_count=FAR, ir_floor=16, ir_gain=125000, ir_noise=8)
NOISE_DS4 = NOISE_IVY.but(seed=0x7654321, sigma0_256=51, sigma2=1074, p_edge_drop=16384, p_edge_fly=22938, disparity_k=350, wall_count=0)
NOISE_DS4_FINE = NOISE_DS4.but(disparity_k=683200)      # the default's K: steps of a third of a count at half a metre, nothing dropped
NOISE_DS4_WALL =NOISE_DS4.but(wall_count=1500, disparity_k=0, fly_bg_count=1500)


def blobs(w, h, B, seed=0, background=FAR):
    """u16[B,h,w]: `background` (the renderer's far count, or 0) with two blobs per frame at 450 .. 800 counts"""
    rng = np.random.default_rng([seed, w, h])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.full((B, h, w), background, np.uint16)
    for f in range(B):
        for k in range(2):
            cx, cy = rng.uniform(0.15, 0.85) * (w - 1), rng.uniform(0.15, 0.85) * (h - 1)
            rx, ry = max(1.3, rng.uniform(0.2, 0.45) * w), max(1.3, rng.uniform(0.2, 0.45) * h)
            steep = (f + k) % 2 == 0
            ax, ay = (rng.uniform(8, 10) * rng.choice([-1, 1]), rng.uniform(0, 6)) if steep else (rng.uniform(-3, 3), rng.uniform(-3, 3))
            z = rng.uniform(520, 720) + ax * (x - cx) + ay * (y - cy)
            inside = ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1.0
            out[f][inside] = np.clip(np.rint(z[inside]), 450, 800).astype(np.uint16)
    return out


def counts(kind, frames, nz):
    """how often the restatement took each branch over a batch"""
    tot = dict(edge_drop=0, fly=0, slope_drop=0, hole=0, disp_drop=0, foreground=0, background=0)
    for f in range(len(frames)):
        info = S.simulate_frame(kind, frames[f], nz, nz.first_index + f)[2]
        for k in ("edge_drop", "fly", "slope_drop", "hole", "disp_drop"):
            tot[k] += int(info[k].sum())
        fg = (frames[f] != 0) & (frames[f] < nz.far_count)
        tot["foreground"] += int(fg.sum()); tot["background"] += int((~fg).sum())
    return tot


# every refusal of the definition, as changes to a call that is fine
def refusals(depth_as_out):
    return [dict(kind=2), dict(kind=-1), dict(w=0), dict(h=0), dict(w=4097), dict(h=4097), dict(B=-1), dict(depth=None), dict(out=None), dict(noise=None), dict(kind=1, ir=None),
            dict(out=depth_as_out), dict(nz=dict(far_count=0)), dict(nz=dict(far_count=65537)), dict(nz=dict(p_edge_drop=-1)), dict(nz=dict(p_edge_fly=65537)), dict(nz=dict(p_slope_drop=65537)),
            dict(nz=dict(p_hole=-1)), dict(nz=dict(p_hole=65537)), dict(nz=dict(p_edge_drop=40000, p_edge_fly=25537)), dict(nz=dict(sigma0_256=65537)), dict(nz=dict(sigma0_256=-1)),
            dict(nz=dict(sigma2=4097)), dict(nz=dict(sigma2=-1)), dict(nz=dict(edge_step=-1)), dict(nz=dict(edge_step=65536)), dict(nz=dict(slope_step=-1)), dict(nz=dict(fly_bg_count=65536)),
            dict(nz=dict(wall_count=-1)), dict(nz=dict(wall_count=65536)), dict(nz=dict(disparity_k=-1)), dict(nz=dict(disparity_k=(1 << 30) + 1)), dict(nz=dict(ir_floor=-1)),
            dict(nz=dict(ir_gain=-1)), dict(nz=dict(ir_noise=65537))]
