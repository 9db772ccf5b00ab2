"""CPU: the numpy restatement of ht_sensor_simulate (tests/sensor_sim_ref.py) against the definition in include/ht_mi355x.h: hand-written frames whose answers
are worked out below, the statistics the definition promises, stream independence, and three plausible mis-readings that must land on other frames.  The GPU
tests (tests/test_gpu_sensor_sim.py) then hold the kernel to this restatement bit for bit."""
import math

import numpy as np
import pytest

import sensor_ref as R
import sensor_sim_frames as F
import sensor_sim_ref as S

# everything off: far count 1000, stream 3 of seed 7
Z = S.Noise(far_count=1000, fly_bg_count=1000, seed=7, first_index=3)
# the fields of that stream's first nine pixels, written out (they pin mix, the key and the field layout)
UA9 = [45137, 23237, 15679, 40838, 34451, 12813, 3356, 46677, 31708]
T9 = [98, 209, 20, 67, 54, 243, 4, 24, 44]
UB9 = [46011, 25607, 10717, 47710, 15901, 30698, 2891, 25527, 14499]
G9 = [-29, -19, -9, 37, -30, 10, 16, 4, 8]
DARK9 = [2, 0, 2, 0, 1, 4, 1, 1, 1]
GI9 = [0, 2, 16, -12, -21, -4, 17, 22, 38]


def one(kind, frame, nz, **kw):
    d, ir, info = S.simulate_frame(kind, np.array(frame, np.uint16), nz, nz.first_index, **kw)
    return d.tolist(), ir.tolist(), info


def test_mix_and_the_fields_are_pinned():
    assert S.mix(0) == 0 and S.mix(1) == 0x5692161D100B05E5 and S.mix(0x123456789ABCDEF) == 0xB2C058E4EBB5112C
    f = S.fields(Z, 3, 9)
    assert [f[k].tolist() for k in ("ua", "t", "ub", "g", "dark", "gi")] == [UA9, T9, UB9, G9, DARK9, GI9]
    assert S.frame_key(Z, 3) == S.mix(7 ^ ((3 * S.C_FRAME) & S.M64)) and S.frame_key(Z, (1 << 64) + 3) == S.frame_key(Z, 3)


def test_a_1x1_frame_and_the_far_count():
    """no neighbour: never an edge, never a slope; 0 and counts >= far_count are background; a dropped pixel's IR is `dark`, below 8"""
    assert one(S.IVY, [[500]], Z)[:2] == ([[500]], [[16]])
    assert one(S.IVY, [[999]], Z)[0] == [[999]] and one(S.IVY, [[1000]], Z)[0] == [[0]] and one(S.IVY, [[0]], Z)[0] == [[0]] and one(S.IVY, [[65535]], Z)[0] == [[0]]
    assert one(S.IVY, [[500]], Z.but(p_edge_drop=65536, p_slope_drop=65536))[0] == [[500]]
    assert one(S.IVY, [[500]], Z.but(p_hole=65536))[:2] == ([[0]], [[2]])
    # DS4: the background becomes the wall; IR = 16 + 125000 // ((d*d >> 8) + 1): 500 -> 976, 800 -> 2500, 999 -> 3898
    assert one(S.DS4, [[500, 0, 1000, 999]], Z.but(wall_count=800, ir_gain=125000))[:2] == ([[500, 800, 800, 999]], [[16 + 127, 16 + 49, 16 + 49, 16 + 32]])
    assert one(S.DS4, [[500, 0, 1000, 999]], Z)[:2] == ([[500, 0, 0, 999]], [[16, 0, 2, 16]])      # dark of pixels 1 and 2
    # IR noise: gi * ir_noise >> 6 with gi = 0, 2, 16, -12 and ir_noise 32: 0, 1, 8, -6; the clamp at 8
    assert one(S.IVY, [[500, 500, 500, 500]], Z.but(ir_noise=32))[1] == [[16, 17, 24, 10]]
    assert one(S.IVY, [[500, 500, 500, 500]], Z.but(ir_noise=32, ir_floor=0))[1] == [[8, 8, 8, 8]] and one(S.IVY, [[5, 5]], Z.but(ir_gain=1 << 20))[1] == [[255, 255]]


def test_a_3x3_frame_with_a_centre_step():
    """every outer pixel sees the centre 100 counts away and flies towards 600 by t / 256; the centre flies towards its first neighbour, 500:
    600 + ((500 - 600) * 54 >> 8) = 600 - 22 (the shift floors)"""
    frame = [[500, 500, 500], [500, 600, 500], [500, 500, 500]]
    d, ir, info = one(S.IVY, frame, Z.but(p_edge_fly=65536))
    assert d == [[500 + (100 * t >> 8) for t in T9[0:3]], [500 + (100 * T9[3] >> 8), 578, 500 + (100 * T9[5] >> 8)], [500 + (100 * t >> 8) for t in T9[6:9]]]
    assert d == [[538, 581, 507], [526, 578, 594], [501, 509, 517]] and info["edge"].all() and info["fly"].all()
    assert one(S.IVY, frame, Z.but(p_edge_drop=65536))[0] == [[0] * 3] * 3 and one(S.IVY, frame, Z)[0] == frame
    # ua decides: drop below 20000 (pixels 2, 5, 6), fly below 20000 + 15000 (pixels 1, 4, 8), the others stay
    assert one(S.IVY, frame, Z.but(p_edge_drop=20000, p_edge_fly=15000))[0] == [[500, 581, 0], [500, 578, 0], [0, 500, 517]]
    # a step of exactly edge_step is no edge
    assert not one(S.IVY, [[500, 520]], Z)[2]["edge"].any() and one(S.IVY, [[500, 521]], Z)[2]["edge"].all()


def test_a_corner_has_three_neighbours():
    frame = [[500, 500, 500], [500, 500, 500], [500, 500, 700]]
    assert one(S.IVY, frame, Z.but(p_edge_drop=65536))[0] == [[500, 500, 500], [500, 0, 0], [500, 0, 0]]
    # the corner itself against the background: its three neighbours are background, worth fly_bg_count
    d, _, info = one(S.IVY, [[500, 0], [0, 0]], Z.but(p_edge_fly=65536))
    assert d == [[500 + (500 * 98 >> 8), 0], [0, 0]] and info["far"].tolist() == [[1000, 0], [0, 0]]


def test_ties_for_the_far_neighbour_go_to_the_first_in_raster_order():
    """the centre has 400 up right (third in the order) and 600 to its left (fourth), both 100 away: it flies towards 400"""
    frame = [[500, 500, 400], [600, 500, 500], [500, 500, 500]]
    d, _, info = one(S.IVY, frame, Z.but(p_edge_fly=65536))
    assert info["far"].tolist() == [[600, 400, 500], [500, 400, 400], [600, 600, 0]]
    assert d == [[538, 418, 407], [573, 478, 405], [501, 509, 500]]
    assert one(S.IVY, frame, Z.but(p_edge_fly=65536), variant="last")[0][1][1] == 521


def test_slope_and_hole_rules():
    """a ramp of 8 counts a pixel: no edges, gx = 16 > 15 inside the row, 0 at its ends; ub decides"""
    row = [[500 + 8 * x for x in range(9)]]
    d, _, info = one(S.IVY, row, Z.but(p_slope_drop=20000))
    want = [0 if 0 < x < 8 and UB9[x] < 20000 else row[0][x] for x in range(9)]
    assert d == [want] == [[500, 508, 0, 524, 0, 540, 0, 556, 564]] and not info["edge"].any()
    assert one(S.IVY, [[500 + 7 * x for x in range(9)]], Z.but(p_slope_drop=65536))[0] == [[500 + 7 * x for x in range(9)]]      # gx = 14
    assert one(S.IVY, [[v] for v in row[0]], Z.but(p_slope_drop=65536))[0] == [[500]] + [[0]] * 7 + [[564]]      # the same along y
    # a background pixel in the row: its two neighbours have no slope
    assert one(S.IVY, [[500, 508, 516, 0, 532, 540]], Z.but(p_slope_drop=65536, edge_step=65535))[0] == [[500, 0, 516, 0, 532, 540]]
    # holes: ub >= 65536 - 20000 = 45536 (pixels 0 and 3)
    assert one(S.IVY, [[500] * 9], Z.but(p_hole=20000))[0] == [[0, 500, 500, 0, 500, 500, 500, 500, 500]]


def test_axial_noise_by_hand():
    """s = 320 at every depth: 500 + (320 * g + 4736) // 9472"""
    nz = Z.but(sigma0_256=320)
    assert one(S.IVY, [[500] * 9], nz)[0] == [[500 + (320 * g + 4736) // 9472 for g in G9]] == [[499, 499, 500, 501, 499, 500, 501, 500, 500]]
    # s grows with d^2: sigma2 = 537 at 1000 counts is 537 * 10^6 >> 20 = 512
    assert int(S.sd256(Z.but(sigma0_256=128, sigma2=537, far_count=65536), 1000)) == 128 + 512
    # the clamp keeps a noisy pixel a pixel: g = -29, -19, -9 pull below 1; g = 37 gives (65536 * 37 + 4736) // 9472 = 256
    assert one(S.IVY, [[1, 1, 1, 1]], Z.but(sigma0_256=65536))[0] == [[1, 1, 1, 257]]
    assert int(S.noise(Z.but(sigma0_256=65536, sigma2=4096), 65535, 126)) == 65535 and int(S.noise(Z.but(sigma0_256=65536, sigma2=4096), 65535, -126)) == 1


def test_the_disparity_round_trip():
    """K = 1000: 400 -> disp 2.5 rounds up to 3 -> 333; 450 -> 2.22 rounds down to 2 -> 500; 2000 -> 1 -> 1000; 2001 -> 0: dropped"""
    assert S.disparity(1000, [400, 450, 300, 2000, 2001, 3, 7]).tolist() == [333, 500, 333, 1000, 0, 3, 7]
    assert S.disparity(1, [1, 2, 3]).tolist() == [1, 1, 0]                       # 3 // 2, 4 // 4, 5 // 6
    assert S.disparity(1 << 30, [1, 65535]).tolist() == [1, 65535]               # disp 2^30 -> 1; disp 16384 -> 65536, clamped
    assert S.disparity(70000, [50000, 20000]).tolist() == [65535, 17500]         # disp 1 -> 70000, clamped; disp 4 -> 140004 // 8
    nz = Z.but(disparity_k=1000, far_count=3000, wall_count=2500)
    assert one(S.DS4, [[400, 450, 2000, 2001, 0]], nz)[:2] == ([[333, 500, 1000, 0, 0]], [[16, 16, 16, 0, 1]])      # the wall is beyond 2K too
    assert one(S.IVY, [[400, 450, 2000, 2001, 0]], nz)[0] == [[400, 450, 2000, 2001, 0]]                             # Ivy has no disparity


def test_everything_off_keeps_the_foreground():
    frames = F.blobs(76, 20, 3)
    off = F.NOISE_IVY.but(sigma0_256=0, sigma2=0, p_edge_drop=0, p_edge_fly=0, p_slope_drop=0, p_hole=0)
    fg = frames < F.FAR
    d, _ = S.simulate(S.IVY, frames, off)
    assert np.array_equal(d[fg], frames[fg]) and (d[~fg] == 0).all() and fg.any() and (~fg).any()
    d, _ = S.simulate(S.DS4, frames, off.but(wall_count=1234))
    assert np.array_equal(d[fg], frames[fg]) and (d[~fg] == 1234).all()
    d, _ = S.simulate(S.DS4, frames, off)
    assert np.array_equal(d[fg], frames[fg]) and (d[~fg] == 0).all()


def test_noise_statistics_on_a_flat_frame():
    """320x240 at 500 counts, s = 320: mean within 6 standard errors of 0, variance within 2 % of (s/256)^2 * 1365/1369 + 1/12 (the sd's own standard error is 0.26 %)"""
    frame = np.full((240, 320), 500, np.uint16)
    d, _, _ = S.simulate_frame(S.IVY, frame, Z.but(sigma0_256=320), 3)
    e = d.astype(np.int64) - 500
    var = (320 / 256) ** 2 * 1365 / 1369 + 1 / 12
    print("mean %.5f sd %.5f theory %.5f" % (e.mean(), e.std(), math.sqrt(var)))
    assert abs(e.mean()) <= 6 * math.sqrt(var / e.size)
    assert abs(e.var() / var - 1) <= 0.02


@pytest.mark.parametrize("p", [3277, 32768])
def test_drop_fractions(p):
    """each probability alone, on frames where every pixel (every interior column for the slope) is eligible: within 6 binomial standard deviations"""
    h, w = 240, 320
    stripes = np.where(np.arange(w) % 2 == 0, 500, 600).astype(np.uint16)[None, :].repeat(h, 0)      # every pixel an edge
    ramp = (400 + 8 * np.arange(w)).astype(np.uint16)[None, :].repeat(h, 0)                          # no edge, gx = 16 inside
    nz = Z.but(far_count=3999, fly_bg_count=3999)

    def within(k, n):
        sd = math.sqrt(n * (p / 65536) * (1 - p / 65536))
        print("%d of %d, expected %.1f +- %.1f" % (k, n, n * p / 65536, sd))
        assert abs(k - n * p / 65536) <= 6 * sd
    info = S.simulate_frame(S.IVY, stripes, nz.but(p_edge_drop=p, p_edge_fly=p), 3)[2]
    assert info["edge"].all()
    within(int(info["edge_drop"].sum()), w * h); within(int(info["fly"].sum()), w * h)
    d, _, info = S.simulate_frame(S.IVY, ramp, nz.but(p_slope_drop=p), 3)
    assert not info["edge"].any() and not info["slope_drop"][:, [0, -1]].any() and np.array_equal(d == 0, info["slope_drop"])
    within(int(info["slope_drop"].sum()), (w - 2) * h)
    d, _, info = S.simulate_frame(S.IVY, ramp, nz.but(p_hole=p), 3)
    assert np.array_equal(d == 0, info["hole"])
    within(int(info["hole"].sum()), w * h)


def test_flying_pixels_lie_between_the_pixel_and_its_far_neighbour():
    frames = F.blobs(76, 20, 4)
    nz = F.NOISE_IVY.but(sigma0_256=0, sigma2=0, p_hole=0)
    n = 0
    for f in range(4):
        d, _, info = S.simulate_frame(S.IVY, frames[f], nz, f)
        fly = info["fly"]
        p, far, base = frames[f].astype(np.int64)[fly], info["far"][fly], info["base"][fly]
        assert (np.minimum(p, far) <= base).all() and (base <= np.maximum(p, far)).all() and np.array_equal(d[fly], base)
        n += int(fly.sum())
    assert n > 100


def test_a_frames_stream_is_first_index_plus_f():
    frames = F.blobs(36, 20, 12)
    d12, i12 = S.simulate(S.DS4, frames, F.NOISE_DS4)
    d5, i5 = S.simulate(S.DS4, frames[5:10], F.NOISE_DS4.but(first_index=F.NOISE_DS4.first_index + 5))
    assert np.array_equal(d12[5:10], d5) and np.array_equal(i12[5:10], i5)
    assert not np.array_equal(d12[0], S.simulate(S.DS4, frames[:1], F.NOISE_DS4.but(seed=1))[0][0])


def test_three_wrong_restatements_land_on_other_frames():
    frames = F.blobs(36, 20, 3)
    for kind, nz in ((S.IVY, F.NOISE_IVY), (S.DS4, F.NOISE_DS4)):
        right = S.simulate(kind, frames, nz)[0]
        assert not np.array_equal(S.simulate(kind, frames, nz, keyed_by_position=True)[0], right)
        assert not np.array_equal(S.simulate(kind, frames, nz, variant="wrap")[0], right)
        ties = np.random.default_rng(5).choice(np.array([400, 500, 600], np.uint16), (3, 20, 36))      # many pixels 100 counts from neighbours on both sides
        fine = nz.but(disparity_k=0)      # K = 350 maps every depth of this frame to the same disparity
        assert not np.array_equal(S.simulate(kind, ties, fine, variant="last")[0], S.simulate(kind, ties, fine)[0])
        assert np.array_equal(S.simulate(kind, frames, nz.but(first_index=0), keyed_by_position=True)[0], S.simulate(kind, frames, nz.but(first_index=0))[0])


def test_filter_ds4_removes_every_dark_pixel_of_a_simulated_frame():
    frames = F.blobs(76, 40, 2)
    for nz in (F.NOISE_DS4, F.NOISE_DS4_WALL):
        d, ir = S.simulate(S.DS4, frames, nz)
        for f in range(2):
            out = R.filter_ds4(d[f], ir[f], None, max_width=76)
            dark = ir[f] < 8
            assert dark.any() and (~dark).any() and (out[dark] == 4096).all() and np.array_equal(dark, d[f] == 0) and (out != 4096).any()


def test_the_test_frames_take_every_branch():
    for w, h, B in ((3, 3, 64), (4, 4, 64), (17, 9, 3), (36, 20, 3)):
        c = F.counts(S.DS4, F.blobs(w, h, B), F.NOISE_DS4)
        assert min(c.values()) > 0, (w, h, c)
