"""CPU: pins the yardstick of the sensor filters (tests/sensor_ref.py, a restatement of the reference's include/dcam.h:157-226) and the properties of the
frames tests/test_gpu_sensor.py runs the device on (tests/sensor_frames.py)."""
import numpy as np
import pytest

import sensor_frames as F
import sensor_ref as R

CAM = np.array([610.0, 610.0, 320.0, 240.0, 0.001, 0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 1.0], np.float32)
GPU_DS4_CASES = ((16, 12, 3), (68, 12, 3), (76, 20, 3), (320, 240, 3), (16, 12, 70))      # (w, h, B) of tests/test_gpu_sensor.py


@pytest.mark.parametrize("make,axis", [(F.cascade_rows, 1), (F.cascade_cols, 0)])
def test_one_dark_pixel_decides_the_far_end_of_its_row_or_column(make, axis):
    """the dependency of the flying-pixel pass runs the whole length of a 320x240 frame: darkening pixel (2, y) / (x, 2) changes the result at x >= w-6 / y >= h-6.
    Measured here: a 400-pixel cascade row keeps 264 of its 396 interior pixels, and none with its pixel 2 dark."""
    d, ir = make(320, 240)
    base = R.filter_ds4(d, ir)
    dark = ir.copy()
    if axis == 1:
        dark[2:-2, 2] = 0
    else:
        dark[2, 2:-2] = 0
    got = R.filter_ds4(d, dark)
    diff = base != got
    far = diff[2:-2, 320 - 6:320 - 2] if axis == 1 else diff[240 - 6:240 - 2, 2:-2]
    assert far.any(axis=axis).all()      # every interior row / column changes within its last four interior pixels
    n = 236 * 316
    assert (base[2:-2, 2:-2] != 4096).sum() > 0.6 * n and (got[2:-2, 2:-2] != 4096).sum() < 0.05 * n
    d4, ir4 = F.cascade_rows(400, 5)
    assert (R.filter_ds4(d4, ir4, max_width=400)[2, 2:-2] != 4096).sum() == 264
    ir4[2, 2] = 0
    assert (R.filter_ds4(d4, ir4, max_width=400)[2, 2:-2] != 4096).sum() == 0


@pytest.mark.parametrize("family", sorted(F.FAMILIES))
def test_the_naive_form_is_wrong_on_every_frame_the_device_is_tested_on(family):
    """a condition on the inputs: on each frame with an interior the naive form differs from the restatement on >= 5 % of the interior and >= 10 % of it is kept"""
    worst = [1.0, 1.0]
    for w, h, B in GPU_DS4_CASES:
        D, I = F.batch(family, w, h, B)
        assert len({D[b].tobytes() + I[b].tobytes() for b in range(B)}) == B      # distinct frames
        for b in range(B):
            differ, kept = F.judge(D[b], I[b])
            worst = [min(worst[0], differ), min(worst[1], kept)]
            assert differ >= F.DIFFER_MIN and kept >= F.KEPT_MIN, (family, w, h, b, differ, kept)
    print(family, "least differing %.3f, least kept %.3f" % tuple(worst))


def test_a_killed_neighbour_counts_as_near_for_values_around_4096():
    """p[i-1] is read as already rewritten: 4090 next to a killed pixel has a near left neighbour (4096), 4080 has not"""
    for v, kept in ((4090, True), (4087, True), (4105, True), (4086, False), (4106, False), (4080, False)):
        d = np.full((5, 8), 1000, np.uint16); ir = np.full((5, 8), 100, np.uint8)
        d[:, 3] = 2000        # column 3: no horizontal neighbour within 10 -> killed at (3, 2)
        d[:, 4] = v           # its right neighbour survives only through the killed pixel's 4096 ...
        d[:, 5] = v + 20      # ... since nothing to its right is near
        d[:, 6] = v if kept else v + 40
        d[:, 2] = 2000 + 30; d[:, 1] = 2000 + 60
        out = R.filter_ds4(d, ir)
        assert out[2, 3] == 4096
        # has(1) at x = 4: right is v + 20 (far), left is the killed 4096; has(2): x = 6 holds v when `kept`
        assert (out[2, 4] == v) == kept, (v, out[2])
    # and the naive form, which reads the left neighbour as 2000, kills 4090
    d = np.full((5, 8), 1000, np.uint16); ir = np.full((5, 8), 100, np.uint8)
    d[:, 3] = 2000; d[:, 4] = 4090; d[:, 5] = 4110; d[:, 6] = 4090; d[:, 2] = 2030; d[:, 1] = 2060
    assert R.filter_ds4(d, ir)[2, 4] == 4090 and F.naive_ds4(d, ir)[2, 4] == 4096


def test_pass_one_and_the_background_model():
    d = np.full((4, 4), 500, np.uint16); ir = np.full((4, 4), 8, np.uint8)
    d[0, 0] = 29; d[0, 1] = 30; ir[1, 1] = 7
    bg = np.full((4, 4), 500, np.uint16); bg[2, 2] = 499
    out = R.filter_ds4(d, ir, bg)
    assert out[0, 0] == 4096 and out[0, 1] == 30 and out[1, 1] == 4096 and out[2, 2] == 4096 and out[3, 3] == 500
    with pytest.raises(ValueError):
        R.filter_ds4(np.zeros((4, 8), np.uint16), np.zeros((4, 8), np.uint8), max_width=4)


def test_ivy_gather_equals_the_repeated_downsample_loop():
    rng = np.random.default_rng(5)
    for (w, h), mw, k in (((12, 8), 12, 0), ((24, 16), 12, 1), ((48, 32), 12, 2), ((36, 20), 9, 2)):
        d = rng.integers(0, 3, (h, w)).astype(np.uint16) * rng.integers(1, 4000, (h, w)).astype(np.uint16)
        a, ca = R.filter_ivy(d, CAM, mw)
        b, cb = R.filter_ivy_loops(d, CAM, mw)
        assert a.shape == (h >> k, w >> k) and np.array_equal(a, b) and ca.tobytes() == cb.tobytes()
        assert np.array_equal(ca[:4], CAM[:4] / np.float32(2 ** k)) and np.array_equal(ca[4:], CAM[4:])
        assert R.out_dims(R.IVY, w, h, mw) == (w >> k, h >> k)


def test_ivy_fills_after_the_halving_and_with_the_reference_value():
    d = np.array([[0, 7, 5, 7], [7, 7, 7, 7], [9, 7, 0, 7], [7, 7, 7, 7]], np.uint16)
    d[0, 1] = 0      # a zero the halving drops
    out, _ = R.filter_ivy(d, CAM, 2)
    assert out.tolist() == [[3999, 5], [9, 3999]]      # 4.0f / 0.001f is 3999.99976 in float: the reference's 4 m background is 3999 counts
    assert R.ivy_fill(0.001) == 3999 and R.ivy_fill(0.000125) == int(np.float32(4.0) / np.float32(0.000125)) and 31999 <= R.ivy_fill(0.000125) <= 32000
    assert R.ivy_fill(0.0001) == int(np.float32(4.0) / np.float32(0.0001)) & 0xFFFF
    assert R.ivy_fill(0.00005) == int(np.float32(4.0) / np.float32(0.00005)) - 65536      # wraps past 16 bits
    assert R.ivy_fill(0.0) == 0 and R.ivy_fill(1e-12) == 0                                  # does not fit an int32: INT_MIN, low bits 0
    for bad in ((R.IVY, 642, 480, 320), (R.IVY, 640, 481, 320), (R.DS4, 640, 480, 320), (R.IVY, 0, 4, 4), (R.IVY, 4097, 4, 4), (R.IVY, 4, 4, 0), (2, 4, 4, 4)):
        with pytest.raises(ValueError):
            R.out_dims(*bad)


def test_addbackground_wraps_below_the_fudge():
    d = np.array([[0, 2, 3, 4000, 5000]], np.uint16)
    bg = R.add_background(None, d, 3)
    assert bg.tolist() == [[4096, 4096, 0, 3997, 4096]]      # 0 - 3 and 2 - 3 wrap to 65533 and 65535
    bg = R.add_background(bg, np.array([[10, 10, 10, 10, 10]], np.uint16), 3)
    assert bg.tolist() == [[7, 7, 0, 7, 7]]
