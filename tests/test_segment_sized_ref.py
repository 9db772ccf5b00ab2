"""CPU side of the sized segmentation (ht_segment_vr_sized, ht_update_frames_sized_*): the numpy SampleD the GPU tests judge the 128x128 tiles with is pinned
to the reference's own tiles, the size rule's table, and the new symbols.

tests/segment_ref.py must reproduce all 16 reference tiles of tests/golden/segment6.npz bit for bit at side 64, given the reference's own cameras (six frames under
option 0xF, the first two also under 1, 2, 4, 8 and 5; tiles with 0 to 1773 pixels outside the source).  That holds with or without the sized calls; the table and the
symbols need them.
"""
import os
import subprocess

import numpy as np
import pytest

import segment_ref
from hand_tracking_samples_amd import native

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "segment6.npz"))
CASES = [(i, o) for i in range(6) for o in ([15, 1, 2, 4, 8, 5] if i < 2 else [15])]


def test_numpy_sample_d_reproduces_every_reference_tile():
    outside = []
    for frame, opt in CASES:
        cam = FIX["s%d__o%d__cam" % (frame, opt)]
        tile, out = segment_ref.sample_d(FIX["s%d__depth" % frame], FIX["s%d__cam" % frame], cam, 64)
        assert (tile != FIX["s%d__o%d__tile" % (frame, opt)]).sum() == 0, (frame, opt)
        outside.append(int(out.sum()))
    assert len(CASES) == 16 and min(outside) == 0 and max(outside) > 1000, outside      # both branches of SampleD are pinned


def test_side128_camera_is_the_side64_camera_scaled():
    cam = FIX["s0__o15__cam"]
    c = segment_ref.side128_camera(cam)
    assert c[0] == cam[0] * 2 and c[1] == cam[1] * 2 and c[2] == 64 and c[3] == 64 and c[4:].tobytes() == cam[4:].tobytes()
    assert np.frexp(c[0])[0] == np.frexp(cam[0])[0]      # a power of two: the mantissa does not move


@pytest.mark.parametrize("w,h,side,ok", [(8, 8, 64, True), (320, 240, 64, True), (324, 240, 64, True), (640, 480, 64, True), (2560, 120, 64, True), (120, 2560, 64, True),
                                         (8, 8, 128, True), (320, 240, 128, True), (324, 240, 128, True), (640, 480, 128, True), (2560, 120, 128, True), (120, 2560, 128, True),
                                         (644, 480, 64, False), (642, 480, 64, False), (4, 8, 64, False), (644, 480, 128, False), (642, 480, 128, False), (4, 8, 128, False),
                                         (640, 480, 96, False), (640, 480, 0, False), (320, 240, 96, False), (320, 240, 0, False)])
def test_supported_table(w, h, side, ok):
    L = native.load()
    assert L.ht_segment_vr_supported(w, h, side) == (0 if ok else 1)      # HT_OK / HT_ERR_ARG
    assert native.segment_vr_supported(w, h, side) == ok


def test_symbols_exported_and_bound():
    L = native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    header = open(os.path.join(os.path.dirname(HERE), "include", "ht_mi355x.h")).read()
    for s in ("ht_segment_vr_supported", "ht_segment_vr_sized", "ht_segment_vr_sized_dev", "ht_update_frames_sized_sync", "ht_update_frames_sized_dev"):
        assert s in native.SYMBOLS and s in exported and hasattr(L, s) and ("int %s(" % s) in header, s
    for m in ("segment_vr_sized", "update_frames_sized_sync", "update_frames_sized_dev"):
        assert hasattr(native.Context, m), m
