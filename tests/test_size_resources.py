"""What the compiler made of the hand-size kernels (the build's kernel-resource-usage remarks, as tests/test_calib_resources.py reads them): no private segment and no
register spilled to memory in either.  k_size_accum carries 37 float64 sums in registers beside the closest-feature walk k_calib_accum runs with 29: 138 VGPRs, which is
three waves a SIMD where k_calib_accum's 112 give four (holding it to 128 spills 10 registers, 44 bytes a lane of scratch), and an LDS footprint of
the body table and the 4 x 37 doubles the waves meet through.  k_size_solve holds a slot's 38 sums and the 7 x 7 factor in registers: 120 VGPRs, four waves a SIMD (its
block of 256 threads needs one), 80 bytes of LDS."""
import pytest

from hand_tracking_samples_amd import build


@pytest.fixture(scope="module")
def usage():
    u = build.resource_usage()
    if not any("k_size_accum" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    return u


def _one(usage, part):
    hits = [k for k in usage if part in k]
    assert len(hits) == 1, (part, hits)
    return usage[hits[0]]


@pytest.mark.parametrize("kernel,vgprs,occupancy,lds", [("k_size_accum", 144, 3, 32 * 32 * 4 + 4 * 37 * 8), ("k_size_solve", 128, 4, 10 * 8)])
def test_size_kernels(usage, kernel, vgprs, occupancy, lds):
    k = _one(usage, kernel)
    print(kernel, k)
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0
    assert k["VGPRs"] <= vgprs and k["Occupancy"] >= occupancy and k["LDS Size"] <= lds
