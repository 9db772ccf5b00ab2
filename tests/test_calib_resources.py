"""What the compiler made of the calibration kernels (the build's kernel-resource-usage remarks, as tests/test_views_resources.py reads them): no private segment and no
register spilled to memory in any of the three.  k_calib_cloud is k_fuse_views' walk of one view and is held as that kernel is (64 VGPRs, eight waves a SIMD).
k_calib_accum carries 29 float64 sums in registers beside the closest-feature walk: 128 VGPRs at most, four waves a SIMD, and an LDS footprint of the body table and the
4 x 29 doubles the waves meet through -- not 29 x 256 doubles.  k_calib_solve holds the 6 x 6 factor in registers."""
import pytest

from hand_tracking_samples_amd import build


@pytest.fixture(scope="module")
def usage():
    u = build.resource_usage()
    if not any("k_calib_accum" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    return u


def _one(usage, part):
    hits = [k for k in usage if part in k]
    assert len(hits) == 1, (part, hits)
    return usage[hits[0]]


@pytest.mark.parametrize("kernel,vgprs,occupancy,lds", [("k_calib_cloud", 64, 8, 64), ("k_calib_accum", 128, 4, 32 * 32 * 4 + 4 * 29 * 8), ("k_calib_solve", 96, 5, 32 * 8)])
def test_calibration_kernels(usage, kernel, vgprs, occupancy, lds):
    k = _one(usage, kernel)
    print(kernel, k)
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0
    assert k["VGPRs"] <= vgprs and k["Occupancy"] >= occupancy and k["LDS Size"] <= lds
