"""What the compiler made of the several-views kernels (the build's kernel-resource-usage remarks, as tests/test_build_resources.py reads them for the others): no
private segment and no register spilled to memory.  k_fuse_views is a byte mover that hides its loads behind other waves: within 64 VGPRs, eight waves a SIMD.
k_view_rows is k_cloud_rows' per-frame code in its views mode and is held as that kernel is: no scratch, 128 VGPRs at most (four blocks a CU), the same LDS."""
import pytest

from hand_tracking_samples_amd import build


@pytest.fixture(scope="module")
def usage():
    u = build.resource_usage()
    if not any("k_fuse_views" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    return u


def _one(usage, part):
    hits = [k for k in usage if part in k]
    assert len(hits) == 1, (part, hits)
    return usage[hits[0]]


def test_fuse_kernel(usage):
    k = _one(usage, "k_fuse_views")
    print(k)
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0
    assert k["VGPRs"] <= 64 and k["Occupancy"] >= 8 and k["LDS Size"] <= 64


def test_view_rows_kernel(usage):
    k, parent = _one(usage, "k_view_rows"), _one(usage, "k_cloud_rows")
    print(k, parent)
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["VGPRs"] <= 128 and k["Occupancy"] >= 4
    assert k["LDS Size"] == parent["LDS Size"]
    assert k["SGPRs Spill"] <= parent["SGPRs Spill"]      # scalar registers parked in vector lanes, never in memory (ScratchSize 0): no more of them than the kernel it is a mode of
