"""CPU: tests/views_ref.py, the restatement the device's several-views calls are held to (tests/test_gpu_views.py), pinned on the reference-pinned oracle: a view with
identity pose and no mirror is ho_pointcloud bit for bit; every source of the shared scenes has points; the rows are CloudConstraint from each point's own origin with
FitPointCloud's limits; and the per-source origin matters: judged from view 0's origin, most rows of a camera on the far side of the hand come out differently."""
import ctypes as C

import numpy as np
import pytest

import joints_inputs as ji
import kpfit_inputs as ki
import oracle_lib as ol
import views_ref as vr

SIZES = ((37, 29), (80, 60))      # no multiples of 4; 1073 and 4800 pixels: several 256-pixel chunks
# rows of the second view (180 degrees about the vertical through the palm) that differ between the right origins and origin 0, of all its rows, measured on the cases of
# test_the_origin_matters; the assertion asks for more than half
MEASURED_WRONG_ORIGIN = {("hand17", 37, 29): (390, 440), ("hand17", 80, 60): (1896, 2023), ("hand26", 37, 29): (56, 82)}


@pytest.fixture(scope="module")
def oracles():
    made = {}

    def get(name):
        if name not in made:
            made[name] = ol.Oracle(None, ji.model_path(name))
        return made[name]
    yield get
    for o in made.values():
        o.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fraction", [1, 4])
def test_identity_views_are_the_references_pointcloud(w, h, fraction):
    """deprojection, range and ranking: takesubsample(PointCloud(dimage, {0.1, hi}), fraction) (misc_image.h:409-417, physmodel.h:58-64) per view, bit for bit"""
    L = ol.lib()
    sc = vr.two_view_scene("hand17", (0, 5), w, h, degrees=180.0)
    cam = vr.frame_camera(w, h)
    for b in range(2):
        for v in range(2):
            d = np.ascontiguousarray(sc["depth"][b, v])
            got, kept = vr.view_cloud(d, cam, None, 0.1, 0.65, fraction, 0.02)
            want = np.zeros((w * h, 3), np.float32); nfull = C.c_int(0)
            ocam = ol.camera(cam, w, h)
            n = L.ho_pointcloud(ol.u16ptr(d.reshape(-1)), C.byref(ocam), 0.1, 0.65, fraction, ol.f3ptr(want), w * h, C.byref(nfull))
            assert n == len(got) == (kept + fraction - 1) // fraction and n > 20, (b, v, n, len(got))
            assert np.array_equal(_bits(got[:, :3]), _bits(want[:n])) and not got[:, 3].any()
    # the fused cloud of identity views is their clouds one after the other, the second view's source 2
    f = vr.fuse(sc["depth"], np.tile(cam, (2, 2, 1)), None, 0.1, 0.65, fraction)
    a, b = vr.view_cloud(sc["depth"][1, 0], cam, None, 0.1, 0.65, fraction, 0.02)[0], vr.view_cloud(sc["depth"][1, 1], cam, None, 0.1, 0.65, fraction, 0.02, v=1)[0]
    assert np.array_equal(_bits(f["points"][1]), _bits(np.concatenate([a, b]))) and f["per_source"][1].tolist() == [len(a), 0, len(b), 0] and (b[:, 3] == 2).all()


@pytest.mark.parametrize("w,h", SIZES)
def test_every_source_has_points(w, h):
    sc = vr.two_view_scene("hand17", (0, 3, 9), w, h, degrees=180.0)
    f = vr.fuse(sc["depth"], sc["cams"], None, 0.1, 0.65, 1)
    assert (f["per_source"][:, [0, 2]] > 20).all() and not f["per_source"][:, [1, 3]].any()      # two cameras, no mirror: the direct sources
    assert (f["origins"][:, 0] == 0).all() and (np.abs(f["origins"][:, 2]).max(axis=1) > 0.3).all()      # the second camera sits beyond the hand
    # the posed view's points lie on the far side of the same hand in tracking space: each within the hand's thickness (the forearm's 8 cm at most) of a view-0 point
    for b in range(3):
        p = f["points"][b]; first, second = p[p[:, 3] == 0][:, :3].astype(np.float64), p[p[:, 3] == 2][:, :3].astype(np.float64)
        near = np.sqrt(((second[:, None] - first[None]) ** 2).sum(-1)).min(axis=1)
        print("frame %d: second-view points at most %.3f m from a view-0 point" % (b, near.max()))
        assert near.max() < 0.08
    ms = vr.mirror_scene("hand17", (0, 3), w, h)
    g = vr.fuse(ms["depth"], ms["cams"], ms["planes"], 0.1, 0.9, 1)
    assert (g["per_source"] > 20).all() and g["per_source"].shape == (2, 2)      # one camera and its mirror: both sources
    for b in range(2):
        p = g["points"][b]
        assert (p[:, 2] < 0.5).all()      # the virtual hand's points come back in front of the mirror
        assert np.array_equal(g["origins"][b, 1], np.array([0, 0, 1.0], np.float32)) and not g["origins"][b, 0].any()      # the camera's image: 2 x 0.5 m down the axis
        assert (np.diff(np.flatnonzero(p[:, 3] == 1)) > 1).any()      # direct and mirrored points interleave within the view


def _case(name, w, h, frames=(0, 3), lag=1):
    sc = vr.two_view_scene(name, frames, w, h, degrees=180.0)
    f = vr.fuse(sc["depth"], sc["cams"], None, 0.1, 0.65, 1)
    return sc, f, ki.states_of(ki.truths(name)[[(i + lag) % len(ki.truths(name)) for i in frames]])      # lag 1: the pose a frame stale


def test_rows_are_cloud_constraints_from_each_points_origin(oracles):
    orc = oracles("hand17")
    sc, f, state = _case("hand17", 37, 29)
    micro, weak = 3.0, 0.4
    for b in range(2):
        pts, org = f["points"][b], f["origins"][b]
        got = vr.rows(ol, orc, 0, state[b], pts, org, micro, weak)
        orc.set_state(0, state[b]); m = orc.model(0)
        for i in (0, len(pts) // 3, len(pts) - 1):
            r = ol.linears_to_array((ol.Linear * 1)(orc.L.ho_cloud_constraint(m, ol.v3(pts[i, :3]), ol.v3(org[int(pts[i, 3])]))), 1)[0]
            k = np.float32(weak if r[1] <= 2 else 1.0)
            r[13], r[14] = np.float32(-1.0) * k * np.float32(micro), np.float32(1.0) * k * np.float32(micro)
            assert np.array_equal(_bits(got[i]), _bits(r)), i
        assert (got[:, 0] == -1).all() and (got[:, 1] >= 0).all() and (got[:, 1] < 17).all() and np.array_equal(got[:, 2:5], pts[:, :3])
        assert set(np.unique(np.abs(got[:, 13:15]))) <= {np.float32(3.0), np.float32(0.4) * np.float32(3.0)}


@pytest.mark.parametrize("name,w,h", sorted(MEASURED_WRONG_ORIGIN))
def test_the_origin_matters(oracles, name, w, h):
    """The second camera stands on the far side of the hand: its points face away from view 0's origin and towards their own camera.  Judged from origin 0, CloudConstraint
    takes them for points behind the body (dot(v - origin, n) > 0) and casts ConvexHitCheck through the hand: most of the second view's rows differ.  With the model
    at the frames' own ground truth, where "faces away" is the rendered surface's own statement."""
    orc = oracles(name)
    sc, f, state = _case(name, w, h, lag=0)
    differ = total = 0
    for b in range(2):
        pts, org = f["points"][b], f["origins"][b]
        right = vr.rows(ol, orc, 0, state[b], pts, org, 3.0, 0.4)
        wrong = vr.rows(ol, orc, 0, state[b], pts, org, 3.0, 0.4, wrong="origin0")
        second = pts[:, 3] == 2
        assert np.array_equal(_bits(right[~second]), _bits(wrong[~second]))      # view 0's rows do not depend on it
        d = (_bits(right[second]) != _bits(wrong[second])).any(axis=1)
        differ += int(d.sum()); total += int(second.sum())
    print("%s %dx%d: %d of %d second-view rows differ with origin 0" % (name, w, h, differ, total))
    assert total > 40 and 2 * differ > total
