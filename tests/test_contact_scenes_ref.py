"""The contact scenes of tests/contact_scenes.py on the CPU: the generator still makes the scenes the fixtures were made from, the C restatement (oracle/ho_gjk.c) equals
the reference's answers to them bit for bit, and the mix holds what the scenes are there for -- penetrating pairs, pairs at the cut-off, polytopes beyond one 64-triangle
stride, exact candidate counts, patches of several samples, frames beyond the solver's 96-contact tables and beyond the device's pool of 192.  No GPU."""
import numpy as np
import pytest

import contact_oracle as co
import contact_scenes as cs

PAIR = [f for f in cs.FAMILIES if cs.FAMILIES[f][3] == "pair"]
WHOLE = [f for f in cs.FAMILIES if cs.FAMILIES[f][3] == "whole"]
EPA_MAXV, EPA_MAXT, EPA_MAXIT = 96, 192, 128      # what the device's polytope holds (csrc/ht_gjk.hip)


@pytest.mark.parametrize("family", list(cs.FAMILIES))
def test_generator_still_makes_the_fixture_scenes(family):
    fx = co.fixture(family)
    scenes = cs.compact(family)
    assert scenes.dtype == np.float32 and np.array_equal(scenes, fx["scenes"])
    st = cs.states(family, scenes)
    assert st.shape == (len(scenes), cs.model_of(family).nb, 13) and not st[:, :, 7:].any()
    assert np.array_equal(cs.digest(st), fx["digest"])
    assert fx["left_out"].sum() * 100 <= len(scenes)      # at most 1 % of the drawn scenes may be missing a reference answer


@pytest.mark.parametrize("family", PAIR)
def test_restatement_equals_reference_on_pairs(family):
    fx, got = co.fixture(family), co.restate(family)
    ref = co.reference_contacts(family)
    for k in co.kept(family):
        assert np.array_equal(got["answers"][k], fx["pair_out"][k]), "%s scene %d: Separated / ContactPatch" % (family, k)
        # FindShapeShapeContacts reports the patch, or nothing where its sphere test drops the pair
        assert fx["pair_scene_n"][k] in (0, int(fx["pair_out"][k, 10]))
        want = ref[k] if fx["pair_scene_n"][k] else ref[k][:0]
        assert np.array_equal(got["contacts"][k], want), "%s scene %d: contact list" % (family, k)


@pytest.mark.parametrize("family", WHOLE)
def test_restatement_equals_reference_on_whole_scenes(family):
    got, ref = co.restate(family), co.reference_contacts(family)
    for k in co.kept(family):
        assert len(got["contacts"][k]) == len(ref[k]), "%s scene %d: %d contacts, the reference has %d" % (family, k, len(got["contacts"][k]), len(ref[k]))
        assert np.array_equal(got["contacts"][k], ref[k]), "%s scene %d" % (family, k)


def test_mix_penetrating_pairs():
    ans = co.restate("a")["answers"]
    pen = int((ans[:, 9] <= 0).sum())
    print("family a: %d scenes, %d penetrating, %d touching, %d apart" % (len(ans), pen, int(((ans[:, 10] > 0) & (ans[:, 9] > 0)).sum()), int((ans[:, 10] == 0).sum())))
    assert pen >= 300


def test_mix_cutoff_pairs():
    n = np.array([len(c) for c in co.restate("b")["contacts"]]).reshape(-1, 2)
    d = co.fixture("b")["distances"]
    differ = int((n[:, 0] != n[:, 1]).sum())
    ans = co.restate("b")["answers"]
    broad = int(((ans[0::2, 10] > 0) & (ans[1::2, 10] > 0) & (n[:, 1] == 0)).sum())      # the patch is still there, the sphere test has dropped the pair
    print("family b: %d draws, %d with a contact at one distance and none at the next float32, %d of them ended by the broad phase" % (len(n), differ, broad))
    assert differ >= 100
    assert np.all((d[:, 0] == d[:, 1]) | (np.nextafter(d[:, 0], np.float32(1)) == d[:, 1]))
    assert broad >= 5


def test_mix_polytope_sizes():
    worst = {}
    for family in cs.FAMILIES:
        runs, mv, mt, mi, peak = co.restate(family)["epa"]
        worst[family] = (runs, mv, mt, mi, peak)
        print("family %s: %d polytope runs, at most %d vertices, %d triangles at a face search, %d held at once, %d face searches" % (family, runs, mv, mt, peak, mi))
        assert mv <= EPA_MAXV and peak <= EPA_MAXT and mi <= EPA_MAXIT, family      # no device capacity is in play
    assert worst["c"][2] > 64      # the face search's second stride of 64 triangles really runs


@pytest.mark.parametrize("family", ["d17", "d26"])
def test_mix_candidate_counts(family):
    poses, want = cs.family_d(family)
    M = cs.model_of(family)
    got = [len(cs.candidates(M, p)) for p in poses]
    assert got == list(cs.CANDIDATES[family]) == list(want)
    # every candidate of these scenes overlaps deeply: the restatement reports one contact per candidate pair, so the restated broad phase is the oracle's
    assert [len(c) for c in co.restate(family)["contacts"]] == got


def test_mix_patches():
    ans = co.restate("f")["answers"]
    cnt = ans[:, 10].astype(int)
    print("family f: samples per patch %s" % np.bincount(cnt, minlength=6).tolist())
    assert int((cnt >= 2).sum()) >= 30


def test_mix_cluster_contacts():
    n = np.array([len(c) for c in co.restate("e26")["contacts"]])
    sig = cs.family_e("e26")[1]
    print("family e26: contacts at sigma 10 mm %s, at 5 mm %s" % (n[sig == 10].tolist(), n[sig == 5].tolist()))
    assert np.all((n[sig == 10] > 96) & (n[sig == 10] <= 192))
    assert np.all(n[sig == 5] > 192)
    n17 = np.array([len(c) for c in co.restate("e17")["contacts"]])
    print("family e17: contacts %s" % n17.tolist())
    assert n17.max() <= 96
