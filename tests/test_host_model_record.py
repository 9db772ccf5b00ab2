"""The host view of a model (ht_model_*) answers what it answered before ht_model_open and ht_create were rebuilt on one host record of a model: every getter, the two
ray casts and the two renderers' definitions, for three models (two baked, one through the JSON builder) as opened, scaled, mirrored and in both orders of the two,
and the refusals of ht_model_open, word for word.  tests/golden/host_model.json was recorded from the commit before (tests/golden/make_host_model.py); nothing here
records."""
import json

import pytest

import model_record_cases as M
from hand_tracking_samples_amd import native


@pytest.fixture(scope="module")
def recording():
    with open(M.HOST_RECORDING) as f:
        return json.load(f)


@pytest.mark.parametrize("state", list(M.STATES))
@pytest.mark.parametrize("name", list(M.MODELS))
def test_host_model_answers_what_it_did(recording, name, state):
    m = M.bring(native.HostModel(M.MODELS[name]), state)
    try:
        got = M.host_state(m)
    finally:
        m.close()
    want = recording["models"][name][state]
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], "%s %s: %s differs from the recording" % (name, state, k)
    assert min(want["hits"]) > 0      # the segments and frames see the model


def test_open_refuses_what_it_refused_in_the_same_words(recording, tmp_path):
    got = M.host_refusals(M.refusal_files(tmp_path))
    assert got == recording["refusals"]
    assert got["without_physics"] == [0, ""] and got["without_b0/tris"][0] != 0      # the host view does without the physics constants, not without the hull triangles
