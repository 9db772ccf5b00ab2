"""A context answers what it answered before ht_create and ht_model_open were rebuilt on one host record of a model: for both hand models as created, after
ht_scale(1.15) and after ht_scale(0.9) on top, the three renderers' frames with body labels, the keypoint tables, sampled poses, joint coordinates, staged contacts
(the padded collision vertices, HT_BC_DIAM) and, for the 17-bone hand, one update of four golden frames; and the refusals of ht_create, word for word.
tests/golden/model_record_gpu.json was recorded on the MI355X from the commit before (tests/golden/make_model_record_gpu.py); nothing here records.  In every state
the mesh renderers' frames also equal the host model's in the same state, bit for bit."""
import json

import numpy as np
import pytest

import model_record_cases as M
from hand_tracking_samples_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recording():
    with open(M.GPU_RECORDING) as f:
        return json.load(f)


@pytest.mark.parametrize("name", M.GPU_MODELS)
def test_context_answers_what_it_did_in_every_state(recording, name):
    host = native.HostModel(M.MODELS[name])

    def check(state, ctx, rest, golden):
        want = recording["models"][name][state]
        got = M.gpu_state(ctx, rest, golden)
        assert sorted(got) == sorted(want)
        for k in sorted(want):
            assert got[k] == want[k], "%s %s: %s differs from the recording" % (name, state, k)
        assert min(want["labelled"]) > 0 and want["ncontacts"][2] > 0      # the frames see the hand, the squeezed hand touches itself
        factor = dict(M.GPU_STATES)[state]
        if factor:
            host.scale(factor)
        poses = M.gpu_poses(ctx, rest); frames = M.gpu_frames(ctx, poses)
        for entry, definition in (("render_mesh_depth", host.render_mesh), ("raster_mesh_depth", host.raster_mesh)):
            for k in range(len(poses)):
                d, b = definition(poses[k], M.cam(80), 80, 60)
                assert np.array_equal(frames[entry][0][k], d) and np.array_equal(frames[entry][1][k], b), "%s %s: %s of pose %d is not the host model's" % (name, state, entry, k)

    try:
        M.gpu_walk(name, check)
    finally:
        host.close()


def test_create_refuses_what_it_refused_in_the_same_words(recording, tmp_path):
    got = M.gpu_refusals(M.refusal_files(tmp_path))
    assert got == recording["refusals"]
    assert got["without_b0/tris"] == [0, ""]      # a context does without the hull triangles
    assert got["without_physics"][1] == "model entry missing: physics"
    assert got["bodies32"][1].startswith("model too large")
