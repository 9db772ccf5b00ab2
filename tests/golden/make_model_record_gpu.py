"""Writes tests/golden/model_record_gpu.json: what a context of either hand model answers as created, after ht_scale(1.15) and after ht_scale(0.9) on top (hashes of
the three renderers' frames, the keypoint tables, joint coordinates, sampled poses, staged contacts and, for the 17-bone hand, one update of four golden frames), and
what ht_create answers to the files it refuses (tests/model_record_cases.py).

    python tests/golden/make_model_record_gpu.py [out.json]      (on the MI355X, with the library of the commit to record)

The recording was made once, twice over with equal results, from the commit before ht_create and ht_model_open were rebuilt on one host record of a model;
tests/test_gpu_model_record.py compares against it and never records.  The script uses the Python API alone, so it runs unchanged on any commit that has these calls."""
import json
import os
import sys
import tempfile

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TESTS)); sys.path.insert(0, TESTS)
import model_record_cases as M      # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else M.GPU_RECORDING
    with tempfile.TemporaryDirectory() as tmp:
        first, second = M.gpu_recording(tmp), M.gpu_recording(tmp)
    assert first == second, "two recordings of one library differ"
    with open(out, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d models x %d states, %d refusals" % (out, len(first["models"]), len(M.GPU_STATES), len(first["refusals"])))
