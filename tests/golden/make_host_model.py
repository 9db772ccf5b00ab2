"""Writes tests/golden/host_model.json: the host view of every model of tests/model_record_cases.py in every state (hashes of every getter, of the two ray casts
and of the two renderers' definitions) and what ht_model_open answers to the files it refuses.

    python tests/golden/make_host_model.py [out.json]      (no GPU; with the library of the commit to record)

The recording was made once, twice over with equal results, from the commit before ht_create and ht_model_open were rebuilt on one host record of a model;
tests/test_host_model_record.py compares against it and never records.  The script uses the Python API alone, so it runs unchanged on any commit that has ht_model_*."""
import json
import os
import sys
import tempfile

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TESTS)); sys.path.insert(0, TESTS)
import model_record_cases as M      # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else M.HOST_RECORDING
    with tempfile.TemporaryDirectory() as tmp:
        first, second = M.host_recording(tmp), M.host_recording(tmp)
    assert first == second, "two recordings of one library differ"
    with open(out, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d models x %d states, %d refusals" % (out, len(first["models"]), len(M.STATES), len(first["refusals"])))
