"""Writes tests/golden/update_entries.json: what every update entry point launches (profile scope -> launches, per frame kind) and what it answers to every fault of
tests/update_entries_cases.py (return code, ht_last_error).

    python tests/golden/make_update_entries.py      (on the MI355X, with the library of the commit to record)

The recording was made once, from the commit before the entry points were rewritten around one request record; tests/test_gpu_update_entries.py compares against
it and never records.  The script uses the Python API alone, so it runs unchanged on any commit that has these entry points."""
import json
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TESTS)); sys.path.insert(0, TESTS)
import update_entries_cases as U      # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else U.RECORDING
    env = U.Env()
    try:
        rec = {"launches": {e: U.launch_counts(env, e) for e in U.ENTRIES}, "faults": {e: U.run_faults(env, e) for e in U.ENTRIES}}
    finally:
        env.close()
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d good calls, %d faults" % (out, sum(len(v) for v in rec["launches"].values()), sum(len(v) for v in rec["faults"].values())))
