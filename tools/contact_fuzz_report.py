"""profiles/contact_fuzz.json: the scene mix of tests/contact_scenes.py as the C restatement sees it (counts per family, polytope maxima) and, given the report a GPU run of
tests/test_gpu_contact_fuzz.py wrote (HT_CONTACT_FUZZ_REPORT=<file>), the scenes compared per kernel form, the mismatches, the capacity counters and the seconds per test.

    python tools/contact_fuzz_report.py [gpu_report.json] > profiles/contact_fuzz.json
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import contact_oracle as co      # noqa: E402
import contact_scenes as cs      # noqa: E402


def mix():
    out = {}
    for family, (model, scale, clear, kind) in cs.FAMILIES.items():
        r = co.restate(family)
        n = np.array([len(c) for c in r["contacts"]])
        runs, mv, mt, mi, peak = r["epa"]
        f = dict(model=model, scale=scale, kind=kind, scenes=len(n), reference_left_out=int(co.fixture(family)["left_out"].sum()), contacts_total=int(n.sum()), contacts_max=int(n.max()),
                 polytope=dict(runs=runs, max_vertices=mv, max_triangles_at_a_face_search=mt, max_triangles_held=peak, max_face_searches=mi))
        if kind == "pair":
            a = r["answers"]
            f.update(penetrating=int((a[:, 9] <= 0).sum()), touching_apart=int(((a[:, 10] > 0) & (a[:, 9] > 0)).sum()), no_contact=int((n == 0).sum()),
                     samples_per_patch=np.bincount(a[:, 10].astype(int), minlength=6).tolist())
        if family == "b":
            p = n.reshape(-1, 2)
            f.update(draws=len(p), draws_whose_two_scenes_differ=int((p[:, 0] != p[:, 1]).sum()),
                     ended_by_the_broad_phase=int(((a[0::2, 10] > 0) & (a[1::2, 10] > 0) & (p[:, 1] == 0)).sum()))
        if family.startswith("d"):
            f.update(candidate_pairs=[len(cs.candidates(cs.model_of(family), p)) for p in cs.family_d(family)[0]], contacts=n.tolist())
        if family.startswith("e"):
            f.update(sigma_mm=cs.family_e(family)[1].tolist(), contacts=n.tolist())
        out[family] = f
    return out


if __name__ == "__main__":
    rep = {"what": "tests/contact_scenes.py: scene mix and polytope maxima from the C restatement (oracle/ho_gjk.c, ho_epa_stats); gpu: tests/test_gpu_contact_fuzz.py on one MI355X",
           "device_capacities": dict(polytope_vertices=96, polytope_triangles=192, polytope_iterations=128, pool=192, patch_slots=40, solver_lds_contacts=96), "mix": mix()}
    if len(sys.argv) > 1:
        with open(sys.argv[1]) as f:
            runs = json.load(f)
        rep["gpu"] = dict(runs=runs, scenes_per_kernel={k: sum(r["scenes"] for r in runs if r["kernel"] == k) for k in sorted({r["kernel"] for r in runs})},      # "a+b": batches of several sizes, a form each
                          mismatches=sum(r["mismatches"] for r in runs), seconds_total=round(sum(r["seconds"] for r in runs), 3))
    json.dump(rep, sys.stdout, indent=1)
    print()
