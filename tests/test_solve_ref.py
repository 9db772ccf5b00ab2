"""The solver fuzz's references against each other, on the CPU: every scene of tests/solve_scenes.py through the fp32 restatement (ho_physics_update) and
through the float64 statement (tests/solve_ref.py).

E_ref(family, quantity) = max |oracle32 - f64| is the restatement's own rounding distance; BOUND = 8 x E_ref is what tests/test_gpu_solve_fuzz.py allows the device.
A bound is worth something only if a wrong solver misses it, so each mutant of the float64 statement (rows swapped, a post-sweep fewer, no RemoveBias on angular rows,
friction limits a sweep late, the last angular run gone) must move the result by more than 10 x BOUND, in some quantity, on at least half of the scenes it applies to,
family by family.  A family that cannot show that has slack rows: the generator is to be strengthened, never the threshold.

HT_SOLVE_FUZZ_REPORT=<file>: E_ref, the bounds and each mutant's median distance per family and quantity are merged into that JSON (profiles/solve_fuzz.json)."""
import json
import os

import numpy as np
import pytest

import solve_oracle as so
import solve_ref
import solve_scenes as ss

_ANGULAR, _FRICTION = ("angular", "mixed", "with_contacts", "crowded"), ("groups", "friction", "mixed", "with_contacts", "crowded")
MUTANTS = dict(swap=tuple(ss.FAMILIES), post=tuple(ss.FAMILIES), nobias=_ANGULAR, stale_friction=_FRICTION, drop_last_run=_ANGULAR)      # the families with rows each mutant changes
FLT_MAX = ss.FLT_MAX


def merge_report(section, family, values):
    path = os.environ.get("HT_SOLVE_FUZZ_REPORT")
    if not path:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {}
    if isinstance(values, dict):
        doc.setdefault(family, {}).setdefault(section, {}).update(values)
    else:
        doc.setdefault(family, {})[section] = values
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


def applies(mutant, sc, lin):
    """whether the mutant changes anything the scene computes"""
    ang = sc["ang"]
    if mutant == "swap":
        return ss.swap_index(sc, lin) >= 0
    if mutant == "post":
        return len(lin) + len(ang) > 0
    if mutant == "nobias":
        return bool(np.any(((ang[:, 6] < 0) & (ang[:, 5] != 0)) | ((ang[:, 6] >= 0) & (ang[:, 5] > 0))))
    if mutant == "stale_friction":
        return bool(np.any(lin[:, 15] != 0))
    if mutant == "drop_last_run":
        return len(ang) > 0 and bool(np.any(ang[solve_ref.angular_runs(ang)[-2]:, 5] != -FLT_MAX) or np.any(ang[solve_ref.angular_runs(ang)[-2]:, 6] < 0))
    raise KeyError(mutant)


@pytest.mark.parametrize("family", tuple(ss.FAMILIES))
def test_float64_statement_agrees_with_the_restatement(family):
    """The two references state the same computation: they differ by fp32 rounding and no more.  In units of FLT_EPSILON x the quantity's largest magnitude in the family
    the distance is 0.3 to 7 everywhere but on the quaternions of `crowded` (33: deep overlaps spin small bodies by radians per step); 64 is allowed.  A statement that
    applied a row differently would be off by a thousand such units and more (the mutants below)."""
    scenes = ss.scenes(family)
    assert (32 <= len(scenes) <= 64) or family == "chains_long"
    e, s64 = so.e_ref(family), so.restated(family)[1]
    units = {q: e[q] / (float(np.finfo(np.float32).eps) * np.abs(s64[:, :, sl]).max()) for q, sl in so.QUANTITIES}
    print("E_ref %s: %s; in FLT_EPSILON x magnitude: %s" % (family, {q: "%.2e" % v for q, v in e.items()}, {q: "%.1f" % v for q, v in units.items()}))
    merge_report("e_ref", family, e); merge_report("bound", family, so.bound(family)); merge_report("scenes", family, len(scenes))
    assert all(v > 0 for v in e.values()) and all(v <= 64 for v in units.values())


@pytest.mark.parametrize("family,mutant", [(f, m) for m, fams in MUTANTS.items() for f in fams])
def test_mutants_miss_the_bound(family, mutant):
    scenes = ss.scenes(family)
    _, s64, lins = so.restated(family)
    on = np.array([applies(mutant, sc, lin) for sc, lin in zip(scenes, lins)])
    assert on.any()
    arg = (mutant, [ss.swap_index(sc, lin) for sc, lin in zip(scenes, lins)]) if mutant == "swap" else (mutant,)
    d = so.distance(so.f64(family, arg), s64)
    bound = so.bound(family)
    shown = np.zeros(len(scenes), bool)
    for q, v in d.items():
        shown |= v > 10.0 * bound[q]
    med = {q: float(np.median(v[on])) for q, v in d.items()}
    print("%s / %s: %d of %d scenes beyond 10 x BOUND; median distance %s" % (family, mutant, int(shown[on].sum()), int(on.sum()), {q: "%.1e" % v for q, v in med.items()}))
    merge_report("mutant_median", family, {mutant: dict(med, scenes=int(on.sum()), beyond_10_bound=int(shown[on].sum()))})
    assert not shown[~on].any()      # where it does not apply it changes nothing
    assert 2 * int(shown[on].sum()) >= int(on.sum())


def test_families_reach_their_edges():
    """what the issue lists per family is really in the scenes"""
    def groups(f): return [ss.tail_groups(sc["lin"]) for sc in ss.scenes(f)]
    per_body = {int(c) for sc in ss.scenes("chains") for c in np.bincount(sc["lin"][:, 1].astype(int), minlength=17)}
    assert per_body >= set(ss.COUNTS)
    assert any(np.bincount(sc["lin"][:, 1].astype(int), minlength=26)[16:].min() > 0 for sc in ss.scenes("chains26"))
    assert sorted({len(sc["lin"]) for sc in ss.scenes("chains_long")}) == [ss.POINT_CAPACITY + 1, ss.POINT_CAPACITY + 65]
    assert {g for _, g in groups("groups")} >= {1, 8, 9, 31, 32} and max(g for _, g in groups("groups")) == ss.MAX_GROUPS
    assert any(p > 0 and g > 0 for p, g in groups("groups"))
    assert any(np.any(sc["lin"][ss.tail_groups(sc["lin"])[0]:, 0] < 0) for sc in ss.scenes("groups"))      # rb0 == NULL in the tail
    assert sorted(int(np.sum(sc["lin"][:, 15] == -1)) for sc in ss.scenes("friction")) == list(range(1, 33))
    runs = {ss.angular_runs(sc["ang"]) for sc in ss.scenes("angular")}; rows = {len(sc["ang"]) for sc in ss.scenes("angular")}
    assert runs >= {1, 8, 9, 63, 64, 65, 125, 126} and rows >= {124, 125, 126} and max(rows) == ss.MAX_ANGULAR      # a caller's list ends at 126 rows: beyond, the call is refused
    assert any(sc["switched"] for sc in ss.scenes("angular")) and any(not sc["switched"] and np.any(sc["ang"][:, 5] == -FLT_MAX) for sc in ss.scenes("angular"))
    wc = ss.scenes("with_contacts")
    assert any(sc["tail"] for sc in wc) and any(not sc["tail"] for sc in wc) and not any(sc["switched"] for sc in wc)
    assert all(len(lin) > len(sc["lin"]) for sc, lin in zip(wc, so.restated("with_contacts")[2]))      # every scene really has contacts
    total = [ss.tail_groups(lin)[1] for lin in so.restated("crowded")[2]]                                 # the caller's groups and the contact triples of a frame
    assert {64, 65} <= set(total) and max(total) > 96 and min(total) <= 32
    assert [(len(sc["ang"]), ss.angular_runs(sc["ang"])) for sc in ss.too_many_angular()] == [(127, 127), (253, 127), (300, 100), (129, 129), (200, 200)]
    for f in tuple(ss.FAMILIES):
        for sc in ss.scenes(f):
            assert len(sc["ang"]) <= ss.MAX_ANGULAR and ss.tail_groups(sc["lin"])[1] <= ss.MAX_GROUPS
            assert np.all(sc["lin"][:, 0] != sc["lin"][:, 1]) and np.all(sc["ang"][:, 0] != sc["ang"][:, 1])
            assert np.allclose(np.linalg.norm(sc["lin"][:, 8:11], axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(sc["ang"][:, 2:5], axis=1), 1, atol=1e-6)
            assert np.all(np.linalg.norm(sc["lin"][:, 2:5], axis=1) <= 0.02) and np.all(np.linalg.norm(sc["lin"][:, 5:8], axis=1) <= 0.02)


def test_profile_is_committed():
    """profiles/solve_fuzz.json holds, per family and quantity, E_ref, the bound and each mutant's median distance (and the device's measured ratio, from the GPU run)"""
    doc = json.load(open(os.path.join(ss.HERE, "..", "profiles", "solve_fuzz.json")))
    for f in tuple(ss.FAMILIES):
        assert set(doc[f]["e_ref"]) == set(doc[f]["bound"]) == {q for q, _ in so.QUANTITIES}
        for q, v in doc[f]["e_ref"].items():
            assert doc[f]["bound"][q] == pytest.approx(so.FACTOR * v)
