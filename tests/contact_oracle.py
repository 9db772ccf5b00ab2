"""The C restatement's side of the contact scenes (tests/contact_scenes.py): one oracle per family's (model, scale), its contact lists and pair answers, and
the families' fixtures (tests/golden/contact_fuzz_*.htfx, made by tests/golden/make_contact_fuzz.py from the reference's own answers)."""
import os
import tempfile

import numpy as np

import contact_scenes as cs
import htfx
import oracle_lib as ol

DRIFTMAX = np.float32(0.03 / 8.0)      # physics_driftmax as the tracker sets it (handtrack.h:837-838)
_tmp = None


def model_path(family):
    """the family's model file; one with the family's pairs taken off the ignore lists is written to a temporary directory"""
    global _tmp
    name, _, clear, _ = cs.FAMILIES[family]
    if not clear:
        return cs.MODELS[name]
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="contact_fuzz_")
    path = os.path.join(_tmp.name, "%s_%s.htfx" % (name, "_".join("%d-%d" % p for p in clear)))
    if not os.path.exists(path):
        m = dict(htfx.load(cs.MODELS[name]))
        ign = m["ignore"].copy()
        for i, j in clear:
            ign[i, j] = ign[j, i] = 0
        m["ignore"] = ign
        htfx.save(path, m)
    return path


def open_oracle(family):
    orc = ol.Oracle(None, model=model_path(family))
    scale = cs.FAMILIES[family][1]
    if scale != 1.0:
        orc.L.ho_scale(orc.h, scale)
    return orc


def find_contacts(orc, state, cap=512):
    """ho_find_contacts on one state [nb, 13] -> [k, 12]: rb0 rb1 normal p0w p1w separation, the rows stage_contacts returns"""
    orc.set_state(0, state)
    buf = (ol.Contact * cap)()
    k = orc.L.ho_find_contacts(orc.h, orc.model(0), buf, cap)
    assert k < cap
    return np.array([[x.rb0, x.rb1, x.normal.x, x.normal.y, x.normal.z, x.p0w.x, x.p0w.y, x.p0w.z, x.p1w.x, x.p1w.y, x.p1w.z, x.separation] for x in buf[:k]], np.float32).reshape(k, 12)


def pair_answer(orc, state, a, b):
    """the 46 numbers S13 of the reference harness keeps of a pair: Separated's normal p0w p1w separation, ContactPatch's count and up to five (p0w p1w separation)"""
    orc.set_state(0, state)
    m = orc.model(0)
    pa, pb = orc.L.ho_body_ptr(m, a), orc.L.ho_body_ptr(m, b)
    h = orc.L.ho_separated_bodies(pa, pb)
    out = np.zeros(46, np.float32)
    out[:10] = [h.normal.x, h.normal.y, h.normal.z, h.p0w.x, h.p0w.y, h.p0w.z, h.p1w.x, h.p1w.y, h.p1w.z, h.separation]
    hits = (ol.GjkContact * 5)()
    cnt = orc.L.ho_contact_patch_bodies(pa, pb, DRIFTMAX, hits)
    out[10] = cnt
    for k in range(cnt):
        out[11 + 7 * k:18 + 7 * k] = [hits[k].p0w.x, hits[k].p0w.y, hits[k].p0w.z, hits[k].p1w.x, hits[k].p1w.y, hits[k].p1w.z, hits[k].separation]
    return out


def contacts_of_pair_answer(case, ans):
    """the contact rows FindShapeShapeContacts makes of a pair's patch (a < b): every sample carries the first one's normal (gjk.h:633)"""
    n = int(ans[10])
    out = np.zeros((n, 12), np.float32)
    for k in range(n):
        out[k] = np.concatenate([case[:2], ans[0:3], ans[11 + 7 * k:18 + 7 * k]])
    return out


def rest_pose(family):
    """the model's rest pose [nb, 7]"""
    return htfx.load(cs.MODELS[cs.FAMILIES[family][0]])["rest_state"][:, :7].copy()


_fixtures = {}


def fixture(family):
    if family not in _fixtures:
        _fixtures[family] = htfx.load(cs.fixture_path(family))
    return _fixtures[family]


def kept(family):
    """indices of the family's scenes the reference answered (the others are listed in the fixture's left_out)"""
    return np.flatnonzero(fixture(family)["left_out"] == 0)


def reference_contacts(family):
    """per scene the reference's contact rows [k, 12] (None where it was left out)"""
    fx = fixture(family)
    scenes = fx["scenes"]
    out = []
    if cs.FAMILIES[family][3] == "pair":
        for k in range(len(scenes)):
            out.append(None if fx["left_out"][k] else contacts_of_pair_answer(scenes[k], fx["pair_out"][k]))
    else:
        off = np.concatenate([[0], np.cumsum(fx["scene_n"])])
        for k in range(len(scenes)):
            out.append(None if fx["left_out"][k] else fx["scene_contacts"][off[k]:off[k + 1]].reshape(-1, 12))
    return out


_restated = {}


def restate(family):
    """the restatement on every scene of the family, once per process: dict(contacts=[rows [k, 12] per scene], answers=[n, 46] (pair families), epa=(runs, max_verts,
    max_tris, max_iterations, peak_tris) over the family)"""
    if family not in _restated:
        orc = open_oracle(family)
        try:
            st = cs.states(family)
            ol.epa_stats(reset=True)
            out = {"contacts": [find_contacts(orc, s) for s in st]}
            if cs.FAMILIES[family][3] == "pair":
                scenes = cs.compact(family)
                out["answers"] = np.stack([pair_answer(orc, st[k], int(scenes[k, 0]), int(scenes[k, 1])) for k in range(len(st))])
            out["epa"] = ol.epa_stats(reset=True)
        finally:
            orc.close()
        _restated[family] = out
    return _restated[family]
