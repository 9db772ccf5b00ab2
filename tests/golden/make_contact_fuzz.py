"""Makes tests/golden/contact_fuzz_<family>.htfx: the scenes of tests/contact_scenes.py in compact form, a digest of their full states and the reference's own answers
(oracle/_ref/ref_harness contacts ..., built by `make -C oracle ref` where the reference tree is present).  Family b's distances are bisected here with the C restatement;
every other number comes from the generator or from the reference.

    python tests/golden/make_contact_fuzz.py [family ...]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import contact_oracle as co      # noqa: E402
import contact_scenes as cs      # noqa: E402
import htfx                      # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
REF_MODEL = {"hand17": ("hand", None), "hand26": ("hand", os.path.join(ROOT, "oracle", "_ref", "model_hand26.json")), "chain3": (os.path.join(HERE, "model_chain3.json"), None)}


def reference(family, scenes, tmp):
    name, scale, clear, kind = cs.FAMILIES[family]
    arrays = {"pairs" if kind == "pair" else "poses": scenes}
    if clear:
        arrays["clear_ignore"] = np.array(clear, np.int32)
    fin, fout = os.path.join(tmp, family + "_in.htfx"), os.path.join(tmp, family + "_out.htfx")
    htfx.save(fin, arrays)
    model, json26 = REF_MODEL[name]
    env = dict(os.environ)
    if json26:
        env["HT_REF_MODEL_JSON"] = json26
    subprocess.check_call([HARNESS, "contacts", model, repr(scale), fin, fout], env=env)
    return htfx.load(fout)


def make(family, tmp):
    kind = cs.FAMILIES[family][3]
    out = {}
    if family == "b":
        orc = co.open_oracle("b")
        nb = cs.model_of("b").nb
        out["distances"] = cs.bisect_cutoffs(lambda case: len(co.find_contacts(orc, cs.pair_states(case[None], nb)[0])))
        orc.close()
        scenes = cs.family_b(out["distances"])
    else:
        scenes = cs.compact(family)
    ref = reference(family, scenes, tmp)
    out["scenes"] = scenes
    out["digest"] = cs.digest(cs.states(family, scenes))
    if kind == "pair":
        out["left_out"] = ref["pair_failed"]; out["pair_out"] = ref["pair_out"]; out["pair_scene_n"] = ref["pair_scene_n"]
    else:
        out["left_out"] = ref["scene_failed"]; out["scene_n"] = ref["scene_n"]; out["scene_contacts"] = ref["scene_contacts"][:int(ref["scene_n"].sum())] if ref["scene_n"].sum() else ref["scene_contacts"][:0]
        if family.startswith("d"):
            out["candidates"] = cs.family_d(family)[1]
        else:
            out["sigma_mm"] = cs.family_e(family)[1]
    assert out["left_out"].sum() * 100 <= len(scenes), "the reference failed on more than 1 %% of family %s" % family
    path = cs.fixture_path(family)
    htfx.save(path, out)
    print("%s: %d scenes, %d left out, %d bytes" % (family, len(scenes), int(out["left_out"].sum()), os.path.getsize(path)))


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        for fam in (sys.argv[1:] or list(cs.FAMILIES)):
            make(fam, tmp)
