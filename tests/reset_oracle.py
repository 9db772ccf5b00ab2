"""The reset fuzz's two references side by side on the scenes of tests/reset_scenes.py: the fp32 restatement (ho_pose_from_scratch, ho_unibody_fit, with the float sin / cos
rounded once from double as the device forms them) and the float64 statement (tests/reset_ref.py).  From them the yardsticks of tests/test_reset_ref.py and
tests/test_gpu_reset_fuzz.py:

    E_ref(quantity, family, k) = max |fp32 round k - float64 round k|, both started from the fp32 state before round k with the fp32 rows made at that state: the
        restatement's own rounding distance over ONE round.
    S(quantity, family, k), k = 2, 3: the fp32 state before round k moved by E_ref(k - 1) in each of four seeded sign patterns, the fp32 round run from there; the largest
        movement of the result.  What a difference of rounding size after one round is allowed to become in the next, measured on the restatement alone.
    A scene whose own sensitivity exceeds 100 x its family's median has had a closest-body choice flipped by the nudge: it leaves the comparisons of rounds >= k.

Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as ol
import reset_ref
import reset_scenes as rs

# position and quaternion: of the model's bodies (and of the proxy body, which says the same); momenta: the proxy body's after its PhysicsUpdate, post sweeps included.
# UnibodyFit drops them, so they exist on the two references alone; the model's own momenta are zero after PoseFromScratch and no round touches them.
QUANTITIES = (("position", slice(0, 3)), ("quaternion", slice(3, 7)), ("momenta", slice(7, 13)))
FACTOR = 8.0          # as tests/solve_oracle.py: the product applies the same rows in the same order with the same clamps and differs in association only
ROUNDS = 3            # steps_unibody of the reference
DIRECTIONS = 4
FLIP = 100.0
F = np.float32


class _Oracles:
    """one tracker per model file, the restatement's float functions rounded once while open"""

    def __enter__(self):
        self.orc = {}
        ol.lib().ho_set_round_once(1)
        return self

    def __exit__(self, *a):
        ol.lib().ho_set_round_once(0)
        for o in self.orc.values():
            o.close()

    def of(self, sc):
        if sc["model"] not in self.orc:
            self.orc[sc["model"]] = ol.Oracle(model=rs.model_path(sc["model"]))
        o = self.orc[sc["model"]]
        o.head.phys.unibody_force = sc["unibody_force"]
        return o


def _pts(sc):
    return np.ascontiguousarray(np.concatenate([sc["cloud"], np.zeros((1, 3), F)]))      # never empty


def analysis_struct(an):
    assert C.sizeof(ol.Analysis) == 84 * 4
    return ol.Analysis.from_buffer_copy(np.ascontiguousarray(an, F).tobytes())


def pose_from_scratch(o, sc):
    an = analysis_struct(sc["analysis"]); cam = ol.camera(sc["cam"])
    o.reset(sc["start"])
    o.L.ho_pose_from_scratch(o.h, o.model(1), ol.f3ptr(_pts(sc)), sc["n"], C.byref(an), cam.pose)
    return o.get_state(1)


def unibody_fit(o, sc, state):
    """one round from `state` ([nb,13], or what this returns) -> [nb + 1,13]: the model's bodies, and behind them the proxy body as its PhysicsUpdate left it"""
    proxy = np.zeros((1, 13), F)
    o.set_state(1, state[:o.nb])
    o.L.ho_unibody_fit_proxy(o.h, o.model(1), ol.f3ptr(_pts(sc)), sc["n"], ol.v3(sc["cam"][5:8]), ol.fptr(proxy))
    return np.concatenate([o.get_state(1), proxy])


def rows(o, sc, state, first=0):
    """UnibodyFit's rows at `state` (handtrack.h:457: CloudConstraint of every 4th point from the camera's position) -> [nr,16]; first: the subsample's first point"""
    o.set_state(1, state[:o.nb])
    m = o.model(1); origin = ol.v3(sc["cam"][5:8])
    idx = range(first, sc["n"], 4)
    lin = (ol.Linear * max(1, len(idx)))()
    for k, i in enumerate(idx):
        lin[k] = o.L.ho_cloud_constraint(m, ol.v3(sc["cloud"][i]), origin)
    return ol.linears_to_array(lin, len(idx))


@functools.lru_cache(None)
def chain():
    """the restatement's states of every scene: [scene][k] after PoseFromScratch (k = 0, [nb,13]) and k rounds of UnibodyFit ([nb + 1,13], unibody_fit), float32"""
    out = []
    with _Oracles() as O:
        for sc in rs.scenes():
            o = O.of(sc)
            st = [pose_from_scratch(o, sc)]
            for _ in range(ROUNDS):
                st.append(unibody_fit(o, sc, st[-1]))
            out.append(st)
    return out


_F64 = {}      # (k, mutant) -> [state per scene]


def prepare(ks, mutants=()):
    """round k of every scene in float64, from the restatement's state before it on the restatement's rows there, for every k of `ks`; and round 1 under each of
    `mutants`.  Everything missing is solved in ONE batched PhysicsUpdate: its cost is that of the longest cloud, whatever the number of frames."""
    jobs = [j for j in [(k, None) for k in ks] + [(1, m) for m in mutants] if j not in _F64]
    if not jobs:
        return
    scs, ch = rs.scenes(), chain()
    models, states, rws, forces, mus = [], [], [], [], []
    with _Oracles() as O:
        for k, mutant in jobs:
            for i, sc in enumerate(scs):
                models.append(rs.model(sc["model"])[0]); states.append(ch[i][k - 1]); forces.append(sc["unibody_force"])
                rws.append(rows(O.of(sc), sc, ch[i][k - 1], 1 if mutant == "start1" else 0))
                mus.append(None if mutant == "start1" else mutant)
    res = reset_ref.unibody_rounds(models, states, rws, forces, mus)
    for j, job in enumerate(jobs):
        _F64[job] = res[j * len(scs):(j + 1) * len(scs)]


def f64(k, mutant=None):
    prepare(() if mutant else (k,), (mutant,) if mutant else ())
    return _F64[(k, mutant)]


def distance(a, b):
    """{quantity: max |a - b|} of two states"""
    n = min(len(a), len(b))
    a, b = a[:n], b[:n]
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return {q: float(d[:, sl].max()) for q, sl in QUANTITIES}


def _family_max(per_scene, keep=None):
    scs = rs.scenes()
    out = {}
    for f in rs.FAMILIES:
        ds = [per_scene[i] for i, sc in enumerate(scs) if sc["family"] == f and (keep is None or i in keep)]
        out[f] = {q: max(d[q] for d in ds) for q, _ in QUANTITIES}
    return out


@functools.lru_cache(None)
def e_ref(k):
    """{family: {quantity: E_ref}} of round k"""
    ch, r64 = chain(), f64(k)
    return _family_max([distance(ch[i][k], r64[i]) for i in range(len(ch))])


@functools.lru_cache(None)
def sensitivity(k):
    """per scene {quantity: the largest movement of round k's result under the four nudges of size E_ref(k - 1)}"""
    scs, ch, e = rs.scenes(), chain(), e_ref(k - 1)
    out = []
    with _Oracles() as O:
        for i, sc in enumerate(scs):
            o = O.of(sc)
            worst = {q: 0.0 for q, _ in QUANTITIES}
            for d in range(DIRECTIONS):
                rng = np.random.default_rng(5000 + 16 * i + 4 * k + d)
                st = ch[i][k - 1][:o.nb].copy()
                for q, sl in QUANTITIES[:2]:      # the momenta of the model's bodies are zero throughout and stay so
                    st[:, sl] = (st[:, sl].astype(np.float64) + rng.choice([-1.0, 1.0], st[:, sl].shape) * e[sc["family"]][q]).astype(F)
                moved = distance(unibody_fit(o, sc, st), ch[i][k])
                worst = {q: max(worst[q], moved[q]) for q in worst}
            out.append(worst)
    return out


@functools.lru_cache(None)
def kept(k):
    """the scenes compared after round k >= 2: those no nudge before rounds 2 .. k flipped.  A family's yardstick is its median sensitivity, or the nudge itself where
    the median is smaller (a family of near-empty clouds, where a round moves nothing)"""
    if k < 2:
        return frozenset(range(len(rs.scenes())))
    scs, sens, e = rs.scenes(), sensitivity(k), e_ref(k - 1)
    keep = set(kept(k - 1))
    for f in rs.FAMILIES:
        idx = [i for i, sc in enumerate(scs) if sc["family"] == f]
        for q, _ in QUANTITIES[:2]:
            yard = max(float(np.median([sens[i][q] for i in idx])), e[f][q])
            keep -= {i for i in idx if sens[i][q] > FLIP * yard}
    return frozenset(keep)


@functools.lru_cache(None)
def s_ref(k):
    """{family: {quantity: S}} of round k over the scenes kept"""
    return _family_max(sensitivity(k), kept(k))


def bound(k):
    """{family: {quantity: what the product build may differ by after round k}}: 8 x E_ref(1) from the float64 round for k = 1, 8 x (E_ref(k) + S(k)) from the
    restatement's chain for k = 2, 3"""
    e = e_ref(k)
    if k == 1:
        return {f: {q: FACTOR * v for q, v in e[f].items()} for f in e}
    s = s_ref(k)
    return {f: {q: FACTOR * (e[f][q] + s[f][q]) for q in e[f]} for f in e}


def merge_report(family, section, values):
    """HT_RESET_FUZZ_REPORT=<file>: merge {family: {section: values}} into that JSON (profiles/reset_fuzz.json)"""
    import json
    import os
    path = os.environ.get("HT_RESET_FUZZ_REPORT")
    if not path:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {}
    if isinstance(values, dict):
        doc.setdefault(family, {}).setdefault(section, {}).update(values)
    else:
        doc.setdefault(family, {})[section] = values
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
