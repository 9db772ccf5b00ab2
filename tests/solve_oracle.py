"""The solver fuzz's two references side by side: the fp32 restatement (ho_physics_update, oracle/ho_physics.c) and the float64 statement (tests/solve_ref.py) on the
scenes of tests/solve_scenes.py, and E_ref = max |oracle32 - f64| per family and quantity: the reference's own rounding distance, the yardstick of every bound of
tests/test_solve_ref.py and tests/test_gpu_solve_fuzz.py.  Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as ol
import solve_ref
import solve_scenes as ss

QUANTITIES = (("position", slice(0, 3)), ("quaternion", slice(3, 7)), ("linear_momentum", slice(7, 10)), ("angular_momentum", slice(10, 13)))
FACTOR = 8.0      # BOUND = FACTOR x E_ref: the product applies the same rows in the same order with the same clamps and differs in association only


def _fill_linear(L, rows):
    for i, r in enumerate(rows):
        L[i].rb0 = int(r[0]); L[i].rb1 = int(r[1]); L[i].position0 = ol.v3(r[2:5]); L[i].position1 = ol.v3(r[5:8]); L[i].normal = ol.v3(r[8:11])
        L[i].targetdist = float(r[11]); L[i].targetspeednobias = float(r[12]); L[i].forcelimit = ol.F2(float(r[13]), float(r[14])); L[i].friction_master = int(r[15])
        L[i].targetspeed = 0.0; L[i].impulsesum = 0.0


def _fill_angular(A, rows):
    for i, r in enumerate(rows):
        A[i].rb0 = int(r[0]); A[i].rb1 = int(r[1]); A[i].axis = ol.v3(r[2:5]); A[i].torque = 0.0; A[i].targetspin = float(r[5]); A[i].mintorque = float(r[6]); A[i].maxtorque = float(r[7])


def oracle32(scenes):
    """every scene through ho_physics_update -> (states float32 [S,nb,13], the linear rows each scene was solved with: the caller's, then the contact rows ConstrainContacts
    built when the scene collides)"""
    name = scenes[0]["model"]
    o = ol.Oracle(model=ss.MODEL_PATH[name])
    L = o.L
    m = o.model(0)
    bodies = (C.c_void_p * o.nb)(*[L.ho_body_ptr(m, b) for b in range(o.nb)])
    states, lins = [], []
    try:
        for sc in scenes:
            nl, na = len(sc["lin"]), len(sc["ang"])
            cap = nl + 3 * 256
            rows = (ol.Linear * cap)(); ang = (ol.Angular * max(1, na))()
            _fill_linear(rows, sc["lin"]); _fill_angular(ang, sc["ang"])
            o.set_state(0, sc["state"])
            o.head.phys.use_collision = 1 if sc["collide"] else 0
            nc = 0
            if sc["collide"]:
                cs = (ol.Contact * 256)()
                nc = L.ho_find_contacts(o.h, m, cs, 256)
            L.ho_physics_update(o.h, bodies, o.nb, m if sc["collide"] else None, rows, nl, cap, ang, na)
            states.append(o.get_state(0))
            lins.append(np.concatenate([sc["lin"], ol.linears_to_array(rows, nl + 3 * nc)[nl:]]) if nc else sc["lin"])
    finally:
        o.close()
    return np.stack(states), lins


@functools.lru_cache(None)
def scenes(family):
    """the family's scenes as PhysicsUpdate sees them.  many_runs goes through PhysModel::FitPointCloud (ht_fit_rows) without a cloud: the model's nailed joint rows and,
    behind the caller's angular rows, its joint-range rows join, as the restatement builds them for the scene's pose; of the angular rows those of the first 128 runs are
    kept, which is what k_solve documents (`dropped`: whether that left rows out)"""
    if family != "many_runs":
        return ss.scenes(family)
    o = ol.Oracle(model=ss.MODEL_PATH["hand17"]); m = o.model(0)
    out = []
    try:
        for sc in ss.many_runs():
            o.set_state(0, sc["state"])
            L, A, n, z = (ol.Linear * 96)(), (ol.Angular * 128)(), C.c_int(0), ol.F3(0, 0, 0)
            o.L.ho_enhancements(o.h, m, A, C.byref(n), 0, z, z, 0)      # brings the joint ranges up to date; no rows of its own in this mode
            assert n.value == 0
            nl = o.L.ho_joint_linears(m, L); na = o.L.ho_joint_angulars(o.h, m, A)
            ang = np.concatenate([sc["ang"], ol.angulars_to_array(A, na)])
            heads = solve_ref.angular_runs(ang)
            keep = heads[ss.MAX_RUNS] if len(heads) - 1 > ss.MAX_RUNS else len(ang)
            out.append(dict(sc, lin=ol.linears_to_array(L, nl), ang=ang[:keep], dropped=keep < len(ang), runs=len(heads) - 1))
    finally:
        o.close()
    return out


@functools.lru_cache(None)
def restated(family):
    """(oracle32 states, float64 states, linear rows as solved) of the family's scenes"""
    s32, lins = oracle32(scenes(family))
    return s32, f64(family, None, lins), lins


def f64(family, mutant, lins=None):
    scs = scenes(family)
    if lins is None:
        lins = restated(family)[2] if scs[0]["collide"] else [sc["lin"] for sc in scs]
    m = ss.model(scs[0]["model"])
    return solve_ref.physics_update(np.stack([sc["state"] for sc in scs]), lins, [sc["ang"] for sc in scs], m["body_f"], m["physics"], mutant=mutant)[0]


def distance(a, b):
    """max |a - b| per scene and quantity: {quantity: [S]}"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return {q: d[:, :, sl].reshape(len(d), -1).max(1) for q, sl in QUANTITIES}


@functools.lru_cache(None)
def e_ref(family):
    s32, s64, _ = restated(family)
    return {q: float(v.max()) for q, v in distance(s32, s64).items()}


def bound(family):
    return {q: FACTOR * v for q, v in e_ref(family).items()}
