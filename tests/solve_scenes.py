"""Seeded scenes for the solver fuzz (tests/test_solve_ref.py, tests/test_gpu_solve_fuzz.py): caller-built rows for ht_physics_update, the general door into k_solve.

A scene is a dict: model ("hand17" / "hand26"), state [nb,13], lin [n,16], ang [n,8] (float32, the layouts of tests/solve_ref.py), collide (physics_use_collision),
and notes a test selects by: `switched` (an angular row RemoveBias switches on: targetspin -FLT_MAX with mintorque < 0) and `tail` (a two-body linear row).  FAMILIES[name](seed) -> list of scenes; scenes(name) caches the committed seed's.

Rows are kept well conditioned: unit normals and axes, lever arms <= 2 cm, rb0 != rb1, limits from {0, finite, +-FLT_MAX} (clamped, one-sided and free rows all occur),
target distances of millimetres.  Bodies carry more rows than they have degrees of freedom in most scenes, so the Gauss-Seidel result depends on the row order and on
every sweep: that is what lets tests/test_solve_ref.py tell a mutated reference from the true one."""
import functools
import os

import numpy as np

import htfx

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_PATH = {"hand17": os.path.join(HERE, "golden", "model_hand17.htfx"), "hand26": os.path.join(HERE, "golden", "model_hand26.htfx")}
FLT_MAX = np.float32(np.finfo(np.float32).max)
SEED = 20240607
COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)      # rows per body of the chains: the edges of the blocks of four and eight, and long chains
POINT_CAPACITY = 4096                                      # what a fresh context holds per frame (asserted by the GPU test before chains_long)
CONTACT_FRAMES = (3, 4, 6)                                 # golden8 frames whose start pose has contacts (17, 8, 15)
MAX_GROUPS = 32
MAX_RUNS = 128                                              # runs of consecutive angular rows on one body pair that a solve schedules
MAX_ANGULAR = 126                                           # angular rows a caller may hand to ht_physics_update / ht_fit_rows per frame


@functools.lru_cache(None)
def model(name):
    return htfx.load(MODEL_PATH[name])


@functools.lru_cache(None)
def _golden():
    return htfx.load(os.path.join(HERE, "golden", "golden8.htfx"))


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _state(rng, name, frame=None):
    """the rest state, or a golden start pose (hand17), with small momenta"""
    m = model(name); nb = len(m["nverts"])
    st = np.array(m["rest_state"], np.float32).reshape(nb, 13).copy()
    if frame is not None:
        st[:, :7] = _golden()["f%d/startpose" % frame]
    st[:, 7:10] = rng.normal(scale=2e-3, size=(nb, 3)); st[:, 10:13] = rng.normal(scale=2e-5, size=(nb, 3))
    return st


def _limits(rng, finite=(0.5, 5.0), free=0.4):
    """(lo, hi) with lo in {0, -finite, -FLT_MAX}, hi in {0, finite, FLT_MAX}, never both zero"""
    while True:
        lo = rng.choice(3, p=[0.2, 0.8 - free, free]); hi = rng.choice(3, p=[0.2, 0.8 - free, free])
        if lo or hi:
            f = lambda k: 0.0 if k == 0 else float(rng.uniform(*finite)) if k == 1 else float(FLT_MAX)
            return -f(lo), f(hi)


def lin_row(rng, rb0, rb1, lo=None, hi=None, normal=None, dist=None, fm=0, p0=None, p1=None):
    r = np.zeros(16, np.float32)
    r[0], r[1] = rb0, rb1
    r[2:5] = rng.uniform(-0.0115, 0.0115, 3) if p0 is None else p0      # |lever arm| <= 2 cm
    r[5:8] = rng.uniform(-0.0115, 0.0115, 3) if p1 is None else p1
    r[8:11] = _unit(rng) if normal is None else normal
    r[11] = rng.uniform(-2e-3, 2e-3) if dist is None else dist
    r[12] = 0.0 if rng.random() < 0.7 else -rng.uniform(0.0, 0.02)
    if lo is None:
        lo, hi = _limits(rng)
    r[13], r[14], r[15] = lo, hi, fm
    return r


def ang_row(rng, rb0, rb1, spin=None, lo=None, hi=None):
    r = np.zeros(8, np.float32)
    r[0], r[1] = rb0, rb1
    r[2:5] = _unit(rng)
    r[5] = rng.uniform(-0.5, 0.5) if spin is None else spin
    if lo is None:
        lo, hi = _limits(rng, finite=(0.02, 0.3))
    r[6], r[7] = lo, hi
    return r


def _rows(rows, width):
    return np.array(rows, np.float32).reshape(-1, width)


def _scene(name, st, lin=(), ang=(), **notes):
    lin, ang = _rows(list(lin), 16), _rows(list(ang), 8)
    sw = bool(np.any((ang[:, 5] == -FLT_MAX) & (ang[:, 6] < 0)))
    tail = tail_groups(lin)[1] > 0
    return dict(model=name, state=st, lin=lin, ang=ang, collide=False, switched=sw, tail=tail, **notes)


def tail_groups(lin):
    """How ht_physics_update's documentation splits a row list: (rows of the single-body prefix, groups of the tail).  The prefix is the leading rows that act on one body
    from the world, have no friction master and are not a master themselves; the tail goes in groups of up to three consecutive rows on one body pair, a master with its
    two friction rows being a group of its own."""
    n = len(lin); fm = [int(r[15]) for r in lin]
    p = 0
    while p < n and int(lin[p][0]) < 0 and fm[p] == 0 and not (p + 1 < n and fm[p + 1] != 0):
        p += 1
    groups, slot, pair, triple = 0, 3, None, False
    for i in range(p, n):
        pr = (int(lin[i][0]), int(lin[i][1]))
        if fm[i] != 0:
            slot += 1; triple = True
            continue
        master = i + 1 < n and fm[i + 1] != 0
        if slot > 2 or pr != pair or master or triple:
            groups += 1; slot = 0; pair = pr; triple = False
        slot += 1
    return p, groups


def angular_runs(ang):
    return sum(1 for i in range(len(ang)) if i == 0 or int(ang[i][0]) != int(ang[i - 1][0]) or int(ang[i][1]) != int(ang[i - 1][1]))


def swap_index(sc, lin=None):
    """a row i of [lin | ang] (lin: the linear rows as solved, the contact rows included) that shares a body with row i + 1 of the same kind, neither a friction row nor a
    master nor switched off (-1: none): the middle-most of those whose limits leave both rows room on either side, else the middle-most of all"""
    lin = sc["lin"] if lin is None else lin
    ang, found = sc["ang"], ([], [])
    for rows, base, lo in ((lin, 0, 13), (ang, len(lin), 6)):
        for i in range(len(rows) - 1):
            a, b = rows[i], rows[i + 1]
            if lo == 13 and (a[15] != 0 or b[15] != 0 or (i + 2 < len(rows) and rows[i + 2][15] != 0)):
                continue
            if lo == 6 and (a[5] == -FLT_MAX or b[5] == -FLT_MAX):
                continue
            if {int(a[0]), int(a[1])} & {int(b[0]), int(b[1])} - {-1}:
                found[0 if a[lo] < 0 < a[lo + 1] and b[lo] < 0 < b[lo + 1] else 1].append(base + i)
    best = found[0] or found[1]
    return best[len(best) // 2] if best else -1


# ------------------------------------------------------------------------------------------------- single-body chains
def _chain_rows(rng, counts):
    """counts[b] rows on body b from the world, the bodies interleaved at random (the kernel partitions them by body, keeping each body's order)"""
    owner = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(owner)
    return [lin_row(rng, -1, int(b)) for b in owner]


def _chains(name, seed, nscenes):
    rng = np.random.default_rng(seed); nb = len(model(name)["nverts"])
    out = []
    for k in range(nscenes):
        if k == 0:
            counts = np.zeros(nb, int); counts[nb - 2 if nb > 17 else 5] = 40      # every row on one body (hand26: a hosted body)
        elif k == 1:
            counts = np.ones(nb, int)                                            # one row on every body
        else:
            counts = rng.choice(COUNTS, nb)
            if nb > 17 and k % 2:
                counts[:16] = rng.choice((0, 1, 4), 16)                          # the hosted chains (bodies >= 16) longer than their hosts'
        out.append(_scene(name, _state(rng, name, None if name != "hand17" or k % 3 else k % 8), _chain_rows(rng, counts)))
    return out


def chains(seed=SEED):
    return _chains("hand17", seed, 40)


def chains26(seed=SEED):
    return _chains("hand26", seed + 1, 32)


def chains_long(seed=SEED, capacity=POINT_CAPACITY):
    """prefixes of capacity + 1 and capacity + 65 rows: the context grows its per-point arrays for them"""
    rng = np.random.default_rng(seed + 2)
    out = []
    for extra in (1, 65, 1, 65):
        n = capacity + extra
        owner = rng.integers(0, 17, n)
        rows = [lin_row(rng, -1, int(b), *((-f, f) if rng.random() < 0.8 else (None, None))) for b, f in zip(owner, rng.uniform(0.5, 3.0, n))]
        out.append(_scene("hand17", _state(rng, "hand17"), rows))
    return out


# ------------------------------------------------------------------------------------------------- two-body tails
def _triple(rng, a, b, pull=False):
    """a contact-style triple as ConstrainContacts builds it: the normal row (0..FLT_MAX), then the two friction rows (friction_master -1, -2) on the same anchors"""
    n = _unit(rng); t = np.cross(n, _unit(rng)); t /= np.linalg.norm(t); bn = np.cross(n, t)
    p0, p1 = rng.uniform(-0.0115, 0.0115, 3), rng.uniform(-0.0115, 0.0115, 3)
    d = rng.uniform(0.5e-3, 2e-3) * (1 if pull else -1)
    return [lin_row(rng, a, b, 0.0, float(FLT_MAX), n, d, 0, p0, p1), lin_row(rng, a, b, 0.0, 0.0, bn, 0.0, -1, p0, p1), lin_row(rng, a, b, 0.0, 0.0, t, 0.0, -2, p0, p1)]


def _pairs(rng, graph, n, nb=17):
    if graph == "star":
        c = int(rng.integers(0, nb)); others = [b for b in range(nb) if b != c]
        return [(c, others[k % len(others)]) if k % 2 else (others[k % len(others)], c) for k in range(n)]
    if graph == "chain":
        return [(k % (nb - 1), k % (nb - 1) + 1) for k in range(n)]
    if graph == "disjoint":
        return [(2 * (k % 8), 2 * (k % 8) + 1) for k in range(n)]
    if graph == "one":
        a, b = rng.choice(nb, 2, replace=False)
        return [(int(a), int(b))] * n
    out = []
    for _ in range(n):
        a, b = rng.choice(nb, 2, replace=False); out.append((int(a), int(b)))
    return out


def _tail(rng, graph, ngroups, triples=0.0, sizes=(1, 2, 3)):
    """a tail of exactly `ngroups` groups on the graph's pairs"""
    rows, prev, last = [], None, 0
    for pr in _pairs(rng, graph, ngroups):
        if rng.random() < triples:
            rows += _triple(rng, *pr, pull=rng.random() < 0.25); prev = None
            continue
        if pr == prev:      # rows on the pair of the group before them: that group is filled first, so that these open their own
            rows += [lin_row(rng, *pr) for _ in range(3 - last)]
        last = int(rng.choice(sizes))
        rows += [lin_row(rng, *pr) for _ in range(last)]; prev = pr
    assert tail_groups(_rows(rows, 16)) == (0, ngroups), (graph, ngroups, tail_groups(_rows(rows, 16)))
    return rows


def groups(seed=SEED):
    rng = np.random.default_rng(seed + 3)
    out = []
    plan = [("star", 1), ("star", 8), ("star", 9), ("star", 31), ("star", 32), ("chain", 8), ("chain", 9), ("chain", 31), ("chain", 32),
            ("disjoint", 8), ("disjoint", 9), ("disjoint", 16), ("disjoint", 31), ("disjoint", 32), ("one", 1), ("one", 8), ("one", 9), ("one", 32),
            ("random", 1), ("random", 8), ("random", 9), ("random", 31), ("random", 32)]
    for graph, n in plan:
        out.append(_scene("hand17", _state(rng, "hand17", int(rng.integers(0, 8)) if rng.random() < 0.5 else None), _tail(rng, graph, n)))
    for graph in ("star", "chain", "disjoint", "random"):      # with contact-style triples among the groups
        out.append(_scene("hand17", _state(rng, "hand17"), _tail(rng, graph, int(rng.choice((9, 20, 32))), triples=0.4)))
    for nrows in (4, 5, 4, 5):                                 # four or five consecutive rows on one pair: 3 + 1, 3 + 2
        a, b = (int(v) for v in rng.choice(17, 2, replace=False))
        rows = [lin_row(rng, a, b) for _ in range(nrows)] + _tail(rng, "random", 5)
        if (int(rows[nrows][0]), int(rows[nrows][1])) == (a, b):
            rows = rows[:nrows]
        assert tail_groups(_rows(rows[:nrows], 16)) == (0, 2)
        out.append(_scene("hand17", _state(rng, "hand17"), rows))
    for k in range(4):                                         # a free row directly before a friction triple on its pair
        a, b = (int(v) for v in rng.choice(17, 2, replace=False))
        rows = _tail(rng, "random", 3) if k % 2 else []
        rows += [lin_row(rng, a, b, -float(FLT_MAX), float(FLT_MAX))] + _triple(rng, a, b) + _tail(rng, "chain", 4)
        out.append(_scene("hand17", _state(rng, "hand17"), rows))
    for k in range(5):                                         # rows from the world (rb0 == NULL) in the tail, behind the first two-body row; a prefix in front on odd k
        rows = _chain_rows(rng, rng.choice((0, 1, 2, 5), 17)) if k % 2 else []
        rows += _tail(rng, "random", 2)
        for _ in range(int(rng.integers(1, 6))):
            b = int(rng.integers(0, 17))
            rows += [lin_row(rng, -1, b) for _ in range(int(rng.integers(1, 4)))] + _tail(rng, "random", 1)
        if k == 4:
            rows += _triple(rng, -1, 3)                        # a triple against the world: its master is no prefix row
        assert tail_groups(_rows(rows, 16))[1] <= MAX_GROUPS
        out.append(_scene("hand17", _state(rng, "hand17"), rows))
    assert 32 <= len(out) <= 64
    return out


def _drive(rng, bodies, per=2):
    """free single-body rows that push the bodies along: tangential speed for the friction rows to work against"""
    return [lin_row(rng, -1, int(b), -float(FLT_MAX), float(FLT_MAX), dist=float(rng.choice((-1, 1)) * rng.uniform(1e-3, 2e-3))) for b in bodies for _ in range(per)]


def friction(seed=SEED):
    rng = np.random.default_rng(seed + 4)
    out = []
    for k in range(1, 33):
        rows, used = [], set()
        pool = [int(v) for v in rng.choice(17, int(rng.integers(2, 9)), replace=False)]      # few bodies: triples share them
        for _ in range(k):
            a, b = (int(v) for v in rng.choice(pool, 2, replace=False)); used |= {a, b}
            rows += _triple(rng, a, b, pull=rng.random() < 0.25)
        out.append(_scene("hand17", _state(rng, "hand17", k % 8 if k % 2 else None), _drive(rng, sorted(used)) + rows))
    return out


# ------------------------------------------------------------------------------------------------- angular rows
def _angular_rows(rng, lengths, nb=17, off=0.0, one_body=0.15):
    """runs of the given lengths, consecutive runs on different body pairs; `off`: share of rows with targetspin -FLT_MAX, half of them with mintorque < 0"""
    rows, prev = [], None
    for n in lengths:
        while True:
            a, b = (int(v) for v in rng.choice(nb, 2, replace=False))
            if rng.random() < one_body:
                a = -1
            if (a, b) != prev:
                break
        prev = (a, b)
        for _ in range(n):
            if rng.random() < off:
                rows.append(ang_row(rng, a, b, -float(FLT_MAX), *((0.0, float(rng.uniform(0.02, 0.3))) if rng.random() < 0.5 else (-float(rng.uniform(0.02, 0.3)), float(rng.uniform(0.02, 0.3))))))
            else:
                rows.append(ang_row(rng, a, b))
    return rows


def _lengths(rng, runs=None, rows=None):
    """run lengths 1..6 with the given number of runs and / or rows"""
    if runs is None:
        out = []
        while sum(out) < rows:
            out.append(min(int(rng.integers(1, 7)), rows - sum(out)))
        return out
    out = [1] * runs
    while rows is not None and sum(out) < rows:
        k = int(rng.integers(0, runs))
        if out[k] < 6:
            out[k] += 1
    if rows is None:
        out = [int(rng.integers(1, 7)) if runs <= 40 else int(rng.choice((1, 1, 2))) for _ in range(runs)]
    return out


def angular(seed=SEED):
    rng = np.random.default_rng(seed + 5)
    plan = [dict(runs=1, rows=1), dict(runs=1, rows=6), dict(runs=8), dict(runs=9), dict(runs=63), dict(runs=64), dict(runs=65), dict(runs=126, rows=126),
            dict(runs=63, rows=125), dict(runs=64, rows=126), dict(runs=65, rows=125), dict(runs=100, rows=126), dict(rows=124), dict(rows=125), dict(rows=126),
            dict(runs=125, rows=125)]
    out = []
    for k, p in enumerate(plan + plan):
        off = 0.0 if k < len(plan) else 0.15      # the second half with rows that are off, some of which RemoveBias switches on
        ln = _lengths(rng, p.get("runs"), p.get("rows"))
        sc = _scene("hand17", _state(rng, "hand17", k % 8 if k % 2 else None), (), _angular_rows(rng, ln, off=off))
        assert angular_runs(sc["ang"]) == len(ln) and len(sc["ang"]) <= MAX_ANGULAR
        out.append(sc)
    for k in range(4):      # rows that are off with mintorque == 0 only: RemoveBias leaves them off, the blocked form holds the frame
        rows = _angular_rows(rng, _lengths(rng, rows=40 + 20 * k))
        for r in rows[::3]:
            r[5] = -FLT_MAX; r[6] = 0.0
        out.append(_scene("hand17", _state(rng, "hand17"), (), rows))
        assert not out[-1]["switched"]
    return out


def mixed(seed=SEED):
    rng = np.random.default_rng(seed + 6)
    out = []
    for k in range(32):
        pre = _chain_rows(rng, rng.choice((0, 1, 3, 4, 5, 8, 9), 17))
        tail = _tail(rng, str(rng.choice(("star", "chain", "disjoint", "random"))), int(rng.integers(4, 31)), triples=0.3) if k % 4 else []
        ang = _angular_rows(rng, _lengths(rng, rows=int(rng.integers(10, 61))), off=0.1 if k % 2 else 0.0)
        out.append(_scene("hand17", _state(rng, "hand17", k % 8 if k % 3 == 0 else None), pre + tail, ang))
    return out


def with_contacts(seed=SEED):
    """golden fist start poses with physics_use_collision = 1: the contact triples follow the caller's rows.  Even scenes have no two-body caller row and no switched-on
    angular row (the blocked form holds them), odd scenes have one two-body group."""
    rng = np.random.default_rng(seed + 7)
    out = []
    for k in range(32):
        frame = CONTACT_FRAMES[k % 3]
        pre = _chain_rows(rng, rng.choice((0, 1, 2, 4, 5), 17))
        tail = _tail(rng, "random", 1) if k % 2 else []
        ang = _angular_rows(rng, _lengths(rng, rows=int(rng.integers(4, 30))))
        sc = _scene("hand17", _state(rng, "hand17", frame), pre + tail, ang, frame=frame)
        sc["collide"] = True
        out.append(sc)
    return out


def too_many_angular(seed=SEED):
    """angular row lists beyond the 126 rows a caller may hand over (127, 253, 300 rows, 129 and 200 runs of one row): ht_physics_update refuses them"""
    rng = np.random.default_rng(seed + 8)
    return [_scene("hand17", _state(rng, "hand17"), (), _angular_rows(rng, ln)) for ln in ([1] * 127, [2] * 126 + [1], [3] * 100, [1] * 129, [1] * 200)]


def crowded(seed=SEED):
    """bodies drawn about one point (tests/contact_scenes.py: d17 with 31 to 91 contacts, e17 with 45 to 69) with physics_use_collision = 1: more contact triples than a
    tracked hand has, so that with the caller's groups a frame has more than 64 groups (the level schedule then works two groups per lane).  Scenes 0, 3, 6, ... have no
    caller's two-body row (up to 40 contacts the blocked form holds them), the others a tail of 8 or 32 groups."""
    import contact_scenes
    rng = np.random.default_rng(seed + 10)
    poses = [st for st in contact_scenes.states("d17")[5:]] + [st for st in contact_scenes.states("e17")[:16]]
    out = []
    for k in range(32):
        st = np.array(poses[k % len(poses)], np.float32).copy()
        st[:, 7:10] = rng.normal(scale=2e-3, size=(17, 3)); st[:, 10:13] = rng.normal(scale=2e-5, size=(17, 3))
        pre = _chain_rows(rng, rng.choice((0, 1, 2, 4), 17))
        tail = _tail(rng, "random", 32 if k % 3 == 1 else 8) if k % 3 else []
        sc = _scene("hand17", st, pre + tail, _angular_rows(rng, _lengths(rng, rows=int(rng.integers(4, 30)))))
        sc["collide"] = True
        out.append(sc)
    return out


def many_runs(seed=SEED):
    """For ht_fit_rows, not ht_physics_update: caller's angular rows in runs of one row on changing body pairs, ahead of the model's own joint rows (16 runs).  112 rows make
    the 128 runs the level schedule holds; 113, 120 and 126 make more, and the rows from run 128 on are dropped and counted (csrc/ht_solve_shared.hpp: MAXA_RUNS).  One row
    in three is off and switched on by RemoveBias, so that no frame is one the blocked form holds."""
    rng = np.random.default_rng(seed + 11)
    out = []
    for k, n in enumerate((112, 113, 120, 126)):
        rows = _angular_rows(rng, [1] * n, one_body=0.0)
        for r in rows[::3]:
            r[5] = -FLT_MAX; r[6] = -float(rng.uniform(0.02, 0.3))
        out.append(_scene("hand17", _state(rng, "hand17", 2 * k), (), rows))
    return out


FAMILIES = dict(chains=chains, chains26=chains26, chains_long=chains_long, groups=groups, friction=friction, angular=angular, mixed=mixed,
                with_contacts=with_contacts, crowded=crowded)


@functools.lru_cache(None)
def scenes(family):
    return FAMILIES[family]()
