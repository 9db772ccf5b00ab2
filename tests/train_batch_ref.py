"""References for the mini-batch training step (csrc/ht_train_batch.hip), built from tests/train_ref.py.  A helper, not a test.

One step on samples s_0..s_{n-1} from weights w:   w' = w - alpha * sum_b g_b(w).
    float64   w64' = w + sum_b (train_ref.train_step(w, x_b, t_b, alpha)["w"] - w)
    float32   w32' = w + sum_b (train_ref.oracle_step(w, x_b, t_b, alpha)["w"] - w)      (the differences and the sum taken in float64)
A later step of the same call starts from w64' (float64) and from w32' rounded to float32 (the oracle).

The rule is DESIGN.md section 18.1's, per weight tensor T of W1 B1 W2 B2 W3 B3 W4 B4:
    max|T_dev' - T_64'| <= 4 d_orc(T) + 4 * 2^-24 max|T_64'|,   d_orc(T) = max|T_32' - T_64'|
and per sample, for a3 a6 a8 e9 e7 e6 e3 and the loss, train_ref's expression on that sample's own float64 / oracle step at the step's weights (for a
case of train_ref.CASES on the seeded weights that is train_ref.bound(case, T, weights): the per-sample tensors do not depend on alpha).

Samples: the cases of train_ref ("a" "b0" "b1" "c" "e"; "d" is "c" on the weights scaled by SAT_SCALE), "f1" (the middle frame of train3.htfx) and the
seeded extras "x<i>": dense default_rng(100 + i) inputs and targets.
Batches (name -> weights, pool, order, samples per step, alpha):
    S1    [c]                                   one sample
    S5    [a, b0, b1, c, e]                     no multiple of 4 (a padded k-group), an all-0 and an all-1 tile;  S5hi: the same at alpha 0.25
    S5r   S5 with order [0, 3, 3, 1, 4]         a sample twice
    S33   S5 + f1 + x0..x26                     one row past a 32-row tile
    Sd    [d, x0] on the scaled weights         tanh at exactly +-1.0f
    S5x2  S5 + [f1, x0, x1, x2, x3], 5 a step   the second step starts from the first's weights
    S3 [a, c, b1], S3hi [a, c, e] at 0.25 and S5x2stale (the second step's samples at the seeded weights) serve tests/test_train_batch_ref.py only.
All steps that share weights and alpha are computed in one pass over their samples, each sample's step once; results are cached and not to be modified."""
import numpy as np

import train_ref as tr

PER_SAMPLE = ("a3", "a6", "a8", "e9", "e7", "e6", "e3", "mse")
TENSORS = tuple(tr.OFF)
S5 = ["a", "b0", "b1", "c", "e"]
STEP2 = ["f1", "x0", "x1", "x2", "x3"]
BATCHES = {
    "S1": dict(w="seed", pool=["c"], order=None, batch=1, alpha=0.001),
    "S5": dict(w="seed", pool=S5, order=None, batch=5, alpha=0.001),
    "S5hi": dict(w="seed", pool=S5, order=None, batch=5, alpha=0.25),
    "S5r": dict(w="seed", pool=S5, order=[0, 3, 3, 1, 4], batch=5, alpha=0.001),
    "S33": dict(w="seed", pool=S5 + ["f1"] + ["x%d" % i for i in range(27)], order=None, batch=33, alpha=0.001),
    "Sd": dict(w="sat", pool=["d", "x0"], order=None, batch=2, alpha=0.001),
    "S5x2": dict(w="seed", pool=S5 + STEP2, order=None, batch=5, alpha=0.001),
    "S3": dict(w="seed", pool=["a", "c", "b1"], order=None, batch=3, alpha=0.001),
    "S3hi": dict(w="seed", pool=["a", "c", "e"], order=None, batch=3, alpha=0.25),
    "S5x2stale": dict(w="seed", pool=STEP2, order=None, batch=5, alpha=0.001),
}
GPU_BATCHES = ("S1", "S5", "S5hi", "S5r", "S33", "Sd", "S5x2")
_cache = {}


def sample(name, weights):
    """(input [4096], target [2304]) float32"""
    if name in tr.CASES:
        _, x, t, _ = tr.case(name, weights)
        return x, t
    if name == "f1":
        xs, ts = tr._fixture()
        return xs[1], ts[1]
    rng = np.random.default_rng(100 + int(name[1:]))
    return rng.random(4096).astype(np.float32), rng.random(2304).astype(np.float32)


def start_weights(key, weights):
    return np.array(weights, np.float32, copy=True) if key == "seed" else tr.case("d", weights)[0]


def sequence(name):
    """the samples of a batch in the order they are trained on, and its steps as (first, last) positions of that sequence"""
    B = BATCHES[name]
    seq = [B["pool"][i] for i in B["order"]] if B["order"] is not None else list(B["pool"])
    return seq, [(k, min(k + B["batch"], len(seq))) for k in range(0, len(seq), B["batch"])]


def pool_arrays(name, weights):
    """(inputs [n, 4096], targets [n, 2304]) of a batch's pool"""
    xt = [sample(s, weights) for s in BATCHES[name]["pool"]]
    return np.stack([x for x, _ in xt]), np.stack([t for _, t in xt])


def _one(w64, w32, x, t, alpha):
    """a sample's float64 and oracle steps: its tensors, their bounds, both weight differences (float64) and how far it moves each weight tensor"""
    f = tr.train_step(w64, x, t, alpha)
    o = tr.oracle_step(w32, x, t, alpha)
    small = {T: np.array(f[T]) for T in PER_SAMPLE}
    bnd = {T: 4.0 * tr.dist(o[T], f[T]) + 4.0 * 2.0 ** -24 * float(np.abs(f[T]).max()) for T in PER_SAMPLE}
    d64 = f["w"] - w64
    d32 = np.float64(o["w"]) - np.float64(w32)
    eff = {T: float(np.abs(v).max()) for T, v in tr.split(d64).items()}
    return dict(tensors=small, bound=bnd, effect=eff), d64, d32


def _steps(jobs, weights):
    """jobs: (key, w64, w32, [sample names], alpha) that share w64 / w32 / alpha -> {key: step record}; every distinct sample is stepped once"""
    w64, w32, alpha = jobs[0][1], jobs[0][2], jobs[0][4]
    acc = {j[0]: [np.zeros(tr.COUNT), np.zeros(tr.COUNT)] for j in jobs}
    per = {}
    for s in sorted({s for j in jobs for s in j[3]}):
        x, t = sample(s, weights)
        per[s], d64, d32 = _one(w64, w32, x, t, alpha)
        for j in jobs:
            for _ in range(j[3].count(s)):
                acc[j[0]][0] += d64; acc[j[0]][1] += d32
    out = {}
    for j in jobs:
        e64, e32 = w64 + acc[j[0]][0], np.float64(w32) + acc[j[0]][1]
        P, Q = tr.split(e64), tr.split(e32)
        d_orc = {T: tr.dist(Q[T], P[T]) for T in TENSORS}
        out[j[0]] = dict(w64=e64, w32=e32.astype(np.float32), d_orc=d_orc, bound={T: 4.0 * d_orc[T] + 4.0 * 2.0 ** -24 * float(np.abs(P[T]).max()) for T in TENSORS},
                         samples=[per[s] for s in j[3]], names=list(j[3]))
    return out


def references(names, weights):
    """{batch: [step record, ...]} for the batches asked for.  A step record: w64 (float64 weights after the step), d_orc and bound per weight
    tensor, samples = per position of the step a dict(tensors, bound, effect) and names."""
    todo = [n for n in names if n not in _cache]
    groups = {}
    for n in todo:
        B = BATCHES[n]
        seq, steps = sequence(n)
        groups.setdefault((B["w"], B["alpha"]), []).append((n, seq[steps[0][0]:steps[0][1]]))
    for (wk, alpha), members in groups.items():
        w = start_weights(wk, weights)
        got = _steps([(n, np.float64(w), w, seq, alpha) for n, seq in members], weights)
        for n, _ in members:
            _cache[n] = [got[n]]
    for n in todo:      # later steps of a call, each from the step before it
        seq, steps = sequence(n)
        for a, b in steps[1:]:
            prev = _cache[n][-1]
            _cache[n].append(_steps([(n, prev["w64"], prev["w32"], seq[a:b], BATCHES[n]["alpha"])], weights)[n])
    return {n: _cache[n] for n in names}
