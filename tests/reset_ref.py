"""The full-reset branch (handtrack.h:451-506) in numpy float64: PoseFromScratch, and one round of UnibodyFit on rows handed to it.  The plain statement that the reset
fuzz (tests/test_reset_ref.py, tests/test_gpu_reset_fuzz.py) measures the fp32 restatement (oracle/ho_track.c: ho_pose_from_scratch, ho_unibody_fit) and k_reset against.
numpy and tests/solve_ref.py only; nothing of the oracle is imported.

    PoseFromScratch: palm ray = the normalised sum of the first three landmark rays; the cloud's centroid weighted by 1 / (1e-6 + |p x palmray|^2); every body back at its
    start pose, the model carried so that body 1 sits at (centroid, camera orientation x palmq); the four fingers curled by a/2, a, 1.25 a about x in their joint frames;
    FixPositions joint by joint; momenta zero.
    UnibodyFit, one round: rows [n,16] (CloudConstraint of every 4th point from the camera's position, limits -1 .. 1) -> each row's position1 re-expressed on the proxy body
    (a cube at body 1's position + the cube's com, body 1's orientation), limits x unibody_force -> PhysicsUpdate of that one body (solve_ref.physics_update) -> the model
    carried by (proxy after) x inverse(body 1 before).

mutant= (for this reference only): "no_com" the rows re-expressed about body 1's position without the proxy's com; "limits" force limits not scaled by unibody_force;
"drop_last" the last row dropped; "no_removebias" post sweeps without RemoveBias's min(ts, targetspeednobias).  ("start1", the stride-4 subsample starting at point 1,
is a mutant of the rows and so of the caller: tests/reset_oracle.py.)"""
import numpy as np

import htfx
import solve_ref

F64 = np.float64
W_EPS, SUM_EPS = float(np.float32(0.000001)), float(np.float32(0.00000000001))      # handtrack.h:486-487, as float literals
MUTANTS = ("no_com", "limits", "drop_last", "start1", "no_removebias")


class Model:
    """what the reset branch reads of a baked model file"""

    def __init__(self, path):
        m = htfx.load(path)
        self.path, self.nb, self.nj = path, int(m["nb"][0]), int(m["nj"][0])
        bf = m["body_f"].astype(F64).reshape(self.nb, 26)
        self.com, self.pos0, self.q0 = bf[:, 7:10], bf[:, 10:13], bf[:, 13:17]
        self.joint_i = m["joint_i"].reshape(self.nj, 2).astype(np.intp)
        jf = m["joint_f"].astype(F64).reshape(self.nj, 16)
        self.p0, self.p1, self.jframe = jf[:, 0:3], jf[:, 3:6], jf[:, 12:16]
        self.physics = m["physics"].astype(F64)
        u = m["unibody/f"].astype(F64)      # mass massinv radius damping friction gravscale com[3] tensorinv[9]
        self.ub_com = u[6:9]
        self.ub_body_f = np.zeros((1, 26), F64)
        self.ub_body_f[0, 1], self.ub_body_f[0, 4], self.ub_body_f[0, 5], self.ub_body_f[0, 17:26] = u[1], u[3], u[4], u[9:18]


def qrot(q, v):
    return np.einsum("...ij,...j->...i", solve_ref.qmat(np.asarray(q, F64)), np.asarray(v, F64))


def qconj(q):
    return np.asarray(q, F64) * np.array([-1.0, -1.0, -1.0, 1.0])


def pose_mul(a, b):
    return a[0] + qrot(a[1], b[0]), solve_ref.qmul(a[1], b[1])


def pose_inverse(a):
    return -qrot(qconj(a[1]), a[0]), qconj(a[1])


def palm_ray(an):
    cs = np.asarray(an[0:4], F64) + np.asarray(an[4:8], F64) + np.asarray(an[8:12], F64)
    return cs[:3] / np.sqrt((cs[:3] ** 2).sum())


def centroid(pts, an):
    pts = np.asarray(pts, F64).reshape(-1, 3)
    c = np.cross(pts, palm_ray(an))
    w = 1.0 / (W_EPS + (c * c).sum(-1))
    return (pts * w[:, None]).sum(0) / (SUM_EPS + w.sum())


def _carry(dp, pos, q):
    return dp[0] + qrot(dp[1], pos), solve_ref.qmul(np.broadcast_to(dp[1], q.shape), q)


def pose_from_scratch(model, pts, an, cam, pcom=None):
    """-> state [nb,13] float64.  an: the analysis [84] (rays 0:32, palmq 75:79, clench angles 79:84), cam [12] (pose 5:12).  pcom: stands in for the cloud's centroid"""
    an, cam = np.asarray(an, F64), np.asarray(cam, F64)
    pcom = centroid(pts, an) if pcom is None else np.asarray(pcom, F64)
    pos, q = model.pos0.copy(), model.q0.copy()
    dp = pose_mul((pcom, solve_ref.qmul(cam[8:12], an[75:79])), pose_inverse((pos[1], q[1])))
    pos, q = _carry(dp, pos, q)
    for finger in range(1, 5):
        a = an[79 + finger]
        for k, ang in enumerate((a / 2.0, a, a * 1.25)):
            b = 2 + k + finger * 3
            q[b] = solve_ref.qmul(model.jframe[1 + finger * 3], solve_ref.qmul(q[b], np.array([np.sin(ang / 2.0), 0.0, 0.0, np.cos(ang / 2.0)])))
    for j in range(model.nj):      # FixPositions (physmodel.h:404-408)
        r0, r1 = model.joint_i[j]
        u0 = pos[r0] + qrot(q[r0], -model.com[r0]); u1 = pos[r1] + qrot(q[r1], -model.com[r1])
        pos[r1] = pos[r1] + ((u0 + qrot(q[r0], model.p0[j])) - (u1 + qrot(q[r1], model.p1[j])))
    return np.concatenate([pos, q, np.zeros((model.nb, 6))], -1)


def proxy_rows(model, state, rows, unibody_force, mutant=None):
    """the rows of one frame as UnibodyFit hands them to PhysicsUpdate (handtrack.h:457-462) -> (proxy state [1,13], rows [n,16])"""
    state = np.asarray(state, F64)[:model.nb]
    pos, q = state[:, 0:3], state[:, 3:7]
    ubpos, ubq = pos[1] + model.ub_com, q[1]
    r = np.array(rows, F64).reshape(-1, 16)
    b = r[:, 1].astype(np.intp)
    world = pos[b] + qrot(q[b], r[:, 5:8])
    r[:, 5:8] = qrot(qconj(ubq), world - (pos[1] if mutant == "no_com" else ubpos))
    r[:, 1] = 0.0
    if mutant != "limits":
        r[:, 13:15] *= float(unibody_force)
    if mutant == "drop_last":
        r = r[:-1]
    if mutant == "no_removebias":
        r[:, 12] = np.inf
    return np.concatenate([ubpos, ubq, np.zeros(6)])[None], r


def unibody_rounds(models, states, rows, forces, mutants=None):
    """one round of UnibodyFit for every frame of a batch: models (a Model per frame, all with the same proxy cube but for its com), states: a list of [nb,13],
    rows: a list of [n_s,16], forces [S], mutants: one per frame or None -> a list of [nb + 1,13] float64: the model's bodies, and behind them the proxy body as its
    PhysicsUpdate left it (its momenta are where the post sweeps show: UnibodyFit drops them).  One batched PhysicsUpdate, whatever the frames' models."""
    S = len(states)
    mutants = mutants or [None] * S
    assert all(np.array_equal(m.ub_body_f, models[0].ub_body_f) and np.array_equal(m.physics, models[0].physics) for m in models)
    prox = [proxy_rows(m, s, r, f, mu) for m, s, r, f, mu in zip(models, states, rows, forces, mutants)]
    after = solve_ref.physics_update(np.stack([p[0] for p in prox]), [p[1] for p in prox], [np.zeros((0, 8))] * S, models[0].ub_body_f, models[0].physics)[0]
    out = []
    for s in range(S):
        st = np.asarray(states[s], F64)[:models[s].nb]
        pos, q = st[:, 0:3], st[:, 3:7]
        dp = pose_mul((after[s, 0, 0:3], after[s, 0, 3:7]), pose_inverse((pos[1], q[1])))
        new = st.copy()
        new[:, 0:3], new[:, 3:7] = _carry(dp, pos, q)
        out.append(np.concatenate([new, after[s]]))
    return out
