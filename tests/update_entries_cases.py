"""The update entry points of the C ABI as a table: every entry, each of its frame kinds, and the faults each refuses.

Shared by tests/test_gpu_update_entries.py (which compares) and tests/golden/make_update_entries.py (which records, once, from the commit before the entry points
were rewritten).  Everything goes through native.Context and the library it loaded; nothing here knows how the entry points are built.

Frames, all B = 3 (two hands: 2 frames = 4 slots): "tile" the first 64x64 tiles of golden8.htfx, "qvga" the two 320x240 frames of fullframe320close.htfx (as 0, 1, 0),
"c128" their central 128x128 pixels (the camera's principal point moved with the window).
"""
import ctypes as C
import os

import numpy as np
import torch

import htfx
import oracle_lib as ol
from hand_tracking_samples_amd import native, weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDING = os.path.join(HERE, "golden", "update_entries.json")
DEV = "cuda:0"
B, CAP = 3, 4
SPLIT = dict(lo=0, hi=650, step=65535, minpx=50, far=3999)      # tests/split_ref.py: SCENE_HI, SCENE_MIN_PIXELS, SCENE_FAR
MERGED, ALWAYS = native.SPLIT_MODEL_MERGED, native.SPLIT_MODEL_ALWAYS

# parameter lists as include/ht_mi355x.h declares them
SIG = {
    ("update", "sync"): "ctx depth cams B poses cnn",
    ("update", "dev"): "ctx depth cams start B poses stream",
    ("frames", "sync"): "ctx depth cams w h scale B poses cnn",
    ("frames", "dev"): "ctx depth cams w h scale start B poses stream",
    ("frames_sized", "sync"): "ctx side depth cams w h scale B poses cnn",
    ("frames_sized", "dev"): "ctx side depth cams w h scale start B poses stream",
    ("direct", "sync"): "ctx depth cams side B poses cnn",
    ("direct", "dev"): "ctx depth cams side start B poses stream",
    ("hands", "sync"): "ctx side depth cams w h scale hands B poses cnn",
    ("hands", "dev"): "ctx side depth cams w h scale hands start B poses stream",
    ("two_hands", "sync"): "ctx side depth cams w h scale lo hi step minpx far flags B poses info cnn",
    ("two_hands", "dev"): "ctx side depth cams w h scale lo hi step minpx far flags start B poses info stream",
    ("two_hands_model", "sync"): "ctx side depth cams w h scale lo hi step minpx far maxdist mode flags B poses info source cnn",
    ("two_hands_model", "dev"): "ctx side depth cams w h scale lo hi step minpx far maxdist mode flags start B poses info source stream",
    ("cnn_model", "sync"): "ctx depth cams w h scale B apply poses acc cnn",
    ("passes", "sync"): "ctx depth cams w h B poses",
    ("job_start", "sync"): "ctx main depth cams w h scale B",
}
ENTRIES = sorted({e for e, _ in SIG})
TWO = ("two_hands", "two_hands_model")
SIDED = ("frames_sized", "direct", "hands") + TWO


def _symbol(entry, form):
    return "ht_job_start" if entry == "job_start" else "ht_update_%s" % form if entry == "update" else "ht_update_%s_%s" % (entry, form)


def _frames(name):
    G = htfx.load(os.path.join(HERE, "golden", name))
    n = len(G["rows"])
    return (np.ascontiguousarray(np.stack([G["f%d/depth" % f] for f in range(n)])), np.stack([G["f%d/cam" % f] for f in range(n)]).astype(np.float32),
            np.stack([G["f%d/startpose" % f] for f in range(n)]).astype(np.float32))


def _sets():
    td, tc, ts = _frames("golden8.htfx")
    qd, qc, qs = _frames("fullframe320close.htfx")
    idx = [0, 1, 0]
    qd, qc, qs = qd[idx], qc[idx], qs[idx]
    cd = np.ascontiguousarray(qd[:, 56:184, 96:224]); cc = qc.copy(); cc[:, 2] -= 96.0; cc[:, 3] -= 56.0
    return {"tile": (np.ascontiguousarray(td[:B]), tc[:B], ts[:B]), "qvga": (np.ascontiguousarray(qd), qc, qs), "c128": (cd, cc, qs)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


class Env:
    """ctx: both nets' weights; ctx64: the 64x64 net's alone (the `second context` of the fault table); job: the overlapped update's second context"""

    def __init__(self):
        self.sets = _sets()
        w64, w128 = W.make_cnnb(), W.make_cnnb128()
        self.ctx, self.ctx64, self.job = (native.Context(ol.MODEL, CAP) for _ in range(3))
        for c in (self.ctx, self.ctx64, self.job):
            c.load_weights(w64); c.set_params(microforce=3.0, mainthreadpasses=3)
        self.ctx.load_weights128(w128)
        self.L = L = self.ctx.L
        u16, fp = C.POINTER(C.c_uint16), C.POINTER(C.c_float)
        L.ht_job_start.argtypes = [C.c_void_p, C.c_void_p, u16, fp, C.c_int, C.c_int, C.c_float, C.c_int]
        L.ht_job_wait.argtypes = [C.c_void_p]
        L.ht_job_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.ht_update_passes_sync.argtypes = [C.c_void_p, u16, fp, C.c_int, C.c_int, C.c_int, fp]
        self.nb = self.ctx.nb
        self.big = np.zeros((B, 480, 640), np.uint16)      # what the refused 640x480 calls point at: never read
        self.keep = []      # device tensors of the calls in flight

    def close(self):
        for c in (self.ctx, self.ctx64, self.job):
            c.close()

    def args(self, entry, form, frames="tile", side=64, hands=None, n=None, start=True, mode=MERGED, flags=0, ctx=None):
        """the named arguments of one good call; `n` frames (default: 3, two hands 2)"""
        depth, cams, st = self.sets[frames] if isinstance(frames, str) else frames
        two = entry in TWO
        n = (2 if two else B) if n is None else n
        slots = 2 * n if two else n
        h, w = depth.shape[1:]
        depth, cams, st = depth[:n], cams[:n], st[:n]
        if two:
            st = np.repeat(st, 2, axis=0)
        a = dict(ctx=(ctx or self.ctx).h, B=n, w=w, h=h, side=side, scale=0.17, apply=0, maxdist=float("inf"), mode=mode, flags=flags, main=self.ctx.h, stream=None, **SPLIT)
        if entry == "job_start":
            a["ctx"] = self.job.h
        if form == "sync":
            a.update(depth=np.ascontiguousarray(depth), cams=np.ascontiguousarray(cams), poses=np.zeros((slots, self.nb, 7), np.float32), cnn=np.zeros((slots, 2304), np.float32),
                     hands=None if hands is None else np.ascontiguousarray(hands[:n], np.uint8), info=np.zeros((n, 2, 8), np.int32), source=np.zeros(n, np.int32), acc=np.zeros(n, np.int32))
        else:
            a.update(depth=_dev(depth), cams=_dev(cams), start=_dev(st) if start else None, poses=torch.zeros(slots * self.nb * 7, dtype=torch.float32, device=DEV),
                     hands=None if hands is None else _dev(np.ascontiguousarray(hands[:n], np.uint8)), info=torch.zeros(n * 16, dtype=torch.int32, device=DEV),
                     source=torch.zeros(n, dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()      # the contexts run on streams of their own
        return a

    def call(self, entry, form, a):
        """-> the return code; the arguments by name, a numpy array or a tensor as its address"""
        fn = getattr(self.L, _symbol(entry, form))
        vals = []
        for name, t in zip(SIG[(entry, form)].split(), fn.argtypes):
            v = a[name]
            if isinstance(v, np.ndarray):
                v = C.cast(v.ctypes.data, t) if t is not C.c_void_p else v.ctypes.data
            elif isinstance(v, torch.Tensor):
                v = v.data_ptr()
            vals.append(v)
        self.keep = [a]
        return fn(*vals)

    def outputs(self, entry, form, a, ctx=None):
        """poses and cnn_out of a finished good call, as numpy arrays"""
        ctx = ctx or self.ctx
        slots = a["B"] * (2 if entry in TWO else 1)
        if entry == "job_start":
            assert self.L.ht_job_wait(self.job.h) == 0 and self.L.ht_job_collect(self.job.h, self.ctx.h, a["B"], None) == 0
            return self.job.get_state(1, slots), self.job.cnn_results(slots)[1]
        if form == "dev":
            ctx.tracker_flags(1)      # waits for the context's stream
            return a["poses"].cpu().numpy().reshape(slots, self.nb, 7), ctx.cnn_results(slots)[1]
        return a["poses"], (np.zeros(1, np.float32) if entry == "passes" else a["cnn"])      # (the caller's part of the overlapped update runs no net)

    def start(self, entry, a, frames, hands=None):
        """every good call runs from the same carried state: the frames' start poses in the slots, as a *_dev call seeds them from its d_start_poses (a left hand's
        mirrored: the slots' state is canonical; two hands: each frame's pose in both of its slots)"""
        st = (self.sets[frames] if isinstance(frames, str) else frames)[2][:a["B"]]
        if entry in TWO:
            st = np.repeat(st, 2, axis=0); hands = np.arange(len(st)) % 2
        if hands is not None:
            st = self.ctx.mirror_poses(st, np.ascontiguousarray(hands[:len(st)], np.uint8))
        self.ctx.tracker_reset(st)
        if entry == "job_start":
            self.job.tracker_reset(st)


# ---- the good calls: entry -> [(label, form, keyword arguments of Env.args)] ---------------------------------------------------------------------------------------
MIXED = np.array([0, 7, 255], np.uint8)      # any nonzero flag is a left hand


def good_calls(entry):
    both = ("sync", "dev")
    if entry == "update":
        return [("tile/" + f, f, dict(frames="tile")) for f in both]
    if entry == "frames":
        return [("%s/%s" % (k, f), f, dict(frames=k)) for k in ("tile", "qvga") for f in both]
    if entry == "frames_sized":
        return [("%d/%s/%s" % (s, k, f), f, dict(frames=k, side=s)) for s, k in ((64, "tile"), (64, "qvga"), (128, "c128"), (128, "qvga"), (128, "tile")) for f in both]
    if entry == "direct":
        return [("%d/%s" % (s, f), f, dict(frames=k, side=s)) for s, k in ((64, "tile"), (128, "c128")) for f in both]
    if entry == "hands":
        return [("%d/%s/%s/%s" % (s, k, "flags" if fl is not None else "null", f), f, dict(frames=k, side=s, hands=fl))
                for s, k in ((64, "tile"), (64, "qvga"), (128, "c128"), (128, "qvga")) for fl in (None, MIXED) for f in both]
    if entry == "two_hands":
        return [("%d/%s/%s" % (s, k, f), f, dict(frames=k, side=s)) for s, k in ((64, "qvga"), (64, "tile"), (128, "c128"), (128, "qvga")) for f in both]
    if entry == "two_hands_model":
        return [("%d/%s/%s/%s" % (s, k, "merged" if m == MERGED else "always", f), f, dict(frames=k, side=s, mode=m)) for s, k in ((64, "qvga"), (128, "c128")) for m in (MERGED, ALWAYS) for f in both]
    if entry == "cnn_model":
        return [("%s/%s" % (k, "kickstart" if ap else "model"), "sync", dict(frames=k, apply=ap)) for k in ("tile", "qvga") for ap in (0, 1)]
    return [(k, "sync", dict(frames=k)) for k in ("tile", "qvga")]      # passes, job_start


def run_good(env, entry, label, form, kw, level=0):
    """one good call from the start poses -> (poses, cnn_out, {scope name: launches} at profile level `level`)"""
    kw = dict(kw); apply = kw.pop("apply", 0)
    a = env.args(entry, form, **kw); a["apply"] = apply
    env.start(entry, a, kw["frames"], kw.get("hands"))
    prof = env.job if entry == "job_start" else env.ctx
    prof.profile_enable(level); prof.profile_read(True)
    try:
        rc = env.call(entry, form, a)
        assert rc == 0, (entry, label, rc, env.L.ht_last_error(a["ctx"]).decode())
        poses, cnn = env.outputs(entry, form, a)
        counts = {k: v[1] for k, v in prof.profile_read(True).items() if v[1]} if level else {}      # (a scope the context has seen stays listed, at 0)
    finally:
        prof.profile_enable(0)
    return np.array(poses, copy=True), np.array(cnn, copy=True), counts


def launch_counts(env, entry):
    """{label: {"1": counts with the solves bracketed alone, "2": counts with every phase bracketed}}"""
    return {label: {str(level): run_good(env, entry, label, form, kw, level)[2] for level in (1, 2)} for label, form, kw in good_calls(entry)}


# ---- the faults: entry -> [(label, form, context, changed arguments)] ---------------------------------------------------------------------------------------------
MARK = "ht_reserve_hands: a frame of 1 to 640x480 pixels"      # what ht_last_error holds before every faulty call (a call that sets no message leaves it)


def _fault_list(env, entry, form):
    names = SIG[(entry, form)].split()
    two, sized, framed = entry in TWO, entry in SIDED and entry != "direct", "w" in names
    ptrs = [p for p in ("main", "depth", "cams", "poses") if p in names and not (entry == "cnn_model" and p == "poses")]
    f = [("null context", {"ctx": None}), ("batch 0", {"B": 0}), ("batch over", {"B": CAP + 1})]
    if two:
        f.append(("2B over", {"B": CAP // 2 + 1}))
    f += [("null " + p, {p: None}) for p in ptrs]
    f += [("null %s + batch 0" % p, {p: None, "B": 0}) for p in ptrs[:1]]
    if "side" in names:
        own = {"_frames": "c128"} if entry == "direct" else {}      # (the direct calls read side x side pixels)
        f += [("side 96", {"side": 96}), ("side 96 + null depth", {"side": 96, "depth": None}), ("side 128 no weights", dict(own, side=128, _ctx="ctx64"))]
        if two:
            f.append(("2B over + side 96", {"B": CAP // 2 + 1, "side": 96}))
    if framed:
        f += [("66x66", {"w": 66, "h": 66}), ("644x480", {"w": 644, "h": 480, "_big": 1}), ("point limit", {"w": 640, "h": 480, "_big": 1, "_sf1": 1})]
    if sized:
        f += [("side 96 + 66x66", {"side": 96, "w": 66, "h": 66}), ("66x66 + side 128 no weights", {"side": 128, "w": 66, "h": 66, "_ctx": "ctx64"}),
              ("side 128 no weights + point limit", {"side": 128, "w": 640, "h": 480, "_big": 1, "_sf1": 1, "_ctx": "ctx64"})]
    if form == "dev" and entry in ("direct", "frames_sized", "hands"):
        f += [("misaligned 128", {"side": 128, "_frames": "c128", "_off": 2}), ("misaligned 128 no weights", {"side": 128, "_frames": "c128", "_off": 2, "_ctx": "ctx64"})]
    if form == "dev" and entry == "hands":
        f.append(("misaligned 128 with flags", {"side": 128, "_frames": "c128", "_off": 2, "_hands": 1}))      # good: the transform reads the context's staging
    if two:
        f += [("unknown split flag", {"flags": 8}), ("66x66 + unknown split flag", {"w": 66, "h": 66, "flags": 8}), ("far below range_hi", {"far": 600})]
    if entry == "two_hands_model":
        f += [("negative mode", {"mode": -1}), ("negative mode + unknown split flag", {"mode": -1, "flags": 8}), ("66x66 + negative mode", {"w": 66, "h": 66, "mode": -1}),
              ("negative max_dist", {"maxdist": -1.0})]
    if entry == "job_start":
        f += [("the same context twice", {"main": "job"}), ("batch 0 + null main", {"B": 0, "main": None})]
    return f


def run_faults(env, entry):
    """{"<form>: <label>": [return code, ht_last_error]} in the table's order"""
    out = {}
    for form in ("sync", "dev"):
        if (entry, form) not in SIG:
            continue
        for label, ch in _fault_list(env, entry, form):
            ch = dict(ch)
            ctx = getattr(env, ch.pop("_ctx", "ctx"))
            if entry == "job_start" and ctx is env.ctx64:
                continue
            frames = ch.pop("_frames", "tile" if entry in ("update", "direct") else "qvga")
            a = env.args(entry, form, frames=frames, side=64, hands=MIXED if ch.pop("_hands", 0) else None, ctx=ctx)
            if ch.pop("_big", 0):
                a["depth"] = env.big[:a["B"]] if form == "sync" else _dev(env.big[:a["B"]])
            off = ch.pop("_off", 0)
            if off:      # the same frames one pixel into an allocation
                d = torch.zeros(a["depth"].numel() + 16, dtype=torch.uint8, device=DEV); d[off:off + a["depth"].numel()] = a["depth"]; a["_base"] = d; a["depth"] = d.data_ptr() + off
            sf1 = ch.pop("_sf1", 0)
            if ch.get("main") == "job":
                ch["main"] = env.job.h
            a.update(ch)
            h = a["ctx"]
            if sf1:
                ctx.set_params(subsample_fraction=1)
            try:
                if h is not None:
                    assert env.L.ht_reserve_hands(h, 0, 0) == 1 and env.L.ht_last_error(h).decode() == MARK
                before = ctx.point_capacity()
                torch.cuda.synchronize()
                rc = env.call(entry, form, a)
                msg = env.L.ht_last_error(h).decode()
                if rc == 0:
                    ctx.tracker_flags(1)
                assert ctx.point_capacity() == before or rc == 0, (entry, form, label)      # a refused call has grown nothing
            finally:
                if sf1:
                    ctx.set_params(subsample_fraction=4)
            out["%s: %s" % (form, label)] = [rc, msg]
    return out
