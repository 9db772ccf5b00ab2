"""What a hand model gives through the C ABI, as a table of hashes: the host view (ht_model_*) and a context (ht_create, ht_scale and what rides on them), in every
state the two are used in, and what both entries answer to files they refuse.

Shared by tests/test_host_model_record.py and tests/test_gpu_model_record.py (which compare) and tests/golden/make_host_model.py and make_model_record_gpu.py (which
recorded, once, from the commit before both entries were rebuilt on one host record of a model).  Everything goes through native.HostModel, native.Context and the
library they loaded; nothing here knows how a model is kept.
"""
import ctypes as C
import hashlib
import os

import numpy as np

import htfx
from hand_tracking_samples_amd import native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_RECORDING = os.path.join(HERE, "golden", "host_model.json")
GPU_RECORDING = os.path.join(HERE, "golden", "model_record_gpu.json")
ASSETS = os.path.join(ROOT, "hand_tracking_samples_amd", "assets")
MODELS = {"hand17": os.path.join(ASSETS, "model_hand17.htfx"), "hand26": os.path.join(ASSETS, "model_hand26.htfx"),
          "chain3": os.path.join(HERE, "golden", "model_chain3.json")}      # the last one is the JSON path through ht_build_model
STATES = {"opened": (), "scale": (1.15,), "mirror": ("m",), "mirror_scale": ("m", 1.15), "scale_mirror": (1.15, "m"), "scale_scale": (1.15, 0.9)}
GPU_MODELS = ("hand17", "hand26")
GPU_STATES = (("created", None), ("scale", 1.15), ("scale_scale", 0.9))      # one context walks through them: the factor brings it from the state before
AWAY = 0.18                                                                    # metres the rest pose is moved down the camera's axis
QVGA_CAM = np.array([305, 305, 160, 120, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)
# 16 directions with small integer components, none along an axis: the segments run 0.4 m either side of a body's rest position
DIRECTIONS = [(1, 2, 3), (-2, 1, 3), (3, -1, 2), (1, 1, 1), (-1, 2, -2), (2, 3, -1), (-3, -2, 1), (1, -3, 2), (2, -2, 3), (-1, -1, 3), (3, 2, 2), (-2, 3, 1), (1, 4, -2), (-4, 1, 2), (2, 1, -3), (-1, 3, 4)]
REMOVED = ("nb", "body_f", "b0/tris", "b0/planes", "joint_f", "physics")      # one baked file of model_chain3 without each


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def cam(w):
    """the application's camera scaled to a frame w pixels wide (4:3)"""
    c = QVGA_CAM.copy(); c[:4] *= w / 320.0
    return c


def bring(m, state):
    for op in STATES[state]:
        m.mirror() if op == "m" else m.scale(op)
    return m


def rest_poses(m):
    """the model's own rest pose [nb,7] as the host view hands it out, AWAY in front of the camera"""
    p = np.stack([m.body(b)[4] for b in range(m.nb)]).astype(np.float32)
    p[:, 2] += np.float32(AWAY)
    return p


def segments(poses):
    out = []
    for k, d in enumerate(DIRECTIONS):
        d = np.array(d, np.float64); d = d / np.sqrt((d * d).sum()) * 0.4
        c = poses[k % len(poses), :3].astype(np.float64)
        out.append(((c - d).astype(np.float32), (c + d).astype(np.float32)))
    return out


def host_state(m):
    """every getter, the two ray casts on the fixed segments and the two renderers' definitions, of a host model as it stands"""
    bodies = [m.body(b) for b in range(m.nb)]
    poses = rest_poses(m)
    hull = [m.hitcheck(poses, v0, v1) for v0, v1 in segments(poses)]
    mesh = [m.hitcheck_mesh(poses, v0, v1) for v0, v1 in segments(poses)]
    rd, rb = m.render_mesh(poses, cam(32), 32, 24); zd, zb = m.raster_mesh(poses, cam(32), 32, 24)
    lo, hi, sw = m.joint_limits()
    return {"counts": [m.nb, m.nj],
            "body": sha(*[np.concatenate([[len(v), len(t), len(p)], c.view(np.int32), r.view(np.int32)]).astype(np.int32) for v, t, p, c, r in bodies]),
            "body_mesh": sha(*[a for v, t, p, c, r in bodies for a in (v, t)]),
            "body_sdmesh": sha(*[m.sdmesh(b) for b in range(m.nb)]),
            "body_planes": sha(*[a for b in range(m.nb) for a in (bodies[b][2], m.sdmesh_planes(b))]),
            "joint_limits": sha(lo, hi, sw.astype(np.int32)),
            "hitcheck": sha(*[np.concatenate([i.view(np.int32), n.view(np.int32), [b]]).astype(np.int32) for i, n, b in hull]),
            "hitcheck_mesh": sha(*[np.concatenate([i.view(np.int32), n.view(np.int32), [b, t]]).astype(np.int32) for i, n, b, t in mesh]),
            "hits": [sum(1 for h in hull if h[2] >= 0), sum(1 for h in mesh if h[2] >= 0), int((rb >= 0).sum()), int((zb >= 0).sum())],      # that the hashes are of something
            "render_mesh": sha(rd, rb), "raster_mesh": sha(zd, zb)}


def refusal_files(tmp):
    """{name: path}: a path that does not exist, eight bytes of magic, model_chain3 baked without one entry each, and with 32 bodies claimed"""
    tmp = str(tmp)
    G = htfx.load(os.path.join(HERE, "golden", "model_chain3.htfx"))
    out = {"absent": os.path.join(tmp, "no_such_model.htfx"), "magic_only": os.path.join(tmp, "magic_only.htfx")}
    with open(out["magic_only"], "wb") as f:
        f.write(b"HTFX0001")
    for name in REMOVED:
        out["without_" + name] = p = os.path.join(tmp, "without_%s.htfx" % name.replace("/", "_"))
        htfx.save(p, {k: v for k, v in G.items() if k != name})
    out["bodies32"] = os.path.join(tmp, "bodies32.htfx")
    htfx.save(out["bodies32"], dict(G, nb=np.array([32], np.int32)))
    return out


def _told(text, files):
    for p in files.values():      # the texts name the path they were given: recorded without the directory
        text = text.replace(os.path.dirname(p) + os.sep, "")
    return text


def host_refusals(files):
    """{name: [return code, ht_model_error]} of ht_model_open"""
    L = native.load(); L.ht_model_error.restype = C.c_char_p
    out = {}
    for name, p in files.items():
        m = C.c_void_p()
        rc = L.ht_model_open(p.encode(), 1, C.byref(m))
        out[name] = [rc, _told(L.ht_model_error(m).decode(), files)]
        L.ht_model_close(m)
    return out


def host_recording(tmp):
    rec = {"models": {}, "refusals": host_refusals(refusal_files(tmp))}
    for name, path in MODELS.items():
        rec["models"][name] = {}
        for state in STATES:
            m = bring(native.HostModel(path), state)
            try:
                rec["models"][name][state] = host_state(m)
            finally:
                m.close()
    return rec


# ---- a context, on the device ----
def gpu_refusals(files):
    """{name: [return code, ht_last_error]} of ht_create"""
    L = native.load()
    out = {}
    for name, p in files.items():
        h = C.c_void_p()
        rc = L.ht_create(p.encode(), 1, 0, C.byref(h))
        out[name] = [rc, _told(L.ht_last_error(h).decode(), files)]
        L.ht_destroy(h)
    return out


def gpu_poses(ctx, rest):
    """the rest pose and one draw of the pose sampler about its root, as centre-of-mass poses [2,nb,7]"""
    return np.stack([rest, ctx.sample_poses(rest[:1], 23, 5, 0.9, com_poses=True)[0]])


def gpu_frames(ctx, poses):
    """the three renderers' frames with body labels at 80x60: {entry: (depth, body)}"""
    cams = np.tile(cam(80), (len(poses), 1))
    return {"render_depth": ctx.render_depth(poses, cams, 80, 60, want_body=True), "render_mesh_depth": ctx.render_mesh_depth(poses, cams, 80, 60, want_body=True),
            "raster_mesh_depth": ctx.raster_mesh_depth(poses, cams, 80, 60, want_body=True)}


def gpu_state(ctx, rest, golden):
    """what a context answers as it stands.  golden: (depth [4,4096], cams, start poses) for one update, or None"""
    poses = gpu_poses(ctx, rest)
    frames = gpu_frames(ctx, poses)
    squeezed = rest.copy(); squeezed[:, :3] = rest[:1, :3] + np.float32(0.6) * (rest[:, :3] - rest[:1, :3])      # the bodies drawn towards the palm: they overlap
    st = np.zeros((3, ctx.nb, native.STATE), np.float32); st[:2, :, :7] = poses; st[2, :, :7] = squeezed
    ctx.set_state(0, st)
    contacts, n = ctx.stage_contacts(0, 3)
    out = {k: sha(*v) for k, v in frames.items()}
    out["labelled"] = [int((v[1] >= 0).sum()) for v in frames.values()]
    out.update({"sampled": sha(poses[1]), "keypoint_table_feature8": sha(*ctx.keypoint_table(native.KP_FEATURE8)), "keypoint_table_skeleton": sha(*ctx.keypoint_table(native.KP_SKELETON)),
                "joint_coords": sha(ctx.joint_coords(poses, com_poses=True)), "contacts": sha(n, *[contacts[k, :n[k]] for k in range(3)]), "ncontacts": [int(x) for x in n]})
    if golden is not None:
        depth, cams, start = golden
        ctx.tracker_reset(start)
        out["update_poses"] = sha(ctx.update_sync(depth, cams))
        out["update_states"] = sha(ctx.get_state(0, 4), ctx.get_state(1, 4))
        out["update_flags"] = sha(*ctx.tracker_flags(4))
    return out


def golden4():
    g = htfx.load(os.path.join(HERE, "golden", "golden8.htfx"))
    return (np.stack([g["f%d/depth" % f].reshape(-1) for f in range(4)]), np.stack([g["f%d/cam" % f] for f in range(4)]), np.stack([g["f%d/startpose" % f] for f in range(4)]))


def gpu_walk(name, each):
    """one context of model `name` through GPU_STATES; each(state, ctx, rest poses of the unscaled model, golden frames or None) after every step"""
    from hand_tracking_samples_amd import weights as W
    m = native.HostModel(MODELS[name]); rest = rest_poses(m); m.close()
    ctx = native.Context(MODELS[name], 4)
    try:
        golden = golden4() if name == "hand17" else None
        if golden:
            ctx.load_weights(W.make_cnnb())
        for state, factor in GPU_STATES:
            if factor:
                ctx.scale(factor)
            each(state, ctx, rest, golden)
    finally:
        ctx.close()


def gpu_recording(tmp):
    rec = {"models": {n: {} for n in GPU_MODELS}, "refusals": gpu_refusals(refusal_files(tmp))}
    for name in GPU_MODELS:
        gpu_walk(name, lambda state, ctx, rest, golden: rec["models"][name].__setitem__(state, gpu_state(ctx, rest, golden)))
    return rec
