"""CPU-only checks of the scene rasteriser's definition (ht_model_raster_scene, include/ht_mi355x.h): the host equals the numpy restatement
(tests/scene_raster_ref.py) bit for bit on every output, on scenes that overlap, tie and hide an instance; one right hand is ht_model_raster_mesh; a left instance is
the mirror composition at pixel offset 0 and the directly mirrored model at both offsets; the background rule; the refusals; the exported symbols, the shared
pieces of csrc/ht_raster.hpp and the kernel's resources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_ray
import mirror_ref
import scene_raster_ref as S
from test_render_mesh_abi import CAM, H, MODELS, OFFSETS, ROOT, W, _poses      # 24x18, six seeded poses, both (offset, far) conventions
from test_raster_mesh_ref import CAM80, H80, W80

W37, H37 = 37, 29      # an odd width: the column flip and the write-out's groups of four
R, L, A = S.RIGHT, S.LEFT, S.ABSENT


def cam_of(w):
    """the application's camera scaled by w / 320, as CAM and CAM80 are"""
    return np.array([305 * w / 320.0, 305 * w / 320.0, 160 * w / 320.0, 120 * w / 320.0, 0.001, 0, 0, 0, 0, 0, 0, 1], np.float32)


CAMS = {(W, H): CAM, (W37, H37): cam_of(W37), (W80, H80): CAM80}
# Which of the six poses make the scenes, per hand.  Measured with the restatement at 24x18, offset 0 / offset 0.5:
#   17 bones  pair [R p0, L p1]: 28 / 25 pixels covered by two or more instances; trio [R p0, R p1, L p2]: 39 / 34 such pixels, wins 21 2 22 / 20 5 22;
#             tie [R p0, L p0]: 35 / 33 such pixels, 12 / 12 of them with equal counts; behind [R p3, R p3 + 3 mm]: 37 / 32 such pixels, the second wins 0
#   26 bones  pair [R p0, L p4]: 34 / 32 (with p1, as for 17 bones, only 9 / 10: the hands barely overlap); trio [R p0, R p1, L p2]: 30 / 42, wins 32 15 16 / 29 20 18;
#             tie [R p0, L p0]: 38 / 39, equal counts on 11 / 13; behind: 33 / 40, the second wins 0
PICK = {17: dict(pair=(0, 1), trio=(0, 1, 2), tie=0, behind=3), 26: dict(pair=(0, 4), trio=(0, 1, 2), tie=0, behind=3)}


def scenes(nb):
    """name -> (poses [H,nb,7], flags): a left instance's poses are taken as the left hand's, as the camera sees it"""
    P, k = _poses(nb), PICK[nb]
    back = P[k["behind"]].copy(); back[:, 2] += np.float32(0.003)
    a, b, c = k["trio"]
    return dict(pair=(np.stack([P[k["pair"][0]], P[k["pair"][1]]]), [R, L]), trio=(np.stack([P[a], P[b], P[c]]), [R, R, L]), tie=(np.stack([P[k["tie"]], P[k["tie"]]]), [R, L]),
                behind=(np.stack([P[k["behind"]], back]), [R, R]), absent=(np.stack([P[a], P[b], P[c]]), [R, A, L]), four=(np.stack([P[0], P[1], P[2], P[3]]), [R, 7, R, L]))


def _same(host, ref):
    depth, hand, body, visible = host
    return np.array_equal(depth, ref["depth"]) and np.array_equal(hand, ref["hand"]) and np.array_equal(body, ref["body"]) and np.array_equal(visible, ref["visible"])


def _multi(ref):
    return int((sum((l[1] >= 0).astype(int) for l in ref["layers"] if l is not None) >= 2).sum())


@pytest.fixture(scope="module", params=[17, 26])
def world(request):
    """per hand: the host model, the float32 mesh and, per (size, scene, convention), the host's outputs beside the restatement's; computed once, left unchanged"""
    from hand_tracking_samples_amd import native
    nb = request.param
    m = native.HostModel(MODELS[nb])
    corners = [m.sdmesh(b).reshape(-1, 3, 3) for b in range(nb)]
    com = np.stack([m.com(b) for b in range(nb)])
    m32 = mesh_ray.Mesh(corners, com, np.float32)
    rec = []
    for (w, h), cam in CAMS.items():
        for name, (poses, flags) in scenes(nb).items():
            for off, far in OFFSETS:
                if w == W80 and (name != "trio" or off != 0.5):      # 80x60 once
                    continue
                rec.append(dict(w=w, h=h, cam=cam, name=name, poses=poses, flags=flags, off=off, far=far, host=m.raster_scene(poses, cam, w, h, np.array(flags, np.uint8), far, off),
                                ref=S.render(m32, poses, flags, cam, w, h, far, off)))
    yield dict(nb=nb, model=m, m32=m32, rec=rec)
    m.close()


def test_host_equals_the_numpy_restatement_bit_for_bit(world):
    assert len(world["rec"]) == 2 * 6 * 2 + 1
    for r in world["rec"]:
        assert _same(r["host"], r["ref"]), (r["w"], r["name"], r["off"])
        depth, hand, body, visible = r["host"]
        assert ((hand >= 0) == (body >= 0)).all() and int(visible.sum()) == int((hand >= 0).sum())
        assert (depth[hand < 0] == np.uint16(int(np.float32(r["far"]) / r["cam"][4]))).all()
        for i, f in enumerate(r["flags"]):
            assert int(visible[i]) == int((hand == i).sum()) and (f != A or visible[i] == 0)


def test_the_scenes_overlap_tie_and_hide(world):
    """what keeps the comparison above from being vacuous, on the restatement at 24x18"""
    seen = 0
    for r in world["rec"]:
        if r["w"] != W:
            continue
        ref, name = r["ref"], r["name"]
        print("bones %d, offset %.1f, %s: %d pixels under two or more instances, wins %s" % (world["nb"], r["off"], name, _multi(ref), ref["visible"]))
        if name in ("pair", "trio", "tie", "behind"):
            assert _multi(ref) >= 20
        if name == "trio":
            assert (ref["visible"] >= 1).all()
        if name == "tie":
            (c0, b0), (c1, b1) = ref["layers"]
            equal = (b0 >= 0) & (b1 >= 0) & (c0 == c1)
            print("    equal counts on %d pixels" % int(equal.sum()))
            assert int(equal.sum()) >= 8 and (ref["hand"][equal] == 0).all()      # the lowest instance keeps them
        if name == "behind":
            assert ref["visible"][1] == 0 and ref["visible"][0] > 20
        if name == "absent":
            assert ref["layers"][1] is None and ref["visible"][1] == 0 and ref["visible"][0] > 0 and ref["visible"][2] > 0
        if name == "four":
            assert (ref["visible"] > 0).sum() >= 3
        seen += 1
    assert seen == 12


def test_one_right_hand_is_the_mesh_rasteriser(world):
    m = world["model"]
    for p in _poses(world["nb"])[:3]:
        for off, far in OFFSETS:
            for flags in (None, np.array([R], np.uint8)):
                depth, hand, body, visible = m.raster_scene(p[None], CAM, W, H, flags, far, off)
                want, wbody = m.raster_mesh(p, CAM, W, H, far, off)
                assert np.array_equal(depth, want) and np.array_equal(body, wbody) and np.array_equal(hand, np.where(wbody >= 0, 0, -1)) and visible[0] == (wbody >= 0).sum()


def test_a_left_instance_is_the_mirror_composition_at_offset_0(world):
    """mirror poses, mirror camera, render, mirror the frame: section 26's composition, whose camera is the whole-pixel convention's"""
    m = world["model"]
    off_centre = CAM.copy(); off_centre[2] += 3.25
    for p in _poses(world["nb"])[:3]:
        for cam in (CAM, off_centre):
            depth, hand, body, _ = m.raster_scene(p[None], cam, W, H, np.array([L], np.uint8), 4.0, 0.0)
            d, b = m.raster_mesh(mirror_ref.poses(p), mirror_ref.cams(cam[None], W)[0], W, H, 4.0, 0.0)
            assert (b >= 0).any() and np.array_equal(depth, mirror_ref.frames(d[None])[0]) and np.array_equal(body, b[:, ::-1])


MEASURED_MIRRORED_MODEL_SHARE = 0.0      # pixels (depth or body) on which a left instance differs from the mirrored model's frame: 0 of 12 frames' pixels, per hand and size


@pytest.mark.parametrize("w,h", [(W, H), (W37, H37)])
def test_a_left_instance_is_the_directly_mirrored_model(world, w, h):
    """geometry, not an identity: ht_model_mirror's meshes at the instance's poses through the unmirrored camera.  The plain ht_mirror_cams camera at offset 0.5 must miss it widely."""
    from hand_tracking_samples_amd import native
    mm = native.HostModel(MODELS[world["nb"]]); mm.mirror()
    m = world["model"]
    cam = cam_of(w); cam[2] += 3.25      # a principal point off the centre
    try:
        diff = total = covered = plain_diff = 0
        for p in _poses(world["nb"]):
            for off, far in OFFSETS:
                depth, _, body, _ = m.raster_scene(p[None], cam, w, h, np.array([L], np.uint8), far, off)
                want, wbody = mm.raster_mesh(p, cam, w, h, far, off)
                diff += int(((depth != want) | (body != wbody)).sum()); total += depth.size; covered += int((wbody >= 0).sum())
                if off == 0.5:
                    d, b = m.raster_mesh(mirror_ref.poses(p), mirror_ref.cams(cam[None], w)[0], w, h, far, off)
                    plain_diff += int(((d[:, ::-1] != want) | (b[:, ::-1] != wbody)).sum())
        print("bones %d, %dx%d: a left instance differs from the mirrored model on %d of %d pixels (%d covered); the plain mirror camera at offset 0.5 on %d"
              % (world["nb"], w, h, diff, total, covered, plain_diff))
        assert covered > 30 * 12      # the hand is in the frames
        assert diff / float(total) <= 2 * MEASURED_MIRRORED_MODEL_SHARE
        assert plain_diff > covered // 8      # half of `covered` is the offset 0.5 frames': more than a quarter of their hand pixels are wrong
    finally:
        mm.close()


def test_background(world):
    m, m32, nb = world["model"], world["m32"], world["nb"]
    poses, flags = scenes(nb)["trio"]
    fl = np.array(flags, np.uint8)
    for off, far in OFFSETS:
        free = S.render(m32, poses, flags, CAM, W, H, far, off)
        on = free["hand"] >= 0
        lo, hi = int(free["depth"][on].min()), int(free["depth"][on].max())
        mid = int(np.median(free["depth"][on]))
        holes = np.full((H, W), mid, np.uint16); holes[::2, ::3] = 0; holes[1::4, 1::2] = 65535
        ties = np.where(on, free["depth"], 1).astype(np.uint16)      # count == bg on every hand pixel
        for name, bg in (("nearer", np.full((H, W), lo - 1, np.uint16)), ("between", np.full((H, W), mid, np.uint16)), ("beyond", np.full((H, W), hi + 1, np.uint16)),
                         ("zeros", np.zeros((H, W), np.uint16)), ("holes", holes), ("ties", ties)):
            ref = S.render(m32, poses, flags, CAM, W, H, far, off, bg=bg)
            host = m.raster_scene(poses, CAM, W, H, fl, far, off, bg=bg)
            assert _same(host, ref), (name, off)
            depth, hand = host[0], host[1]
            assert np.array_equal(depth[hand < 0], bg[hand < 0])
            if name == "nearer":
                assert (hand < 0).all() and np.array_equal(depth, bg)
            if name == "between":
                assert 0 < (hand >= 0).sum() < on.sum()
            if name in ("beyond", "zeros", "ties"):
                assert np.array_equal(hand, free["hand"]) and np.array_equal(depth[on], free["depth"][on])
            if name == "zeros":
                assert (depth[~on] == 0).all()
            if name == "holes":
                assert np.array_equal(hand[::2, ::3], free["hand"][::2, ::3]) and np.array_equal(hand[1::4, 1::2], free["hand"][1::4, 1::2])
            work = bg.copy()      # bg == depth, in place
            again = m.raster_scene(poses, CAM, W, H, fl, far, off, bg=work, in_place=True)
            assert np.shares_memory(again[0], work) and _same(again, ref) and np.array_equal(work, ref["depth"])


def test_degenerate_scenes(world):
    m, nb = world["model"], world["nb"]
    poses, _ = scenes(nb)["trio"]
    bg = np.arange(W * H, dtype=np.uint16).reshape(H, W)
    for under in (None, bg):
        depth, hand, body, visible = m.raster_scene(poses, CAM, W, H, np.array([A, A, A], np.uint8), 4.0, 0.0, bg=under)
        assert (hand == -1).all() and (body == -1).all() and (visible == 0).all() and np.array_equal(depth, np.full((H, W), int(np.float32(4.0) / CAM[4]), np.uint16) if under is None else bg)
    behind = poses.copy(); behind[:, :, 2] = -behind[:, :, 2]
    depth, hand, body, visible = m.raster_scene(behind, CAM, W, H, np.array([R, L, R], np.uint8), 4.0, 0.0, bg=bg)
    assert (hand == -1).all() and (visible == 0).all() and np.array_equal(depth, bg)


def test_refusals():
    from hand_tracking_samples_amd import native
    Lb = native.load()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
    i8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int8))
    nan = float("nan")
    m = native.HostModel(MODELS[17])
    try:
        p = np.zeros((4, 17, 7), np.float32); p[:, :, 6] = 1; p[:, :, 2] = 0.5
        d = np.zeros((8, 8), np.uint16); hb = np.zeros((2, 8, 8), np.int8); vis = np.zeros(4, np.int32); flags = np.zeros(4, np.uint8)
        vp = vis.ctypes.data_as(C.POINTER(C.c_int32)); f8 = flags.ctypes.data_as(C.POINTER(C.c_uint8))
        call = lambda poses, cam, w, h, far, off, depth, H=2, bg=None, hand=None, body=None, v=None: Lb.ht_model_raster_scene(m.m, poses, f8, H, cam, w, h, far, off, bg, depth, hand, body, v)
        assert call(fp(p), fp(CAM), 8, 8, 4.0, 0.0, u16(d)) == 0      # every label output is optional
        assert Lb.ht_model_raster_scene(None, fp(p), f8, 2, fp(CAM), 8, 8, 4.0, 0.0, None, u16(d), None, None, None) != 0
        # null, non-finite and out-of-range arguments: ht_model_raster_mesh's codes
        for args in ((None, fp(CAM), 8, 8, 4.0, 0.0, u16(d)), (fp(p), None, 8, 8, 4.0, 0.0, u16(d)), (fp(p), fp(CAM), 8, 8, 4.0, 0.0, None), (fp(p), fp(CAM), 0, 8, 4.0, 0.0, u16(d)),
                     (fp(p), fp(CAM), 8, 4097, 4.0, 0.0, u16(d)), (fp(p), fp(CAM), 8, 8, 0.0, 0.0, u16(d)), (fp(p), fp(CAM), 8, 8, nan, 0.0, u16(d)), (fp(p), fp(CAM), 8, 8, 4.0, nan, u16(d)),
                     (fp(p), fp(CAM), 8, 8, 4.0, -0.25, u16(d)), (fp(p), fp(CAM), 8, 8, 4.0, 1.25, u16(d))):
            rc = call(*args)
            assert rc != 0 and rc == Lb.ht_model_raster_mesh(m.m, *args, None)
        for H_ in (0, 5, -1):
            assert call(fp(p), fp(CAM), 8, 8, 4.0, 0.0, u16(d), H=H_) == 1      # HT_ERR_ARG
        # overlapping buffers: only bg == depth, exactly, is allowed
        big = np.zeros(8 * 8 + 8, np.uint16)
        assert call(fp(p), fp(CAM), 8, 8, 4.0, 0.0, u16(big[4:]), bg=u16(big)) == 1
        assert call(fp(p), fp(CAM), 8, 8, 4.0, 0.0, u16(big), bg=u16(big)) == 0
        assert call(fp(p), fp(CAM), 8, 8, 4.0, 0.0, u16(d), hand=i8(hb[0]), body=i8(hb[0])) == 1
        assert call(fp(p), fp(CAM), 8, 8, 4.0, 0.0, u16(d), hand=i8(hb[0]), body=i8(hb.reshape(-1)[32:])) == 1
        assert call(fp(p), fp(CAM), 8, 8, 4.0, 0.0, u16(d), hand=C.cast(u16(d), C.POINTER(C.c_int8))) == 1
        assert call(fp(p), fp(CAM), 8, 8, 4.0, 0.0, u16(d), hand=i8(hb[0]), body=i8(hb[1]), v=vp) == 0
    finally:
        m.close()
    # a context that never came up (no device here, or a missing model): every call fails as the mesh rasteriser's does, and does not crash
    h = C.c_void_p()
    Lb.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    poses = np.zeros((1, 2, 17, 7), np.float32); cams = np.zeros((1, 12), np.float32); depth = np.zeros((1, 8, 8), np.uint16); fl = np.zeros((1, 2), np.uint8)
    f8 = fl.ctypes.data_as(C.POINTER(C.c_uint8))
    try:
        assert Lb.ht_raster_scene_depth(None, fp(poses), f8, 2, fp(cams), 8, 8, 4.0, 0.0, 1, None, u16(depth), None, None, None) != 0
        assert Lb.ht_raster_scene_depth_dev(None, poses.ctypes.data, fl.ctypes.data, 2, cams.ctypes.data, 8, 8, 4.0, 0.0, 1, None, depth.ctypes.data, None, None, None, None) != 0
        for H_, a in ((2, (fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, u16(depth))), (2, (None, fp(cams), 8, 8, 4.0, 0.0, 1, u16(depth))), (2, (fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, None)),
                      (2, (fp(poses), fp(cams), 4097, 8, 4.0, 0.0, 1, u16(depth))), (2, (fp(poses), fp(cams), 8, 8, -1.0, 0.0, 1, u16(depth))), (2, (fp(poses), fp(cams), 8, 8, 4.0, nan, 1, u16(depth))),
                      (0, (fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, u16(depth))), (5, (fp(poses), fp(cams), 8, 8, 4.0, 0.0, 1, u16(depth)))):
            rc = Lb.ht_raster_scene_depth(h, a[0], f8, H_, a[1], *a[2:7], None, a[7], None, None, None)
            assert rc != 0 and rc == Lb.ht_raster_mesh_depth(h, *a, None)
            dev = [x if not hasattr(x, "contents") else C.cast(x, C.c_void_p) for x in a]
            rc = Lb.ht_raster_scene_depth_dev(h, dev[0], fl.ctypes.data, H_, dev[1], *dev[2:7], None, dev[7], None, None, None, None)
            assert rc != 0 and rc == Lb.ht_raster_mesh_depth_dev(h, *dev, None, None)
    finally:
        if h:
            Lb.ht_destroy(h)


def test_shared_pieces_of_the_definition(tmp_path):
    """csrc/ht_raster.hpp's scene functions, which host and kernel both call, on their own: the limit H * T <= 65535 on triangle counts no stock model has, the mirrored
    principal point's bits against the restatement's, the flags, the column flip and the composite rule"""
    from hand_tracking_samples_amd import build
    exe = str(tmp_path / "pieces")
    subprocess.check_call([build.HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
                           os.path.join(ROOT, "tests", "hip_scene_pieces.hip"), "-o", exe])
    out = subprocess.check_output([exe]).decode().split()
    want = []
    for Hn, T in ((1, 65535), (1, 65536), (2, 32767), (2, 32768), (3, 21845), (3, 21846), (4, 16383), (4, 16384), (4, 8896), (0, 10), (5, 10), (-1, 10), (4, 0)):
        want.append("fits %d %d %d" % (Hn, T, 1 if 1 <= Hn <= 4 and Hn * T <= 65535 else 0))
    for cx, w, off in ((12.0, 24, 0.0), (15.25, 24, 0.5), (18.5, 37, 0.5), (160.3, 320, 0.0), (160.3, 320, 0.5), (2047.7, 4096, 1.0), (-3.1, 7, 0.25)):
        want.append("px %08x" % int(np.array([S.mirror_px(np.float32(cx), w, off)], np.float32).view(np.uint32)[0]))
    for f in (0, 1, 7, 254, 255):
        want.append("flag %d %d %d" % (f, 1 if f == 255 else 0, 1 if f not in (0, 255) else 0))
    want += ["col %d" % c for c in (5, 31, 0, 36)]
    for count, has, bg in ((10, 0, 5), (10, 1, 0), (10, 1, 10), (10, 1, 9), (10, 1, 11), (0, 1, 0), (65535, 1, 65535), (65535, 1, 65534)):
        want.append("wins %d" % (1 if (not has or bg == 0 or count <= bg) else 0))
    assert " ".join(out) == " ".join(" ".join(want).split())


def test_scene_symbols_exported():
    from hand_tracking_samples_amd import native
    Lb = native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    for s in ("ht_raster_scene_depth", "ht_raster_scene_depth_dev", "ht_model_raster_scene"):
        assert s in native.SYMBOLS and s in exported and hasattr(Lb, s)
    text = open(os.path.join(ROOT, "include", "ht_mi355x.h")).read()
    assert "#define HT_SCENE_RIGHT 0" in text and "#define HT_SCENE_ABSENT 255" in text and "#define HT_SCENE_MAX_HANDS 4" in text
    assert (native.SCENE_RIGHT, native.SCENE_ABSENT, native.SCENE_MAX_HANDS) == (0, 255, 4)


def test_scene_kernel_resources():
    """one kernel, no scratch, no spills; the band's z-buffer and the one pose table leave room for two blocks in a CU's 160 KiB of LDS, at two waves a SIMD or more"""
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not any("k_raster_scene" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    k = {n: v for n, v in u.items() if "k_raster_scene" in n}
    assert len(k) == 1
    for n, v in k.items():
        print("%s VGPRs %d LDS %d scratch %d" % (n, v["VGPRs"], v["LDS Size"], v["ScratchSize"]))
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and 2 * v["LDS Size"] <= 163840 and v["Occupancy"] >= 2, (n, v)
