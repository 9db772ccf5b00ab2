"""CPU-only checks of the sensor-simulation calls (ht_sensor_noise_default, ht_sensor_simulate*): declared, exported and bound with the documented signatures,
the noise struct's layout against the header, the default sets, every refusal without a device, the C++ facade, and what the compiler made of the kernel."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sensor_ref as R
import sensor_sim_frames as F
import sensor_sim_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "ht_sensor_noise_default": "int kind, float depth_scale, float far, ht_sensor_noise *out",
    "ht_sensor_simulate": "ht_ctx *ctx, int kind, const uint16_t *depth, int w, int h, int B, const ht_sensor_noise *noise, uint16_t *depth_out, uint8_t *ir_out",
    "ht_sensor_simulate_dev": "ht_ctx *ctx, int kind, const uint16_t *d_depth, int w, int h, int B, const ht_sensor_noise *noise, uint16_t *d_depth_out, uint8_t *d_ir_out, void *stream",
}
DEFAULT_IVY = dict(seed=0, first_index=0, far_count=3999, sigma0_256=128, sigma2=537, edge_step=20, slope_step=15, p_edge_drop=22938, p_edge_fly=16384, p_slope_drop=32768, p_hole=131,
                   fly_bg_count=3999, disparity_k=0, wall_count=0, ir_floor=16, ir_gain=125000, ir_noise=8)
DEFAULT_DS4 = dict(DEFAULT_IVY, sigma0_256=51, sigma2=1074, p_edge_drop=16384, p_edge_fly=22938, p_hole=655, disparity_k=683200)


def _header():
    return open(os.path.join(ROOT, "include", "ht_mi355x.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from hand_tracking_samples_amd import native
    L = native.load()
    header = _header()
    nm = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    for name, args in NEW.items():
        assert "int %s(%s);" % (name, args) in header, name
        assert name in exported and name in native.SYMBOLS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == args.count(",") + 1, name
    for method in ("sensor_simulate", "sensor_simulate_dev"):
        assert callable(getattr(native.Context, method))
    for words in ("NOBODY HAS MEASURED THESE FIGURES AGAINST A", "not a\n *                       calibrated model", "frays inwards only", "0x9E3779B97F4A7C15", "0xD6E8FEB86659FD93", "0xA0761D6478BD642F", "9472"):
        assert words in header, words


def test_the_struct_is_the_headers_field_for_field():
    from hand_tracking_samples_amd import native
    header = _header()
    body = header[header.index("typedef struct ht_sensor_noise"):header.index("} ht_sensor_noise;")]
    fields = []
    for line in body.splitlines():
        m = re.match(r"\s*(uint64_t|int)\s+([a-z0-9_, ]+);", line)
        if m:
            fields += [(n.strip(), m.group(1)) for n in m.group(2).split(",")]
    assert [n for n, _ in fields] == list(S.FIELDS) == [n for n, _ in native.SensorNoise._fields_]
    for (n, t), (_, ct) in zip(fields, native.SensorNoise._fields_):
        assert ct is (C.c_uint64 if t == "uint64_t" else C.c_int), n
    assert C.sizeof(native.SensorNoise) == 80 and native.SensorNoise.far_count.offset == 16 and native.SensorNoise.ir_noise.offset == 72
    n = native.SensorNoise(seed=(1 << 64) - 1, p_hole=5)
    m = n.but(p_hole=9, wall_count=3)
    assert (n.p_hole, n.wall_count, m.p_hole, m.wall_count, m.seed) == (5, 0, 9, 3, (1 << 64) - 1)
    with pytest.raises(TypeError):
        n.but(p_whole=1)


def test_noise_default_for_both_kinds():
    from hand_tracking_samples_amd import native
    L = native.load()
    for kind, want in ((native.SENSOR_IVY, DEFAULT_IVY), (native.SENSOR_DS4, DEFAULT_DS4)):
        n = native.sensor_noise_default(kind, 0.001, 4.0)
        assert {k: getattr(n, k) for k in S.FIELDS} == want
        assert S.check(kind, S.Noise(**want), 320, 240, 1) is None
    for scale, far in ((0.001, 4.0), (0.000125, 4.0), (0.0001, 4.0), (0.001, 1.5), (0.01, 4.0), (0.00025, 8.0)):      # far_count as FilterIvy forms its constant; every figure inside its range
        for kind in (0, 1):
            n = native.sensor_noise_default(kind, scale, far)
            q = np.float32(far) / np.float32(scale)
            assert n.far_count == (int(q) & 0xFFFF) and (far != 4.0 or n.far_count == R.ivy_fill(scale)), (scale, far)
            assert S.check(kind, S.Noise(**{k: getattr(n, k) for k in S.FIELDS}), 320, 240, 1) is None, (scale, far)
            c = 1.0 / float(np.float32(scale))
            assert n.sigma0_256 == int(256 * (0.0002 if kind else 0.0005) * c + 0.5) and n.edge_step == int(0.02 * c + 0.5) and n.disparity_k == (int(305 * 0.07 * 32 * c + 0.5) if kind else 0)
    keep = native.SensorNoise(seed=77, p_hole=5)
    for kind, scale, far in ((2, 0.001, 4.0), (-1, 0.001, 4.0), (0, 0.0, 4.0), (1, -0.001, 4.0), (0, float("nan"), 4.0), (0, 0.001, 0.0), (0, 0.001, -1.0), (0, 0.001, float("nan")),
                             (0, 2.0 ** -14, 8.0)):      # the last: 131072 counts, whose low 16 bits are 0
        assert L.ht_sensor_noise_default(kind, scale, far, C.byref(keep)) == 1, (kind, scale, far)
        with pytest.raises(ValueError):
            native.sensor_noise_default(kind, scale, far)
    assert (keep.seed, keep.p_hole) == (77, 5)      # a refusal writes nothing
    assert L.ht_sensor_noise_default(0, 0.001, 4.0, None) == 1
    assert native.sensor_noise_default(1, seed=5, p_hole=0).p_hole == 0 and native.sensor_noise_default(1, seed=5).seed == 5


def test_every_refusal_on_a_null_context_writes_nothing():
    from hand_tracking_samples_amd import native
    L = native.load()
    d = np.full((2, 4, 4), 500, np.uint16); out = np.full((2, 4, 4), 7, np.uint16); ir = np.full((2, 4, 4), 7, np.uint8)
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)); u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    base = native.sensor_noise_default(0)
    h = C.c_void_p()
    L.ht_create(b"/nonexistent/model.htfx", 1, 0, C.byref(h))
    cases = [dict()] + F.refusals(u16(d))
    assert len(cases) > 30
    try:
        for ctx in (None, h):
            for kw in cases:
                a = dict(dict(kind=0, depth=u16(d), w=4, h=4, B=2, noise=True, out=u16(out), ir=u8(ir)), **{k: v for k, v in kw.items() if k != "nz"})
                nz = None if a["noise"] is None else C.byref(base.but(**kw.get("nz", {})))
                assert L.ht_sensor_simulate(ctx, a["kind"], a["depth"], a["w"], a["h"], a["B"], nz, a["out"], a["ir"]) != 0, kw
                dev = lambda p: None if p is None else C.cast(p, C.c_void_p)
                assert L.ht_sensor_simulate_dev(ctx, a["kind"], dev(a["depth"]), a["w"], a["h"], a["B"], nz, dev(a["out"]), dev(a["ir"]), None) != 0, kw
        assert (out == 7).all() and (ir == 7).all() and (d == 500).all()
    finally:
        if h:
            L.ht_destroy(h)
    for kw in cases[1:]:      # the restatement's check names the same refusals
        if "nz" in kw:
            assert S.check(S.IVY, S.Noise(**{k: getattr(base, k) for k in S.FIELDS}).but(**kw["nz"]), 4, 4, 2) is not None, kw
    assert S.check(S.IVY, S.Noise(**{k: getattr(base, k) for k in S.FIELDS}), 4, 4, 2) is None and S.check(S.DS4, S.Noise(), 4, 4, 2, ir_given=False) == "ir"


def test_the_accepted_ranges_keep_every_intermediate_inside_its_width():
    """the reasons behind the ranges the header gives: s(d) * g + 4736 inside 31 bits, 2K + d1 inside 32, the shift of sigma2 * d * d inside 25"""
    s_max = 65536 + ((4096 * 65535 * 65535) >> 20)
    assert s_max * 126 + 4736 < 1 << 31 and -(s_max * 126) + 4736 > -(1 << 31)
    assert 2 * (1 << 30) + 65535 < 1 << 32 and 65535 * 65535 < 1 << 32 and 65535 * 255 < 1 << 31 and 63 * 65536 < 1 << 31
    assert abs(math.sqrt(4 * (64 * 64 - 1) / 12) - 36.95) < 0.005      # the sd of g, a sum of four uniform 6-bit fields


def test_cxx_sensor_sim_example_compiles_and_links(tmp_path):
    """include/ht_handtrack.hpp's SensorNoise, RSCam::SimulateIvy / SimulateDS4 / cache_ir build with plain g++ against the C-ABI library"""
    from hand_tracking_samples_amd import native
    native.load()
    exe = str(tmp_path / "sensor_sim")
    libdir = os.path.dirname(native.lib_path())
    subprocess.check_call(["g++", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cxx_sensor_sim_example.cpp"), "-o", exe, "-L" + libdir, "-lht_mi355x", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "model_hand17.htfx")], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stdout      # the defaults answered without a device; the simulation fails loudly, no fallback


def test_the_simulation_kernel_uses_no_scratch_and_spills_nothing():
    """k_sensor_simulate for 8, 4, 2 pixels a thread and for single pixels, each without scratch or spills"""
    from hand_tracking_samples_amd import build
    u = build.resource_usage()
    if not any("k_sensor_simulate" in n for n in u):
        build.build(force=True, verbose=False)
        u = build.resource_usage()
    k = {n: v for n, v in u.items() if "k_sensor_simulate" in n}
    print("\n".join("%s VGPRs %d SGPRs %d LDS %d occupancy %d" % (n, v["VGPRs"], v.get("TotalSGPRs", -1), v["LDS Size"], v["Occupancy"]) for n, v in sorted(k.items())))
    assert sorted(re.search(r"ILi(\d)E", n).group(1) for n in k) == ["1", "2", "4", "8"]
    for n, v in k.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["LDS Size"] == 0, (n, v)
