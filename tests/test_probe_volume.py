"""Probe volumes (include/ptmi_plugin.h Part 16) without a GPU: exports, struct layout, argument checks, the host twins against the
numpy restatement of the rule (tests/volume_ref.py) bit for bit, the properties the rule promises (constant distances, the
octahedral round trip, trilinear reproduction, the Chebyshev cut), the sanitizer build of the host twins and the compile-time
resources of the three kernels.  tests/test_gpu_probe_volume.py holds the kernels to the rule.

The depth record's C name is PTProbeDepthMap: C has one name space for a typedef and a function, and PTProbeDepth is the call."""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from kernel_resources import resources
import probe_ref
import volume_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
F = np.float32
CONTEXT_SYMBOLS = ["PTProbeDepth", "PTProbeDepthHost", "PTProbeGridIrradiance"]
HOST_SYMBOLS = ["PTProbeDepthProjectHost", "PTProbeGridIrradianceHost"]
EPS = 2.0 ** -23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def _grid(origin, spacing, counts, flags=0, bias=0.0):
    g = plugin.probe_grid_desc(origin, spacing, counts, wrap=bool(flags & 1), visibility=bool(flags & 2), normal_bias=bias)
    assert g.flags == flags
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_volume_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in CONTEXT_SYMBOLS + HOST_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 16: probe volumes" in header


def test_volume_structs_match_c_header():
    fields = {"PTProbeDepthMap": ["moments"], "PTProbeGrid": ["origin", "flags", "spacing", "normalBias", "counts", "reserved"]}
    lines = []
    for s, fs in fields.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    lines.append('printf("flags %u %u\\n", PT_GRID_WRAP, PT_GRID_VISIBILITY);')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTProbeDepthMap"]) == C.sizeof(abi.PTProbeDepthMap) == 512
    assert int(got["PTProbeGrid"]) == C.sizeof(abi.PTProbeGrid) == 48
    for s, fs in fields.items():
        for f in fs:
            assert int(got[f"{s}.{f}"]) == getattr(getattr(abi, s), f).offset, (s, f)
    assert [int(got[f"PTProbeGrid.{f}"]) for f in fields["PTProbeGrid"]] == [0, 12, 16, 28, 32, 44]
    assert got["flags"].split() == ["1", "2"] and (abi.PT_GRID_WRAP, abi.PT_GRID_VISIBILITY) == (1, 2)


def _bad_grids():
    ok = dict(origin=(0, 0, 0), spacing=(1, 1, 1), counts=(2, 2, 2))
    cases = {}
    for name, change in {"flag": dict(flags=4), "flag high": dict(flags=0x80000001), "reserved": dict(reserved=1),
                         "count 0": dict(counts=(2, 0, 2)), "count 1025": dict(counts=(2, 2, 1025)),
                         "spacing 0": dict(spacing=(0, 1, 1)), "spacing negative": dict(spacing=(1, -1, 1)),
                         "spacing inf": dict(spacing=(1, 1, math.inf)), "spacing nan": dict(spacing=(math.nan, 1, 1)),
                         "bias negative": dict(bias=-0.5), "bias inf": dict(bias=math.inf), "bias nan": dict(bias=math.nan)}.items():
        g = plugin.probe_grid_desc(change.get("origin", ok["origin"]), change.get("spacing", ok["spacing"]), change.get("counts", ok["counts"]),
                                   wrap=False, visibility=False, normal_bias=change.get("bias", 0.0))
        g.flags = change.get("flags", 0)
        g.reserved = change.get("reserved", 0)
        cases[name] = g
    return cases


def test_volume_argument_errors():
    """every refusal of Part 16 that needs no scene: the context's entry points check their arguments before they touch the GPU"""
    lib = plugin.load_library()
    buf = (C.c_float * 1024)()
    a = (C.addressof(buf) + 15) & ~15
    ok = _grid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    calls = {"PTProbeDepth": lambda: lib.PTProbeDepth(None, a, 1, 0, 4, 1.0, a),
             "PTProbeDepthHost": lambda: lib.PTProbeDepthHost(None, a, 1, 0, 4, 1.0, a),
             "PTProbeGridIrradiance": lambda: lib.PTProbeGridIrradiance(None, C.byref(ok), a, a, a, 1, a)}
    for name, call in calls.items():
        assert call() == abi.PT_ERR_INVALID_ARG, name
        assert b"ctx" in lib.PTGetLastError() and name.encode() in lib.PTGetLastError()
    ctx = C.c_void_p(1)         # never dereferenced: every call below is refused on its arguments alone
    for name, g in _bad_grids().items():
        assert lib.PTProbeGridIrradiance(ctx, C.byref(g), a, a, a, 1, a) == abi.PT_ERR_INVALID_ARG, name
        assert lib.PTProbeGridIrradianceHost(C.byref(g), a, a, a, 1, a) == 0 and lib.PTGetBVHBuildError() != b"", name
    assert lib.PTProbeGridIrradiance(ctx, None, a, a, a, 1, a) == abi.PT_ERR_INVALID_ARG
    vis = _grid((0, 0, 0), (1, 1, 1), (2, 2, 2), flags=abi.PT_GRID_VISIBILITY)
    assert lib.PTProbeGridIrradiance(ctx, C.byref(vis), a, None, a, 1, a) == abi.PT_ERR_INVALID_ARG and b"depth" in lib.PTGetLastError()
    assert lib.PTProbeGridIrradianceHost(C.byref(vis), a, None, a, 1, a) == 0 and b"depth" in lib.PTGetBVHBuildError()
    for args in ((None, a, a, a), (a, a, None, a), (a, a, a, None)):
        assert lib.PTProbeGridIrradiance(ctx, C.byref(ok), args[0], args[1], args[2], 1, args[3]) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    for args in ((a + 8, a, a, a), (a, a + 8, a, a), (a, a, a + 4, a), (a, a, a, a + 8)):
        assert lib.PTProbeGridIrradiance(ctx, C.byref(ok), args[0], args[1], args[2], 1, args[3]) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    for fn in (lib.PTProbeDepth, lib.PTProbeDepthHost):
        for bad in (0.0, -1.0, math.inf, math.nan, abi.PT_FAR_PLANE):
            assert fn(ctx, a, 1, 0, 4, bad, a) == abi.PT_ERR_INVALID_ARG and b"maxDistance" in lib.PTGetLastError(), bad
        for bad in (0, 65537):
            assert fn(ctx, a, 1, 0, bad, 1.0, a) == abi.PT_ERR_UNSUPPORTED and b"samples" in lib.PTGetLastError(), bad
        assert fn(ctx, None, 1, 0, 4, 1.0, a) == abi.PT_ERR_INVALID_ARG and fn(ctx, a, 1, 0, 4, 1.0, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTProbeDepth(ctx, a + 8, 1, 0, 4, 1.0, a) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    assert lib.PTProbeDepth(ctx, a, 1, 0, 4, 1.0, a + 8) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    # the host twins: 0 and a message
    pos = np.zeros((1, 3), F)
    for bad in (0.0, -1.0, math.inf, math.nan, abi.PT_FAR_PLANE):
        with pytest.raises(plugin.PluginError, match="maxDistance"):
            plugin.probe_depth_project(pos, np.ones((1, 4), F), bad)
    with pytest.raises(plugin.PluginError, match="samples"):
        plugin.probe_depth_project(pos, np.ones((1, 0), F), 1.0)
    assert lib.PTProbeDepthProjectHost(None, 1, 0, 4, a, 1.0, a) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTProbeGridIrradianceHost(C.byref(ok), None, a, a, 1, a) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert plugin.probe_depth_project(np.zeros((0, 3), F), np.ones((0, 4), F), 1.0).shape == (0, 64, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# depth
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 2, 4, 63, 64, 70, 4096])
def test_depth_host_equals_the_restated_rule(samples):
    """The sw == 0 branch (a texel no sample reached) is asserted at 1, 2 and 4 samples.  It was planned for 63 samples too, but
    the rule cannot take it there: a texel stays open only if every sample has cos < 2^(-149/32) = 0.04 to its direction (cos^32
    then underflows to 0), which a uniform direction does with probability 0.52, so 63 samples leave a texel open with probability
    0.52^63 = 1e-18.  Measured with the host twin over 2,000 seeds: probes with an open texel 2,000 at 1 and 2 samples, 1,709 at
    4, 493 at 8, 27 at 12, 2 at 16, none at 24, 32, 63 and 64.  At 63 the count is printed."""
    n, max_d = 2, 1.75
    rng = np.random.default_rng(samples)
    pos = rng.uniform(-1, 1, (n, 3)).astype(F)
    seeds = [5, 0xFFFFFFF6]
    dist = rng.uniform(0.05, max_d, (n, samples)).astype(F)
    dist[rng.uniform(0, 1, (n, samples)) < 0.3] = F(max_d)           # misses
    got = plugin.probe_depth_project(pos, dist, max_d, first_sample=0xFFFFFFFE, seeds=seeds)
    d = plugin.probe_directions(pos, samples, first_sample=0xFFFFFFFE, seeds=seeds)[:, 3:6].reshape(n, samples, 3)
    want, open_ = volume_ref.depth_project(d, dist, max_d)
    assert got.shape == (n, 64, 2)
    assert (_bits(got) == _bits(want)).all(), np.argwhere(_bits(got) != _bits(want))[:5]
    print(f"[volume] {samples} samples: {int(open_.sum())} of {open_.size} texels took the sw == 0 branch")
    if samples in (1, 2, 4):
        assert open_.any()
        assert (got[open_][:, 0] == F(max_d)).all() and (got[open_][:, 1] == F(max_d) * F(max_d)).all()
    assert (~open_).any() and (got[~open_][:, 0] < F(max_d)).any()


@pytest.mark.parametrize("samples", [1, 63, 64, 70, 4096])
def test_constant_distance_gives_its_own_moments(samples):
    D, max_d = 0.7, 2.0
    pos = np.zeros((1, 3), F)
    got = plugin.probe_depth_project(pos, np.full((1, samples), D, F), max_d, seeds=[77])[0].astype(np.float64)
    d = plugin.probe_directions(pos, samples, seeds=[77])[:, 3:6].reshape(1, samples, 3)
    _, open_ = volume_ref.depth_project(d, np.full((1, samples), D, F), max_d)
    sampled = ~open_[0]
    assert sampled.any()
    Df = float(F(D))
    # two sequential sums of non-negative terms and one division
    bound = (2 * samples + 2) * 2.0 ** -24
    e1 = np.abs(got[sampled, 0] - Df).max() / Df
    e2 = np.abs(got[sampled, 1] - Df * Df).max() / (Df * Df)
    print(f"[volume] constant distance, {samples} samples, {int(sampled.sum())} sampled texels: mean off by {e1:.2e}, mean2 by {e2:.2e} (bound {bound:.2e})")
    assert e1 <= bound and e2 <= bound


def test_texel_directions_round_trip():
    d = volume_ref.texel_directions()
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 4e-7
    assert [volume_ref.texel_of(d[l]) for l in range(64)] == list(range(64))
    # ... and by the host twin: one probe at the origin, queried from the point 0.5 along every d_l.  A record whose texel l ends
    # before the point (zero variance, nearer) takes the probe's support away from the query along d_l alone
    g = _grid((0, 0, 0), (1, 1, 1), (1, 1, 1), flags=abi.PT_GRID_VISIBILITY)
    sh = np.ones((1, 9, 3), F)
    N = np.tile(np.array([(0.0, 1.0, 0.0)], F), (64, 1))
    for l in range(64):
        depth = np.full((1, 64, 2), 10.0, F)
        depth[..., 1] = 100.0
        depth[0, l] = (0.25, 0.0625)
        support = plugin.probe_grid_irradiance(g, sh, depth, d * F(0.5), N)[:, 3]
        assert support[l] == 0 and (np.delete(support, l) == 1).all(), (l, support)


# ---------------------------------------------------------------------------------------------------------------------------
# lookup
# ---------------------------------------------------------------------------------------------------------------------------
_ORIGIN, _SPACING = (-0.5, 0.25, -0.75), (0.5, 0.75, 0.625)


def _queries(counts, rng):
    hi = [_ORIGIN[a] + _SPACING[a] * (counts[a] - 1) for a in range(3)]
    inside = np.stack([rng.uniform(_ORIGIN[a], max(hi[a], _ORIGIN[a] + 1e-3), 12) for a in range(3)], axis=1)
    outside = []
    for a in range(3):
        for side in (-1, 1):
            p = [0.5 * (_ORIGIN[b] + hi[b]) + 0.1 for b in range(3)]
            p[a] = _ORIGIN[a] - 0.7 if side < 0 else hi[a] + 0.7
            outside.append(p)
    on_probe = [_ORIGIN[0], _ORIGIN[1], _ORIGIN[2]]
    last_plane = [hi[0], 0.5 * (_ORIGIN[1] + hi[1]) + 0.05, hi[2]]
    nan = [math.nan, 0.5, 0.5]
    corner = [hi[0] + 3.0, hi[1] + 3.0, _ORIGIN[2] - 3.0]
    P = np.array(list(inside) + outside + [on_probe, last_plane, nan, corner], F)
    N = _unit(rng.normal(0, 1, P.shape))
    return P, N


@pytest.mark.parametrize("counts", [(3, 2, 2), (1, 1, 1), (2, 1, 3)])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_lookup_host_equals_the_restated_rule(counts, flags):
    rng = np.random.default_rng(100 + sum(counts))
    n = counts[0] * counts[1] * counts[2]
    sh = rng.normal(0.3, 1, (n, 9, 3)).astype(F)
    mean = rng.uniform(0.1, 1.2, (n, 64)).astype(F)
    depth = np.stack([mean, mean * mean + rng.uniform(0, 0.05, (n, 64)).astype(F)], axis=2).astype(F)
    P, N = _queries(counts, rng)
    # the point on a probe takes the r == 0 path only without a bias: half of the cases have none
    bias = 0.0 if flags in (0, 3) else 0.03
    g = _grid(_ORIGIN, _SPACING, counts, flags, bias)
    got = plugin.probe_grid_irradiance(g, sh, depth if flags & 2 else None, P, N)
    assert got.shape == (len(P), 4)
    for k in range(len(P)):
        rgb, sw = volume_ref.lookup(_ORIGIN, _SPACING, counts, flags, bias, sh, depth, P[k], N[k])
        assert (_bits(got[k, :3]) == _bits(rgb)).all() and _bits(got[k, 3:4])[0] == _bits(sw), (k, got[k], rgb, sw)
    assert np.isfinite(got).all() and (got[:, 3] > 0).all()
    if flags == 0:
        assert np.abs(got[:, 3] - 1.0).max() <= 4 * EPS
    if flags == 3:
        assert (got[:, 3] < 0.5).any(), "no weight was cut: the flagged terms are not exercised"


def test_equal_probes_give_that_probes_irradiance():
    rng = np.random.default_rng(5)
    counts = (3, 2, 2)
    one = rng.uniform(0.2, 1.0, (9, 3)).astype(F)
    one[1:] *= F(0.2)                                    # band 0 dominates: E stays well away from 0
    sh = np.tile(one[None], (12, 1, 1))
    P, N = _queries(counts, rng)
    got = plugin.probe_grid_irradiance(_grid(_ORIGIN, _SPACING, counts), sh, None, P, N)
    want = plugin.probe_irradiance(one[None], N, np.zeros(len(P), np.uint32))[:, :3].astype(np.float64)
    assert (want > 0.1).all()
    rel = np.abs(got[:, :3] - want) / want
    print(f"[volume] equal probes: largest relative difference {rel.max():.2e}, |m2 - 1| {np.abs(got[:, 3] - 1.0).max():.2e}")
    assert rel.max() <= 4 * EPS and np.abs(got[:, 3].astype(np.float64) - 1.0).max() <= 4 * EPS


def test_trilinear_weights_reproduce_a_linear_field():
    counts = (3, 2, 2)
    g = _grid(_ORIGIN, _SPACING, counts)
    Q = plugin.probe_grid_positions(g).astype(np.float64)
    assert (_bits(plugin.probe_grid_positions(g)) == _bits(volume_ref.grid_positions(_ORIGIN, _SPACING, counts))).all()
    alpha, beta = 2.0, np.array([0.3, -0.2, 0.25])
    sh = np.zeros((12, 9, 3), F)
    sh[:, 0, :] = (alpha + Q @ beta)[:, None]
    rng = np.random.default_rng(9)
    hi = Q.max(axis=0)
    P = np.stack([rng.uniform(_ORIGIN[a], hi[a], 64) for a in range(3)], axis=1).astype(F)
    N = _unit(rng.normal(0, 1, P.shape))
    got = plugin.probe_grid_irradiance(g, sh, None, P, N)[:, 0].astype(np.float64)
    scale = float(F(3.14159265)) * float(F(0.28209479))                 # E of band 0 alone: A_0 * sh * Y_0
    want = (alpha + P.astype(np.float64) @ beta) * scale
    rel = np.abs(got - want) / want
    print(f"[volume] linear field: largest relative error {rel.max():.2e}")
    assert (want > 1.0).all() and rel.max() <= 1e-6


def test_zero_variance_cuts_a_probe_exactly():
    g_on = _grid((0, 0, 0), (1, 1, 1), (2, 1, 1), flags=abi.PT_GRID_VISIBILITY)
    g_off = _grid((0, 0, 0), (1, 1, 1), (2, 1, 1))
    rng = np.random.default_rng(21)
    sh = rng.uniform(0.2, 1.0, (2, 9, 3)).astype(F)
    sh[:, 1:] *= F(0.2)
    depth = np.empty((2, 64, 2), F)
    depth[0, :, 0], depth[0, :, 1] = 0.3, 0.09                          # probe 0 sees a wall at 0.3 everywhere: variance 0
    depth[1, :, 0], depth[1, :, 1] = 5.0, 25.0
    P = np.array([(0.8, 0.0, 0.0)], F)                                  # 0.8 from probe 0, behind its wall
    N = _unit([(0.3, 0.9, 0.2)])
    own = plugin.probe_irradiance(sh, N, [1])[0, :3].astype(np.float64)
    on = plugin.probe_grid_irradiance(g_on, sh, depth, P, N)[0]
    off = plugin.probe_grid_irradiance(g_off, sh, depth, P, N)[0]
    rel = np.abs(on[:3] - own) / own
    print(f"[volume] zero variance: relative difference to probe 1's own E {rel.max():.2e}; flag off differs by {(np.abs(off[:3] - own) / own).max():.2e}")
    assert rel.max() <= 4 * EPS
    assert _bits(on[3:4])[0] == _bits(np.array([0.8], F) - F(0.0))[0]   # sumW is probe 1's trilinear weight alone: w0 = 0 exactly
    assert (np.abs(off[:3] - own) / own).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# the rest
# ---------------------------------------------------------------------------------------------------------------------------
def test_volume_sanitize_target_runs_clean():
    """the host twins under AddressSanitizer + UBSan in a stand-alone program (csrc/volume_sanitize_main.cpp)"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", CSRC, "volume-sanitize", "VOLUME_SANITIZE_OUT=" + os.path.join(d, "volume_sanitize")],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "volume ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


KERNELS = ["pt_probe_depth_rays", "pt_probe_depth_resolve", "pt_probe_grid_irradiance"]
SHADE_VGPR_BUDGET = 128             # what tests/test_kernel_resources.py holds pt_wf_shade<false, PTRayMap> to


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_volume_kernels_fit_the_shade_kernels_budget():
    res = resources("pt_volume.hip")
    assert len(res) == len(KERNELS), sorted(res)
    for name in KERNELS:
        hits = [r for k, r in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1, (name, sorted(res))
        r = hits[0]
        print(f"[resources] {name}: {r}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgprs"] <= SHADE_VGPR_BUDGET, (name, r)
    resolve = [r for k, r in res.items() if "pt_probe_depth_resolve" in k][0]
    assert resolve["lds"] == 4 * 1024, resolve                          # 1 KB per wave, four probes per workgroup
