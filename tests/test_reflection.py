"""Reflection probes (include/ptmi_plugin.h Part 20) without a GPU: exports, struct layout, argument checks, the host twins against
the numpy restatement of the rule (tests/reflection_ref.py) bit for bit, the properties the rule promises (directions inside their
texels, a constant map, a single bright texel, the cosine lobe's closed form, bilinear convergence across the octahedral wrap, box
projection), the sanitizer build of the host twins and the compile-time resources of the four kernels.
tests/test_gpu_reflection.py holds the kernels to the rule."""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from kernel_resources import resources
import reflection_cases as cases
import reflection_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
F = np.float32
CONTEXT_SYMBOLS = ["PTReflectionRays", "PTReflectionCapture", "PTReflectionCaptureHost", "PTReflectionPrefilter", "PTReflectionLookup"]
HOST_SYMBOLS = ["PTReflectionDirectionsHost", "PTReflectionFoldHost", "PTReflectionPrefilterHost", "PTReflectionLookupHost"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_reflection_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in CONTEXT_SYMBOLS + HOST_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 20: reflection probes" in header


def test_reflection_structs_match_c_header():
    fields = {"PTReflectionTexel": ["rgb", "aux"], "PTReflectionQuery": ["position", "roughness", "direction", "probe"],
              "PTReflectionBox": ["bmin", "pad0", "bmax", "pad1"]}
    lines = []
    for s, fs in fields.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTReflectionTexel"]) == C.sizeof(abi.PTReflectionTexel) == 16
    assert int(got["PTReflectionQuery"]) == C.sizeof(abi.PTReflectionQuery) == 32
    assert int(got["PTReflectionBox"]) == C.sizeof(abi.PTReflectionBox) == 32
    for s, fs in fields.items():
        for f in fs:
            assert int(got[f"{s}.{f}"]) == getattr(getattr(abi, s), f).offset, (s, f)
    assert [int(got[f"PTReflectionQuery.{f}"]) for f in fields["PTReflectionQuery"]] == [0, 12, 16, 28]


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2. directions and fold
# ---------------------------------------------------------------------------------------------------------------------------
_POS = np.array([(0.25, -1.5, 3.0), (-2.0, 0.5, 0.125)], F)
_SEEDS = np.array([5, 0xFFFFFFF6], np.uint32)


@pytest.mark.parametrize("res", [8, 16])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("first", [0, 0xFFFFFFF0])
def test_directions_host_equals_the_restated_rule(res, samples, first):
    got = plugin.reflection_directions(_POS, res, samples, first_sample=first, seeds=_SEEDS)
    want = ref.rays(_POS, _SEEDS, res, first, samples)
    assert got.shape == (2 * res * res * samples, 8)
    assert (_bits(got) == _bits(want)).all(), np.argwhere(_bits(got) != _bits(want))[:5]
    assert (got[:, 7].view(np.uint32) == 0).all()
    # every direction lies inside its texel (on its edge at most): its octahedral coordinates again, in float64
    d = got[:, 3:6].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 4e-7
    s = np.abs(d).sum(axis=1)
    a, b = d[:, 0] / s, d[:, 1] / s
    neg = d[:, 2] < 0
    sg = lambda x: np.where(x < 0, -1.0, 1.0)
    a, b = np.where(neg, (1 - np.abs(b)) * sg(a), a), np.where(neg, (1 - np.abs(a)) * sg(b), b)
    t = np.tile(np.repeat(np.arange(res * res), samples), 2)
    x, y = (a * 0.5 + 0.5) * res, (b * 0.5 + 0.5) * res
    tol = 1e-6 * res            # 1e-6 in the map's [-1, 1] coordinates
    assert ((x >= t % res - tol) & (x <= t % res + 1 + tol) & (y >= t // res - tol) & (y <= t // res + 1 + tol)).all()


def test_direction_samples_do_not_depend_on_the_split():
    whole = plugin.reflection_directions(_POS, 8, 8, first_sample=0, seeds=_SEEDS).reshape(2 * 64, 8, 8)
    part = plugin.reflection_directions(_POS, 8, 4, first_sample=4, seeds=_SEEDS).reshape(2 * 64, 4, 8)
    assert (_bits(whole[:, 4:8]) == _bits(part)).all()


@pytest.mark.parametrize("samples", [1, 3, 70])
def test_fold_host_equals_the_restated_rule(samples):
    rng = np.random.default_rng(samples)
    rad = rng.uniform(0.0, 5.0, (2 * 64 * samples, 4)).astype(F)
    rad[rng.uniform(0, 1, len(rad)) < 0.4, :3] = 0.0
    got = plugin.reflection_fold(rad, 2, 8)
    want = ref.fold(rad, samples).reshape(2, 64, 4)
    assert (_bits(got) == _bits(want)).all()
    assert (got[..., 3] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 3 ... 6. prefilter
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,levels", cases.PREFILTER_SHAPES)
def test_prefilter_host_equals_the_restated_rule(res, levels):
    base = cases.random_base(2, res, seed=res)
    got = plugin.reflection_prefilter(base, res, levels)
    want = ref.prefilter(base, res, levels)
    assert got.shape == (2, plugin.reflection_texel_count(res, levels), 4)
    assert (_bits(got[:, :res * res]) == _bits(base)).all()             # level 0, aux included
    assert (_bits(got) == _bits(want)).all(), np.argwhere(_bits(got) != _bits(want))[:5]
    assert np.isfinite(got).all() and (got[:, res * res:, 3] > 0).all()


@pytest.mark.parametrize("res,levels", cases.PREFILTER_SHAPES)
def test_prefilter_keeps_a_constant_map_exactly(res, levels):
    """acc repeats sw's sequence of sums scaled by 2^-2, so acc / sw is 0.25 whatever the weights were"""
    base = np.full((1, res * res, 4), 0.25, F)
    got = plugin.reflection_prefilter(base, res, levels)
    assert (got[..., :3] == F(0.25)).all()


def test_prefilter_spreads_a_bright_texel_more_with_every_level():
    res, levels = 32, 4
    base = np.zeros((1, res * res, 4), F)
    base[0, 9 * res + 20, :3] = 1000.0
    got = plugin.reflection_prefilter(base, res, levels)[0]
    peak = [float(got[plugin.reflection_texel_count(res, k):plugin.reflection_texel_count(res, k + 1), 0].max()) for k in range(levels)]
    print(f"[reflection] a single bright texel, per-level maximum: {peak}")
    assert all(peak[k + 1] < peak[k] for k in range(levels - 1)) and peak[-1] > 0


def _directions64(R):
    t = np.arange(R * R)
    a, b = ((t % R + 0.5) / R) * 2 - 1, ((t // R + 0.5) / R) * 2 - 1
    z = 1 - np.abs(a) - np.abs(b)
    sg = lambda x: np.where(x < 0, -1.0, 1.0)
    x, y = np.where(z < 0, (1 - np.abs(b)) * sg(a), a), np.where(z < 0, (1 - np.abs(a)) * sg(b), b)
    ln = np.sqrt(x * x + y * y + z * z)
    return np.stack([x, y, z], axis=1) / ln[:, None], ln


def test_jacobian_sums_to_the_sphere():
    _, ln = _directions64(64)
    total = float((1.0 / ln ** 3).sum() * (2.0 / 64) ** 2)
    print(f"[reflection] sum of J x texel area over a 64 x 64 map: {total:.7f} (4 pi = {4 * math.pi:.7f})")
    assert abs(total - 4 * math.pi) < 1e-3


def test_prefilter_last_level_is_the_cosine_lobe():
    """Level levels - 1 has rho = 1: t = 1 and the weight is c J, a cosine-weighted mean over the hemisphere around n.  For the base
    0.5 + 0.5 l_z that mean is 0.5 + n_z / 3.  Measured: float64 quadrature against the closed form 1.94e-04 (the map's discretisation;
    the cap keeps a wrong Jacobian out); twin against the float64 quadrature 1.69e-06 relative, inside the 1e-5 the project allows a
    closed form of this arithmetic depth (1,024 sequential fp32 terms)."""
    res, levels = 32, 4
    l, ln = _directions64(res)
    base64 = 0.5 + 0.5 * l[:, 2]
    base = np.zeros((1, res * res, 4), F)
    base[0, :, :3] = base64.astype(F)[:, None]
    got = plugin.reflection_prefilter(base, res, levels)[0]
    Rk = res >> (levels - 1)
    n, _ = _directions64(Rk)
    c = np.maximum(n @ l.T, 0.0)
    w = c / ln[None, :] ** 3
    # the quadrature of the same sum: the fp32 base values the twin was given, float64 arithmetic
    quad = (w * base[0, :, 0].astype(np.float64)[None, :]).sum(axis=1) / w.sum(axis=1)
    closed = 0.5 + n[:, 2] / 3.0
    e_quad = float(np.abs(quad - closed).max())
    last = got[plugin.reflection_texel_count(res, levels - 1):, 0].astype(np.float64)
    e_twin = float((np.abs(last - quad) / quad).max())
    print(f"[reflection] cosine lobe at {Rk} x {Rk}: float64 quadrature off the closed form by {e_quad:.3e}; twin off the quadrature by {e_twin:.3e} relative")
    assert e_quad < 1e-3
    assert e_twin < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------
# 7 ... 10. lookup
# ---------------------------------------------------------------------------------------------------------------------------
_PROBES = 3


@pytest.mark.parametrize("res,levels", [(8, 2), (16, 3), (32, 4)])
def test_lookup_host_equals_the_restated_rule(res, levels):
    maps = cases.random_maps(_PROBES, res, levels, seed=levels)
    q = cases.query_set(_PROBES)
    assert len(q) == 4096
    got = plugin.reflection_lookup(maps, res, levels, queries=q)
    want = ref.lookup(maps, res, levels, q)
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), np.argwhere(~same)[:5]
    assert (got[7] == 0).all() and (np.delete(got, 7, axis=0)[:, 3] == 1).all()
    assert np.isfinite(got).all()
    # with boxes: positions inside and outside, probes off-centre
    Q, boxes = cases.probe_boxes(_PROBES)
    got_b = plugin.reflection_lookup(maps, res, levels, queries=q, probe_positions=Q, boxes=boxes)
    want_b = ref.lookup(maps, res, levels, q, Q, boxes)
    assert (_bits(got_b) == _bits(want_b)).all(), np.argwhere(_bits(got_b) != _bits(want_b))[:5]
    moved = (_bits(got_b) != _bits(got)).any(axis=1)
    print(f"[reflection] {res}/{levels}: box projection changed {int(moved.sum())} of {len(q)} lookups")
    assert moved.sum() > len(q) // 2 and (~moved).sum() > len(q) // 10


def test_lookup_returns_a_constant_map_exactly():
    res, levels = 16, 3
    maps = np.full((_PROBES, plugin.reflection_texel_count(res, levels), 4), 0.6875, F)
    got = plugin.reflection_lookup(maps, res, levels, queries=cases.query_set(_PROBES))
    assert (np.delete(got, 7, axis=0)[:, :3] == F(0.6875)).all()


def _smooth(d):
    return 0.5 + 0.25 * d[:, 0] + 0.15 * d[:, 1] - 0.1 * d[:, 2]


def _smooth_error(res, levels, d):
    maps = np.zeros((1, plugin.reflection_texel_count(res, levels), 4), F)
    first = 0
    for k in range(levels):
        c, _ = _directions64(res >> k)
        maps[0, first:first + len(c), :3] = _smooth(c).astype(F)[:, None]
        first += len(c)
    got = plugin.reflection_lookup(maps, res, levels, directions=d, roughness=0.0, probes=0)[:, 0].astype(np.float64)
    return float(np.abs(got - _smooth(d.astype(np.float64))).max())


def test_lookup_converges_on_a_smooth_function():
    """measured in float64: 7.85e-3 at R = 32 and 1.58e-2 at R = 16; a wrap that mirrors without the flip reads 1.7e-2 and 3.5e-2"""
    d = cases.unit(np.random.default_rng(3).normal(0, 1, (200000, 3)))
    e32, e16 = _smooth_error(32, 4, d), _smooth_error(16, 3, d)
    print(f"[reflection] smooth function: largest error {e32:.3e} at R = 32, {e16:.3e} at R = 16")
    assert e32 < 0.01 and e32 < 0.6 * e16


def test_box_projection():
    res, levels, n = 16, 3, 2000
    rng = np.random.default_rng(8)
    maps = cases.random_maps(1, res, levels, seed=1)
    Q = np.array([(0.2, -0.15, 0.1)], F)
    box = plugin.reflection_box_rows([(-0.5, -0.5, -0.5)], [(0.5, 0.5, 0.5)])
    P = rng.uniform(-0.45, 0.45, (n, 3)).astype(F)
    D = cases.unit(rng.normal(0, 1, (n, 3)))
    rough = rng.uniform(0, 1, n).astype(F)
    # the corrected direction: the restated rule's against float64
    zeros = np.zeros(n, np.int64)
    got_d = ref.box_project(box[zeros, 0:3], box[zeros, 4:7], P, Q[zeros], D).astype(np.float64)
    P64, D64 = P.astype(np.float64), D.astype(np.float64)
    with np.errstate(divide="ignore"):
        t = np.where(D64 > 0, (0.5 - P64) / D64, np.where(D64 < 0, (-0.5 - P64) / D64, np.inf)).min(axis=1)
    v = P64 + D64 * t[:, None] - Q.astype(np.float64)
    want_d = v / np.linalg.norm(v, axis=1, keepdims=True)
    err = float(np.abs(got_d - want_d).max())
    print(f"[reflection] box projection: corrected direction off float64 by {err:.2e}")
    assert err < 1e-6
    assert np.abs(got_d - D64).max() > 0.1
    # ... and the twin reads exactly that direction: a lookup with the box equals a plain lookup of the corrected direction
    with_box = plugin.reflection_lookup(maps, res, levels, D, rough, 0, positions=P, probe_positions=Q, boxes=box)
    plain = plugin.reflection_lookup(maps, res, levels, got_d.astype(F), rough, 0)
    assert (_bits(with_box) == _bits(plain)).all()
    # a query outside the box keeps D's bits
    P_out = P.copy()
    P_out[:, 1] += 1.0
    outside = plugin.reflection_lookup(maps, res, levels, D, rough, 0, positions=P_out, probe_positions=Q, boxes=box)
    no_box = plugin.reflection_lookup(maps, res, levels, D, rough, 0, positions=P_out, probe_positions=Q)
    no_pos = plugin.reflection_lookup(maps, res, levels, D, rough, 0)
    assert (_bits(outside) == _bits(no_pos)).all()
    assert (_bits(no_box) == _bits(no_pos)).all()                      # dBoxes == NULL: the call without positions


# ---------------------------------------------------------------------------------------------------------------------------
# 11. argument checks
# ---------------------------------------------------------------------------------------------------------------------------
def test_reflection_argument_errors():
    """every refusal of Part 20 that needs no scene: the context's entry points check their arguments before they touch the GPU"""
    lib = plugin.load_library()
    buf = (C.c_float * 65536)()
    a = (C.addressof(buf) + 15) & ~15
    b = a + 128 * 1024
    p = abi.PTFrameParams()
    p.OutputWidth = p.OutputHeight = 8
    p.MaxRayBounces = 2
    pp = C.byref(p)
    calls = {"PTReflectionRays": lambda c: lib.PTReflectionRays(c, pp, a, 1, 8, 0, 1, b),
             "PTReflectionCapture": lambda c: lib.PTReflectionCapture(c, pp, a, 1, 8, 0, 1, b),
             "PTReflectionCaptureHost": lambda c: lib.PTReflectionCaptureHost(c, pp, a, 1, 8, 0, 1, b),
             "PTReflectionPrefilter": lambda c: lib.PTReflectionPrefilter(c, a, 1, 8, 2, b),
             "PTReflectionLookup": lambda c: lib.PTReflectionLookup(c, a, 1, 8, 2, None, None, b, 1, b + 64)}
    for name, call in calls.items():
        assert call(None) == abi.PT_ERR_INVALID_ARG, name
        assert b"ctx" in lib.PTGetLastError() and name.encode() in lib.PTGetLastError()
    ctx = C.c_void_p(1)         # never dereferenced: every call below is refused on its arguments alone
    for fn in (lib.PTReflectionRays, lib.PTReflectionCapture, lib.PTReflectionCaptureHost):
        for bad in (0, 65537):
            assert fn(ctx, pp, a, 1, 8, 0, bad, b) == abi.PT_ERR_UNSUPPORTED and b"samples" in lib.PTGetLastError(), bad
        for bad in (0, 4, 12, 512):
            assert fn(ctx, pp, a, 1, bad, 0, 1, b) == abi.PT_ERR_INVALID_ARG and b"res" in lib.PTGetLastError(), bad
        assert fn(ctx, None, a, 1, 8, 0, 1, b) == abi.PT_ERR_INVALID_ARG
        assert fn(ctx, pp, None, 1, 8, 0, 1, b) == abi.PT_ERR_INVALID_ARG and fn(ctx, pp, a, 1, 8, 0, 1, None) == abi.PT_ERR_INVALID_ARG
        q = p.copy()
        q.MaxRayBounces = 8192
        assert fn(ctx, C.byref(q), a, 1, 8, 0, 1, b) == abi.PT_ERR_UNSUPPORTED and b"MaxRayBounces" in lib.PTGetLastError()
    for fn in (lib.PTReflectionRays, lib.PTReflectionCapture):
        assert fn(ctx, pp, a + 8, 1, 8, 0, 1, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
        assert fn(ctx, pp, a, 1, 8, 0, 1, b + 4) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    bad_layouts = [(4, 2), (12, 2), (512, 2), (8, 1), (8, 3), (16, 4), (256, 8), (64, 0)]
    for res, levels in bad_layouts:
        assert lib.PTReflectionPrefilter(ctx, a, 1, res, levels, b) == abi.PT_ERR_INVALID_ARG, (res, levels)
        assert lib.PTReflectionLookup(ctx, a, 1, res, levels, None, None, b, 1, b + 64) == abi.PT_ERR_INVALID_ARG, (res, levels)
        assert lib.PTReflectionPrefilterHost(a, 1, res, levels, b) == 0 and lib.PTGetBVHBuildError() != b"", (res, levels)
        assert lib.PTReflectionLookupHost(a, 1, res, levels, None, None, b, 1, b + 64) == 0 and lib.PTGetBVHBuildError() != b"", (res, levels)
    assert lib.PTReflectionPrefilter(ctx, a, 1, 8, 2, a) == abi.PT_ERR_INVALID_ARG and b"alias" in lib.PTGetLastError()
    assert lib.PTReflectionPrefilter(ctx, a, 1, 8, 2, a + 512) == abi.PT_ERR_INVALID_ARG and b"alias" in lib.PTGetLastError()
    assert lib.PTReflectionPrefilter(ctx, None, 1, 8, 2, b) == abi.PT_ERR_INVALID_ARG and lib.PTReflectionPrefilter(ctx, a, 1, 8, 2, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTReflectionPrefilter(ctx, a + 4, 1, 8, 2, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    assert lib.PTReflectionLookup(ctx, a, 1, 8, 2, None, a, b, 1, b + 64) == abi.PT_ERR_INVALID_ARG and b"boxes without probes" in lib.PTGetLastError()
    for args in ((None, b, b + 64), (a, None, b + 64), (a, b, None)):
        assert lib.PTReflectionLookup(ctx, args[0], 1, 8, 2, None, None, args[1], 1, args[2]) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    for args in ((a + 8, None, None, b, b + 64), (a, a + 8, None, b, b + 64), (a, a, a + 8, b, b + 64), (a, None, None, b + 8, b + 64), (a, None, None, b, b + 72)):
        assert lib.PTReflectionLookup(ctx, args[0], 1, 8, 2, args[1], args[2], args[3], 1, args[4]) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    # the host twins: 0 and a message
    assert lib.PTReflectionPrefilterHost(a, 1, 8, 2, a) == 0 and b"alias" in lib.PTGetBVHBuildError()
    assert lib.PTReflectionPrefilterHost(None, 1, 8, 2, b) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTReflectionLookupHost(a, 1, 8, 2, None, a, b, 1, b + 64) == 0 and b"boxes without probes" in lib.PTGetBVHBuildError()
    assert lib.PTReflectionLookupHost(None, 1, 8, 2, None, None, b, 1, b + 64) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    for bad in (0, 65537):
        assert lib.PTReflectionDirectionsHost(a, 1, 8, 0, bad, b) == 0 and b"samples" in lib.PTGetBVHBuildError()
        assert lib.PTReflectionFoldHost(a, 1, 8, bad, b) == 0 and b"samples" in lib.PTGetBVHBuildError()
    for bad in (0, 4, 12, 512):
        assert lib.PTReflectionDirectionsHost(a, 1, bad, 0, 1, b) == 0 and b"res" in lib.PTGetBVHBuildError()
        assert lib.PTReflectionFoldHost(a, 1, bad, 1, b) == 0 and b"res" in lib.PTGetBVHBuildError()
    assert lib.PTReflectionDirectionsHost(None, 1, 8, 0, 1, b) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTReflectionFoldHost(a, 1, 8, 1, None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    # count == 0 is fine
    assert plugin.reflection_directions(np.zeros((0, 3), F), 8, 2).shape == (0, 8)
    assert plugin.reflection_prefilter(np.zeros((0, 64, 4), F), 8, 2).shape == (0, 80, 4)
    assert lib.PTReflectionLookupHost(None, 0, 8, 2, None, None, b, 1, b + 64) == 1        # no probes: every index is out of range


# ---------------------------------------------------------------------------------------------------------------------------
# 12, 13. kernel resources and the sanitizer build
# ---------------------------------------------------------------------------------------------------------------------------
KERNELS = ["pt_refl_rays", "pt_refl_fold", "pt_refl_prefilter", "pt_refl_lookup"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_reflection_kernel_resources():
    with ThreadPoolExecutor(3) as ex:
        fa = ex.submit(resources, "pt_wavefront.hip", "a")
        fb = ex.submit(resources, "pt_wavefront.hip", "b")
        fr = ex.submit(resources, "pt_reflection.hip")
        res_a, res_b, res = fa.result(), fb.result(), fr.result()
    assert len(res) == len(KERNELS), sorted(res)
    for name in KERNELS:
        hits = [r for k, r in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1, (name, sorted(res))
        print(f"[resources] {name}: {hits[0]}")
        assert hits[0]["scratch"] == 0 and hits[0]["vgpr_spill"] == 0, (name, hits[0])
    prefilter = [r for k, r in res.items() if "pt_refl_prefilter" in k][0]
    assert 0 < prefilter["lds"] <= 16 * 1024, prefilter
    # the capture composes the radiance query: pt_wavefront.hip's two compilations hold the kernels they held before
    golden = open(os.path.join(ROOT, "tests", "golden", "wavefront_kernel_names.txt")).read().split()
    for unit, r in (("a", res_a), ("b", res_b)):
        assert sorted(r) == sorted(n[2:] for n in golden if n.startswith(unit + ":")), unit


def test_reflection_sanitize_target_runs_clean():
    """the host twins under AddressSanitizer + UBSan in a stand-alone program (csrc/reflection_sanitize_main.cpp)"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", CSRC, "reflection-sanitize", "REFLECTION_SANITIZE_OUT=" + os.path.join(d, "reflection_sanitize")],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "reflection ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
