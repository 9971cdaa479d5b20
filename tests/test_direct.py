"""Direct light at first hits on the host (include/ptmi_plugin.h Part 24): the host twins (csrc/direct_host.cpp)
equal the numpy restatement (tests/direct_ref.py) bit for bit on the hand-made cases of tests/direct_cases.py; the draws do not
depend on the lights' emission; the sum's order; refusals; struct sizes; kernel resources; the sanitizer program; and the twins
against a float64 evaluation of the same formula, within four times the measured deviation."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin

from kernel_resources import resources
import direct_cases as cases
import direct_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
F = np.float32
CONTEXT_SYMBOLS = ["PTDirectPairCount", "PTDirectRays", "PTDirectAccumulate", "PTDirectLight", "PTShadeMixed", "PTShadeMixedFrame"]
HOST_SYMBOLS = ["PTDirectPairCountHost", "PTDirectRaysHost", "PTDirectAccumulateHost"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def entries():
    return cases.entries()


@pytest.fixture(scope="module")
def sets():
    return cases.light_sets()


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_direct_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in CONTEXT_SYMBOLS + HOST_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 24: direct light at first hits" in header


def test_direct_struct_matches_c_header():
    fields = ["structSize", "strata", "seed", "flags", "minAlpha", "reserved"]
    lines = ['printf("%zu %u %u\\n", sizeof(PTDirectParams), PT_DIRECT_CENTERED, PT_DIRECT_MAX_STRATA);']
    lines += [f'printf("{f} %zu\\n", offsetof(PTDirectParams, {f}));' for f in fields]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = subprocess.check_output([exe]).decode().splitlines()
    assert [int(x) for x in got[0].split()] == [C.sizeof(abi.PTDirectParams), abi.PT_DIRECT_CENTERED, abi.PT_DIRECT_MAX_STRATA] and C.sizeof(abi.PTDirectParams) == 32
    offs = dict(l.split(" ") for l in got[1:])
    for f in fields:
        assert int(offs[f]) == getattr(abi.PTDirectParams, f).offset, f


# ---------------------------------------------------------------------------------------------------------------------------
# the twins against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def test_pair_count(sets):
    for name, lights in sets.items():
        for strata in (1, 2, 3, 4):
            assert plugin.direct_pair_count(lights, strata) == ref.pair_count(lights, strata), (name, strata)
    assert plugin.direct_pair_count(sets["all"], 3) == 9 + 0 + 1 + 1
    assert plugin.direct_pair_count(sets["directional"], 4) == 0 and plugin.direct_pair_count(sets["none"], 1) == 0


@pytest.mark.parametrize("name", ["none", "point", "spot", "rect", "directional", "all", "rect_back", "short_range", "dark", "two_rects"])
@pytest.mark.parametrize("strata", [1, 2, 3, 4])
@pytest.mark.parametrize("centered", [True, False])
def test_rays_twin_equals_restatement(entries, sets, name, strata, centered):
    rays, terms, recv = entries
    lights = sets[name]
    min_alpha = 0.2 if strata == 2 else 0.0
    got_rays, got_c = plugin.direct_rays(lights, rays, terms, recv, strata, seed=1234 + strata, centered=centered, min_alpha=min_alpha)
    want_rays, want_c = ref.rays(lights, rays, terms, recv, strata, 1234 + strata, abi.PT_DIRECT_CENTERED if centered else 0, min_alpha)
    assert got_rays.shape == want_rays.shape and got_c.shape == want_c.shape
    assert np.array_equal(_bits(got_rays), _bits(want_rays))
    assert np.array_equal(_bits(got_c), _bits(want_c))
    assert np.isfinite(got_c).all() and np.isfinite(got_rays).all()                  # the NaN position emits none


def test_rays_special_entries(entries, sets):
    """what the cases were made for: the miss, nl <= 0, beyond the range, the rectangle's back, the spot's cones, a zero emission, a
    NaN position"""
    rays, terms, recv = entries
    n = terms.shape[0]
    counts = lambda name, **kw: (plugin.direct_rays(sets[name], rays, terms, recv, **kw)[0][:, 6] > 0).reshape(n, -1)
    point = counts("point")[:, 0]
    assert point.sum() > n // 2
    for k in (cases.MISS, cases.BACK, cases.NAN_P):
        assert not point[k], k
    assert not counts("short_range")[cases.FAR, 0] and counts("short_range")[:, 0].any()
    assert not counts("rect_back", strata=3).any()
    assert not counts("directional").size
    dark = counts("dark", strata=2)
    assert not dark[:, 0].any() and dark[:, 1:].any()
    # the spot: cos(theta) against cos(outer) = 0.7 and cos(inner) = 0.9, from the restated geometry
    spot = sets["spot"][0]
    axis = spot[8:11] / np.linalg.norm(spot[8:11])
    to = recv[:, 0:3] - spot[0:3]
    cos_theta = (to / np.linalg.norm(to, axis=1, keepdims=True)) @ axis
    valid = point & np.isfinite(cos_theta)
    c = plugin.direct_rays(sets["spot"], rays, terms, recv)[1]
    outside, between, inside = valid & (cos_theta < 0.69), valid & (cos_theta > 0.71) & (cos_theta < 0.89), valid & (cos_theta > 0.91)
    assert outside.sum() > 5 and between.sum() > 5 and inside.sum() > 3
    assert not c[outside].any() and (c[between, 0:3] > 0).all() and (c[inside, 0:3] > 0).all()
    # min_alpha widens a glossy lobe: the contribution of the rho = 0.03 entry changes, a rough entry's does not
    a = plugin.direct_rays(sets["point"], rays, terms, recv, min_alpha=0.0)[1]
    b = plugin.direct_rays(sets["point"], rays, terms, recv, min_alpha=0.2)[1]
    rough = np.flatnonzero(point & (terms[:, 3] ** 2 > 0.25))
    assert point[cases.GLOSSY] and not np.array_equal(_bits(a[cases.GLOSSY]), _bits(b[cases.GLOSSY]))
    assert rough.size > 10 and np.array_equal(_bits(a[rough]), _bits(b[rough]))


def test_draws_do_not_depend_on_emission(entries, sets):
    """the jitter of light l is the same whether or not an earlier light's pairs count"""
    rays, terms, recv = entries
    lights = sets["two_rects"].copy()
    lit = plugin.direct_rays(lights, rays, terms, recv, strata=2, seed=99)[0].reshape(terms.shape[0], 8, 8)
    lights[0, 4:7] = 0
    dark = plugin.direct_rays(lights, rays, terms, recv, strata=2, seed=99)[0].reshape(terms.shape[0], 8, 8)
    assert (lit[:, 0:4, 6] > 0).any() and not (dark[:, 0:4, 6] > 0).any()
    assert (dark[:, 4:8, 6] > 0).any() and np.array_equal(_bits(lit[:, 4:8]), _bits(dark[:, 4:8]))
    other = plugin.direct_rays(lights, rays, terms, recv, strata=2, seed=100)[0].reshape(terms.shape[0], 8, 8)
    assert not np.array_equal(_bits(other[:, 4:8]), _bits(dark[:, 4:8]))


def test_accumulate_order_and_occlusion():
    """three pairs whose float32 sum depends on the order: (1 + 2^24) + 1 = 2^24, 2^24 + (1 + 1) = 2^24 + 2; an occluded pair leaves
    the bits"""
    terms = np.zeros((3, 12), F)
    terms[0:2, 7] = 0.5                                                              # entry 2 is a miss
    contrib = np.zeros((9, 4), F)
    contrib[0:3, 0] = (1.0, 16777216.0, 1.0)
    contrib[3:6, 1] = (0.25, 0.5, 0.125)
    contrib[6:9, 2] = 7.0
    hits = np.zeros((9, 4), F)
    hits[:, 3:4].view(np.uint32)[:] = 0xFFFFFFFF
    hits[4, 3:4].view(np.uint32)[:] = 17                                             # the middle pair of entry 1 is occluded
    got = plugin.direct_accumulate(terms, contrib, hits, 3)
    assert np.array_equal(_bits(got), _bits(ref.accumulate(terms, contrib, hits, 3)))
    assert got[0, 0] == (F(1.0) + F(16777216.0)) + F(1.0) == F(16777216.0) and got[0, 0] != F(16777216.0) + (F(1.0) + F(1.0))
    assert got[1, 1] == F(0.375) and got[1, 3] == 1 and not got[2].any()
    # a pair that does not count (zero contribution, tmax 0: Part 3 answers it with a miss) adds nothing, not even to -0 or NaN bits
    assert plugin.direct_accumulate(terms, contrib, hits, 3)[0, 1] == 0 and np.signbit(got[0, 1]) == 0
    assert plugin.direct_accumulate(terms[:0], contrib[:0], hits[:0], 3).shape == (0, 4)
    assert np.array_equal(plugin.direct_accumulate(terms, contrib[:0], hits[:0], 0), np.array([[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0]], F))


def test_accumulate_twin_equals_restatement_on_the_cases(entries, sets):
    rays, terms, recv = entries
    rng = np.random.default_rng(3)
    for strata in (1, 3):
        pair_rays, c = plugin.direct_rays(sets["all"], rays, terms, recv, strata, seed=5)
        pairs = plugin.direct_pair_count(sets["all"], strata)
        hits = np.zeros((pair_rays.shape[0], 4), F)
        hits[:, 0] = pair_rays[:, 6]
        hits[:, 3:4].view(np.uint32)[:, 0] = np.where(rng.uniform(size=hits.shape[0]) < 0.3, 5, 0xFFFFFFFF)
        got = plugin.direct_accumulate(terms, c, hits, pairs)
        assert np.array_equal(_bits(got), _bits(ref.accumulate(terms, c, hits, pairs)))
        assert (got[:, 3] == (terms[:, 7] > 0)).all() and got[:, 0:3].max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# the formula in float64
# ---------------------------------------------------------------------------------------------------------------------------
def test_twins_against_float64(entries, sets):
    """The largest relative deviation of the twins' contributions from the float64 evaluation of the same formula, over every pair
    that counts on both sides, relative to the pair's largest channel.  Measured over these cases: cases.F64_MEASURED (written into
    DESIGN.md 5.29); asserted: four times that, the margin for the cases' spread."""
    rays, terms, recv = entries
    worst, compared = 0.0, 0
    for name in ("point", "spot", "rect", "all", "short_range", "two_rects"):
        for strata, centered, min_alpha in ((1, True, 0.0), (2, False, 0.2), (3, False, 0.0), (4, True, 0.0)):
            flags = abi.PT_DIRECT_CENTERED if centered else 0
            c32 = plugin.direct_rays(sets[name], rays, terms, recv, strata, seed=7, centered=centered, min_alpha=min_alpha)[1][:, 0:3].astype(np.float64)
            ok64, c64 = ref.contributions_f64(sets[name], rays, terms, recv, strata, 7, flags, min_alpha)
            both = ok64 & (c32 > 0).any(axis=1)
            scale = np.abs(c64[both]).max(axis=1)
            dev = (np.abs(c32[both] - c64[both]).max(axis=1) / scale).max()
            worst, compared = max(worst, float(dev)), compared + int(both.sum())
            # a pair counts on one side only at a threshold (nl, a cone, the range): such pairs carry next to nothing
            one = ok64 != (c32 > 0).any(axis=1)
            assert np.abs(c64[one]).max(initial=0.0) < 1e-4 and np.abs(c32[one]).max(initial=0.0) < 1e-4
    print(f"[direct] twins against float64: largest relative deviation {worst:.3e} over {compared} pairs (cap {cases.F64_CAP:.3e})")
    assert compared > 5000
    assert worst <= cases.F64_CAP


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _inputs(buf):
    a = buf.ctypes.data
    s = abi.PTShadeInputs()
    s.grid.spacing[:] = (1.0, 1.0, 1.0)
    s.grid.counts[:] = (2, 2, 2)
    s.dSH, s.dMaps, s.dProbes, s.dDFG = a, a, a, a
    s.probeCount, s.res, s.levels, s.dfgRes = 1, 8, 2, 16
    return s


def _bad_params():
    def make(**over):
        p = abi.direct_params()
        for k, v in over.items():
            setattr(p, k, v)
        return p
    reserved = abi.direct_params()
    reserved.reserved[1] = 1
    return [(make(strata=0), b"strata"), (make(strata=5), b"strata"), (make(flags=2), b"flag"), (reserved, b"reserved"), (make(minAlpha=-0.1), b"minAlpha"),
            (make(minAlpha=float("nan")), b"minAlpha"), (make(minAlpha=float("inf")), b"minAlpha"), (make(structSize=0), b"structSize"),
            (make(structSize=16), b"structSize")]


def test_direct_refusals():
    lib = plugin.load_library()
    buf = np.zeros(4096, np.uint8)
    a = buf.ctypes.data
    a += (-a) % 16
    b = a + 1024
    ab = buf[a - buf.ctypes.data:]
    fp = abi.PTFrameParams()
    fp.structSize = C.sizeof(fp)
    fp.OutputWidth = fp.OutputHeight = 8
    ok, inputs = abi.direct_params(), _inputs(ab)
    n = C.c_uint32()
    calls = {"PTDirectPairCount": lambda c, p=ok: lib.PTDirectPairCount(c, p.strata, C.byref(n)),
             "PTDirectRays": lambda c, p=ok: lib.PTDirectRays(c, C.byref(p), a, a, a, 1, b, b),
             "PTDirectLight": lambda c, p=ok: lib.PTDirectLight(c, C.byref(p), a, a, a, 1, b),
             "PTShadeMixed": lambda c, p=ok: lib.PTShadeMixed(c, C.byref(inputs), C.byref(p), a, a, a, 1, b),
             "PTShadeMixedFrame": lambda c, p=ok: lib.PTShadeMixedFrame(c, C.byref(fp), C.byref(inputs), C.byref(p), b, None)}
    for name, call in calls.items():
        assert call(None) == abi.PT_ERR_INVALID_ARG, name
        assert b"ctx" in lib.PTGetLastError() and name.encode() in lib.PTGetLastError()
    assert lib.PTDirectAccumulate(None, a, a, a, 1, 1, b) == abi.PT_ERR_INVALID_ARG and b"ctx" in lib.PTGetLastError()
    ctx = C.c_void_p(1)         # never dereferenced: every call below is refused on its arguments alone
    for p, word in _bad_params():
        for name, call in calls.items():
            if name == "PTDirectPairCount" and word != b"strata":
                continue
            assert call(ctx, p) == abi.PT_ERR_INVALID_ARG and word in lib.PTGetLastError(), (name, word, lib.PTGetLastError())
        assert lib.PTDirectRaysHost(C.byref(p), None, 0, a, a, a, 1, b, b) == 0 and word in lib.PTGetBVHBuildError(), word
    assert lib.PTDirectPairCount(ctx, 1, None) == abi.PT_ERR_INVALID_ARG
    okp = C.byref(ok)
    assert lib.PTDirectRays(ctx, None, a, a, a, 1, b, b) == abi.PT_ERR_INVALID_ARG and b"params" in lib.PTGetLastError()
    assert lib.PTDirectLight(ctx, None, a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"params" in lib.PTGetLastError()
    assert lib.PTShadeMixed(ctx, C.byref(inputs), None, a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"params" in lib.PTGetLastError()
    assert lib.PTShadeMixed(ctx, None, okp, a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"inputs" in lib.PTGetLastError()
    assert lib.PTShadeMixedFrame(ctx, C.byref(fp), C.byref(inputs), None, b, None) == abi.PT_ERR_INVALID_ARG and b"params" in lib.PTGetLastError()
    assert lib.PTShadeMixedFrame(ctx, None, C.byref(inputs), okp, b, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeMixedFrame(ctx, C.byref(fp), C.byref(inputs), okp, None, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeMixedFrame(ctx, C.byref(fp), C.byref(inputs), okp, b, a + 8) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    for k in range(3):
        args = [a, a, a]
        args[k] = None
        assert lib.PTDirectRays(ctx, okp, *args, 1, b, b) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError(), k
        assert lib.PTDirectLight(ctx, okp, *args, 1, b) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError(), k
        assert lib.PTShadeMixed(ctx, C.byref(inputs), okp, *args, 1, b) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError(), k
        args[k] = a + 8
        assert lib.PTDirectRays(ctx, okp, *args, 1, b, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError(), k
        assert lib.PTDirectLight(ctx, okp, *args, 1, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError(), k
        assert lib.PTShadeMixed(ctx, C.byref(inputs), okp, *args, 1, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError(), k
    assert lib.PTDirectLight(ctx, okp, a, a, a, 1, None) == abi.PT_ERR_INVALID_ARG and lib.PTDirectLight(ctx, okp, a, a, a, 1, b + 4) == abi.PT_ERR_INVALID_ARG
    assert lib.PTDirectRays(ctx, okp, a, a, a, 1, b + 8, b) == abi.PT_ERR_INVALID_ARG and lib.PTDirectRays(ctx, okp, a, a, a, 1, b, b + 8) == abi.PT_ERR_INVALID_ARG
    for args in ((None, a, a, b), (a, None, a, b), (a, a, None, b), (a, a, a, None)):
        assert lib.PTDirectAccumulate(ctx, args[0], args[1], args[2], 1, 2, args[3]) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError(), args
    assert lib.PTDirectAccumulate(ctx, a, a + 8, a, 1, 2, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    assert lib.PTDirectAccumulate(ctx, a, a, a, 1 << 31, 2, b) == abi.PT_ERR_INVALID_ARG and b"2^31" in lib.PTGetLastError()
    assert lib.PTDirectAccumulate(ctx, a, a, a, 0, 2, b) == abi.PT_OK                   # count 0 launches nothing
    # the host twins: 0 and a message; count == 0 is fine
    assert lib.PTDirectPairCountHost(None, 2, 1, C.byref(n)) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTDirectPairCountHost(a, 1, 0, C.byref(n)) == 0 and b"strata" in lib.PTGetBVHBuildError()
    assert lib.PTDirectPairCountHost(a, 1, 1, None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    point = cases.light_sets()["point"]
    assert lib.PTDirectRaysHost(okp, point.ctypes.data, 1, None, a, a, 1, b, b) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTDirectRaysHost(okp, point.ctypes.data, 1, a, a, a, 1, None, b) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTDirectAccumulateHost(a, None, a, 1, 2, b) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTDirectRaysHost(okp, None, 0, None, None, None, 0, None, None) == 1
    assert lib.PTDirectAccumulateHost(None, None, None, 0, 3, None) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' resources and the sanitizer program
# ---------------------------------------------------------------------------------------------------------------------------
def test_direct_kernel_resources():
    """no scratch and no spill, of vector or of scalar registers, in any of the four kernels; the fused kernels' waves per SIMD as
    DESIGN.md 5.29 records them (pt_query's any-hit kernels: 8 flat, 4 with a TLAS)"""
    rep = resources("pt_direct.hip")
    sgpr = {k: r["sgpr_spill"] for k, r in rep.items()}
    names = {"rays": [k for k in rep if "pt_direct_rays" in k], "accumulate": [k for k in rep if "pt_direct_accumulate" in k],
             "light": ["pt_direct_light"], "tlas": ["pt_direct_light_tlas"]}
    for what, ks in names.items():
        assert len(ks) == 1 and ks[0] in rep and ks[0] in sgpr, (what, sorted(rep), sorted(sgpr))
        r = rep[ks[0]]
        print(f"[direct] {ks[0][:40]}: {r}, scalar spill {sgpr[ks[0]]}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and sgpr[ks[0]] == 0, (what, r, sgpr[ks[0]])
    assert rep[names["rays"][0]]["occupancy"] == 8 and rep[names["accumulate"][0]]["occupancy"] == 8
    assert rep["pt_direct_light"]["lds"] == 8 * 64 * 8 + 4 and rep["pt_direct_light"]["occupancy"] >= 6
    assert rep["pt_direct_light_tlas"]["lds"] == 8 * 64 * 8 + 32 * 64 * 4 + 4 and rep["pt_direct_light_tlas"]["occupancy"] >= 4
    query = resources("pt_query.hip")
    assert query["pt_query_anyhit"]["occupancy"] == 8 and query["pt_query_tlas_anyhit"]["occupancy"] == 4


def test_direct_sanitize_program():
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", CSRC, "direct-sanitize", f"DIRECT_SANITIZE_OUT={os.path.join(d, 'direct_sanitize')}"], capture_output=True, text=True,
                             timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "direct ok" in out.stdout
