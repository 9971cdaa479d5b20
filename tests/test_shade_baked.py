"""Shading from the bakes on the host (include/ptmi_plugin.h Part 21): the host twins (csrc/shade_host.cpp) equal
the numpy restatement (tests/shade_ref.py) bit for bit; the DFG table lies within a measured bound of a float64 quadrature of the
same integral, and that bound tells a wrong rule from the right one; refusals; kernel resources; the sanitizer program."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin

from kernel_resources import resources
import shade_cases as cases
import shade_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
F = np.float32
CONTEXT_SYMBOLS = ["PTBakeDFG", "PTShadeSurfaces", "PTShadeCompose", "PTShadeBaked", "PTShadeBakedFrame"]
HOST_SYMBOLS = ["PTBakeDFGHost", "PTShadeTermsHost", "PTShadeComposeHost"]
# The res-16 table against a float64 quadrature of the same integral with 1,024 x 256 samples: the largest absolute difference is
# 0.02539 (entry i = 0, j = 5: N.V = 1 / 32, where 64 x 64 midpoints resolve the narrow lobe least).  The cap is twice that.
DFG_MEASURED = 0.02539
DFG_CAP = 2 * DFG_MEASURED


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dfg16():
    return plugin.bake_dfg(16)


@pytest.fixture(scope="module")
def quadrature16():
    return ref.dfg_quadrature(16)


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_shade_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in CONTEXT_SYMBOLS + HOST_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 21: shading from the bakes" in header


def test_shade_structs_match_c_header():
    fields = ["grid", "dSH", "dDepth", "dPlacement", "dMaps", "dProbes", "dBoxes", "dDFG", "probeCount", "res", "levels", "dfgRes"]
    lines = ['printf("%zu %zu %zu %zu\\n", sizeof(PTShadeDFG), sizeof(PTShadeMaterial), sizeof(PTShadeTerms), sizeof(PTShadeInputs));']
    lines += [f'printf("{f} %zu\\n", offsetof(PTShadeInputs, {f}));' for f in fields]
    lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for s, f in (("PTShadeMaterial", "roughness"), ("PTShadeMaterial", "flags"),
                                                                          ("PTShadeTerms", "rho"), ("PTShadeTerms", "nDotV"), ("PTShadeTerms", "occlusion"))]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = subprocess.check_output([exe]).decode().splitlines()
    assert [int(x) for x in got[0].split()] == [8, 48, 48, C.sizeof(abi.PTShadeInputs)] and C.sizeof(abi.PTShadeInputs) == 120
    offs = dict(l.split(" ") for l in got[1:])
    for f in fields:
        assert int(offs[f]) == getattr(abi.PTShadeInputs, f).offset, f
    # the row layouts the Python side and the tests index by column
    assert [int(offs[k]) for k in ("PTShadeMaterial.roughness", "PTShadeMaterial.flags", "PTShadeTerms.rho", "PTShadeTerms.nDotV", "PTShadeTerms.occlusion")] == \
        [28, 44, 12, 28, 44]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the DFG table
# ---------------------------------------------------------------------------------------------------------------------------
def test_azimuth_literals_are_float32_of_float64():
    """every literal of the header, and of the restatement's own copy, equals np.float32 of numpy's float64 value"""
    c64, s64 = ref.azimuth_float64()
    assert np.array_equal(ref.C, c64.astype(F)) and np.array_equal(ref.S, s64.astype(F))
    text = open(os.path.join(CSRC, "shade_rule.h")).read()
    for name, want in (("C", c64), ("S", s64)):
        body = re.search(r"const float %s\[64\] = \{(.*?)\};" % name, text, re.S).group(1)
        lits = re.findall(r"(-?[0-9.]+(?:e-?[0-9]+)?)f", body)
        assert len(lits) == 64, (name, len(lits))
        assert np.array_equal(np.array([F(x) for x in lits]), want.astype(F)), name


def test_dfg_twin_equals_restatement(dfg16):
    assert dfg16.shape == (16, 16, 2) and dfg16.dtype == np.float32
    assert np.array_equal(_bits(dfg16), _bits(ref.dfg_table(16)))
    t64 = plugin.bake_dfg(64)
    ij = [(0, 0), (63, 63), (5, 60), (40, 3)]
    want = ref.dfg_entries(64, [i for i, _ in ij], [j for _, j in ij])
    for k, (i, j) in enumerate(ij):
        assert np.array_equal(_bits(t64[j, i]), _bits(want[k])), (i, j)


def test_dfg_table_is_within_the_bound_of_a_fine_quadrature(dfg16, quadrature16):
    err = float(np.abs(dfg16.astype(np.float64) - quadrature16).max())
    print(f"[dfg] res 16 against 1,024 x 256 float64 samples: max |difference| = {err:.5f} (cap {DFG_CAP:.5f})")
    assert err <= DFG_CAP
    assert err >= DFG_MEASURED / 2            # the bound is the measured value's, not a loose one
    s = dfg16.sum(axis=-1)
    assert np.all(s > 0) and np.all(s <= 1 + DFG_CAP)
    for res in (32, 64):
        s = plugin.bake_dfg(res).sum(axis=-1)
        assert np.all(s > 0) and np.all(s <= 1 + DFG_CAP), res


@pytest.mark.parametrize("wrong", ["alpha_for_a2", "without_g"])
def test_dfg_bound_catches_a_wrong_rule(quadrature16, wrong):
    """a table made with alpha in place of alpha * alpha, or without G, is not within the bound"""
    bad = ref.dfg_table(16, **{wrong: True})
    err = float(np.abs(bad.astype(np.float64) - quadrature16).max())
    print(f"[dfg] {wrong}: max |difference| = {err:.4f}")
    assert err > DFG_CAP


# ---------------------------------------------------------------------------------------------------------------------------
# 2. terms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    return cases.term_rows()


@pytest.mark.parametrize("name", sorted(cases.probe_sets()))
def test_terms_twin_equals_restatement(rows, name):
    M, rays, S = rows
    assert M.shape[0] == 4096
    probes, boxes = cases.probe_sets()[name]
    got = plugin.shade_terms(M, rays, S, probes, boxes)
    want = ref.terms(M, rays, S, probes, boxes)
    for g, w, what in zip(got, want, ("terms", "receivers", "queries")):
        assert np.array_equal(_bits(g), _bits(w)), (name, what)


def test_terms_edge_cases(rows):
    M, rays, S = rows
    T, recv, qr = plugin.shade_terms(M, rays, S, *cases.probe_sets()["five"])
    # 0 / 1: a back-facing normal is turned to the viewer and gives what the front-facing one gives
    assert np.array_equal(recv[0, 4:7], [0, 0, 1]) and np.array_equal(recv[1, 4:7], [0, 0, 1])
    assert T[0, 7] == T[1, 7] == 1.0 and np.array_equal(qr[0, 4:7], [0, 0, 1])
    # 2 / 3: the view vector is normalised whatever the direction's length
    for i in (2, 3):
        assert abs(np.linalg.norm(qr[i, 4:7].astype(np.float64)) - 1) < 1e-6, i
    # 4 ... 7: metallic 0 keeps f0 = 0.04 and the base colour; metallic 1 has no diffuse and f0 = base; rho = sqrt(roughness)
    assert np.all(T[4, 4:7] == F(0.04)) and np.array_equal(T[4, 0:3], M[4, 0:3])
    assert np.all(T[5, 0:3] == 0) and np.allclose(T[5, 4:7], M[5, 0:3], atol=1e-7)
    assert T[6, 3] == np.sqrt(F(0.001)) and T[7, 3] == 1.0
    # 8: grazing; 9: a miss
    assert T[8, 7] == F(1e-4)
    assert not T[9].any() and not recv[9].any() and not qr[9, 0:7].any() and qr.view(np.uint32)[9, 7] == 0xFFFFFFFF
    # the probe choice: nearest, and the lowest index on a tie
    probes = cases.probe_sets()["five"][0].astype(np.float64)
    d2 = ((S[:, None, 0:3].astype(np.float64) - probes[None]) ** 2).sum(-1)
    gap = np.sort(d2, axis=1)
    clear = (gap[:, 1] - gap[:, 0] > 1e-5) & (np.arange(4096) != 9)
    assert np.array_equal(qr.view(np.uint32)[clear, 7], d2.argmin(1)[clear])
    for name in ("tie", "tie-boxes"):
        q = plugin.shade_terms(M, rays, S, *cases.probe_sets()[name])[2].view(np.uint32)[:, 7]
        assert set(np.unique(np.delete(q, 9))) == {0, 1}, name                       # never 2, which coincides with 0
    q = plugin.shade_terms(M, rays, S, *cases.probe_sets()["none"])[2].view(np.uint32)[:, 7]
    assert np.all(q == 0xFFFFFFFF)
    # boxes that hold some points: a point inside exactly one box takes that probe even when another is nearer
    probes, boxes = cases.probe_sets()["five-boxes-overlap"]
    q = plugin.shade_terms(M, rays, S, probes, boxes)[2].view(np.uint32)[:, 7]
    inside = np.all((boxes[None, :, 0:3] <= S[:, None, 0:3]) & (S[:, None, 0:3] <= boxes[None, :, 4:7]), axis=2)
    one = (inside.sum(1) == 1) & (np.arange(4096) != 9)
    assert one.sum() > 100 and np.array_equal(q[one], inside[one].argmax(1))
    assert (q[one] != d2.argmin(1)[one]).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. compose
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [16, 32, 64])
def test_compose_twin_equals_restatement(res):
    dfg = plugin.bake_dfg(res)
    T, E, R = cases.compose_rows(res)
    got = plugin.shade_compose(T, E, R, dfg)
    assert np.array_equal(_bits(got), _bits(ref.compose(T, E, R, dfg)))
    assert not got[-1].any() and np.all(got[:-1, 3] == 1)                            # the miss, the hits
    # at an entry's centre the table's own value comes back: nDotV = rho = 1 - 0.5 / res is the last entry
    k = np.flatnonzero((T[:, 7] == F(1 - 0.5 / res)) & (T[:, 3] == F(1 - 0.5 / res)))[0]
    ab = ref.dfg_lookup(dfg, T[k:k + 1, 7], T[k:k + 1, 3])[0]
    assert np.allclose(ab, dfg[res - 1, res - 1], atol=1e-6)
    # outside the centres the lookup clamps: nDotV = 1 and 1e-4 read the last and the first column (a fraction of 1 gives
    # p + (q - p): q within an ulp of the larger of the two)
    assert np.allclose(ref.dfg_lookup(dfg, np.array([1.0], F), np.array([0.0], F))[0], dfg[0, res - 1], rtol=0, atol=1e-6)
    assert np.allclose(ref.dfg_lookup(dfg, np.array([1e-4], F), np.array([1.0], F))[0], dfg[res - 1, 0], rtol=0, atol=1e-6)


def test_compose_constant_table_comes_back_exactly():
    T, E, R = cases.compose_rows(32)
    dfg = np.empty((32, 32, 2), F)
    dfg[..., 0], dfg[..., 1] = 0.625, 0.125
    got = plugin.shade_compose(T, E, R, dfg)[:-1]
    t = T[:-1]
    want = t[:, 8:11] + t[:, 11:12] * ((t[:, 0:3] * E[:-1, 0:3]) * ref.INV_PI + R[:-1, 0:3] * (t[:, 4:7] * F(0.625) + F(0.125)))
    assert np.array_equal(_bits(got[:, 0:3]), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _inputs(buf, **over):
    a = buf.ctypes.data
    s = abi.PTShadeInputs()
    s.grid.spacing[:] = (1.0, 1.0, 1.0)
    s.grid.counts[:] = (2, 2, 2)
    s.dSH, s.dMaps, s.dProbes, s.dDFG = a, a, a, a
    s.probeCount, s.res, s.levels, s.dfgRes = 1, 8, 2, 16
    for k, v in over.items():
        setattr(s, k, v)
    return s


def test_shade_refusals():
    lib = plugin.load_library()
    buf = np.zeros(4096, np.uint8)
    a = buf.ctypes.data
    a += (-a) % 16
    b = a + 1024
    ab = buf[a - buf.ctypes.data:]           # the aligned part, as an array
    p = abi.PTFrameParams()
    p.structSize = C.sizeof(p)
    p.OutputWidth = p.OutputHeight = 8
    pp = C.byref(p)
    ok = _inputs(ab)
    calls = {"PTBakeDFG": lambda c: lib.PTBakeDFG(c, 16, a),
             "PTShadeSurfaces": lambda c: lib.PTShadeSurfaces(c, a, a, a, 1, None, None, 0, b, None, None, None),
             "PTShadeCompose": lambda c: lib.PTShadeCompose(c, a, a, a, 1, a, 16, b),
             "PTShadeBaked": lambda c: lib.PTShadeBaked(c, C.byref(ok), a, a, a, 1, b),
             "PTShadeBakedFrame": lambda c: lib.PTShadeBakedFrame(c, pp, C.byref(ok), b, None)}
    for name, call in calls.items():
        assert call(None) == abi.PT_ERR_INVALID_ARG, name
        assert b"ctx" in lib.PTGetLastError() and name.encode() in lib.PTGetLastError()
    ctx = C.c_void_p(1)         # never dereferenced: every call below is refused on its arguments alone
    for bad in (0, 8, 17, 128):
        assert lib.PTBakeDFG(ctx, bad, a) == abi.PT_ERR_INVALID_ARG and b"res" in lib.PTGetLastError(), bad
        assert lib.PTShadeCompose(ctx, a, a, a, 1, a, bad, b) == abi.PT_ERR_INVALID_ARG and b"res" in lib.PTGetLastError(), bad
        assert lib.PTBakeDFGHost(bad, a) == 0 and b"res" in lib.PTGetBVHBuildError(), bad
        assert lib.PTShadeComposeHost(a, a, a, 1, a, bad, b) == 0 and b"res" in lib.PTGetBVHBuildError(), bad
        assert lib.PTShadeBaked(ctx, C.byref(_inputs(ab, dfgRes=bad)), a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"res" in lib.PTGetLastError(), bad
    assert lib.PTBakeDFG(ctx, 16, None) == abi.PT_ERR_INVALID_ARG and lib.PTBakeDFG(ctx, 16, a + 4) == abi.PT_ERR_INVALID_ARG
    # PTShadeSurfaces: NULL, misaligned, boxes without probes, probes missing
    for args in ((None, a, a), (a, None, a), (a, a, None)):
        assert lib.PTShadeSurfaces(ctx, *args, 1, None, None, 0, b, None, None, None) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    assert lib.PTShadeSurfaces(ctx, a, a, a, 1, None, None, 2, b, None, None, None) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    assert lib.PTShadeSurfaces(ctx, a, a, a, 1, None, a, 0, b, None, None, None) == abi.PT_ERR_INVALID_ARG and b"boxes without probes" in lib.PTGetLastError()
    for args in ((a + 8, a, a, None, None, b, None), (a, a + 4, a, None, None, b, None), (a, a, a + 8, None, None, b, None), (a, a, a, a + 8, None, b, None),
                 (a, a, a, a, a + 8, b, None), (a, a, a, None, None, b + 8, None), (a, a, a, None, None, None, b + 8)):
        rc = lib.PTShadeSurfaces(ctx, args[0], args[1], args[2], 1, args[3], args[4], 1 if args[3] else 0, args[5], args[6], None, None)
        assert rc == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError(), args
    # PTShadeCompose
    for k in range(5):
        args = [a, a, a, a, b]
        args[k] = None
        assert lib.PTShadeCompose(ctx, args[0], args[1], args[2], 1, args[3], 16, args[4]) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError(), k
    assert lib.PTShadeCompose(ctx, a + 8, a, a, 1, a, 16, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    assert lib.PTShadeCompose(ctx, a, a, a, 1, a + 4, 16, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    # PTShadeBaked / PTShadeBakedFrame: the struct
    bad_inputs = [({"res": 12}, b"res"), ({"levels": 1}, b"levels"), ({"dSH": None}, b"NULL"), ({"dDFG": None}, b"NULL"), ({"dMaps": None}, b"NULL"),
                  ({"dProbes": None}, b"NULL"), ({"dBoxes": a, "dProbes": None, "probeCount": 0}, b"boxes without probes"), ({"dSH": a + 8}, b"aligned"),
                  ({"dPlacement": a + 4}, b"aligned"), ({"dDFG": a + 4}, b"aligned")]
    for over, word in bad_inputs:
        s = _inputs(ab, **over)
        assert lib.PTShadeBaked(ctx, C.byref(s), a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and word in lib.PTGetLastError(), over
        assert lib.PTShadeBakedFrame(ctx, pp, C.byref(s), b, None) == abi.PT_ERR_INVALID_ARG and word in lib.PTGetLastError(), over
    s = _inputs(ab)
    s.grid.flags = abi.PT_GRID_VISIBILITY
    assert lib.PTShadeBaked(ctx, C.byref(s), a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"depth" in lib.PTGetLastError()
    s = _inputs(ab)
    s.grid.counts[0] = 0
    assert lib.PTShadeBaked(ctx, C.byref(s), a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeBaked(ctx, None, a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"inputs" in lib.PTGetLastError()
    assert lib.PTShadeBaked(ctx, C.byref(ok), None, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and lib.PTShadeBaked(ctx, C.byref(ok), a, a, a, 1, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeBaked(ctx, C.byref(ok), a, a, a, 1, b + 8) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    assert lib.PTShadeBakedFrame(ctx, None, C.byref(ok), b, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeBakedFrame(ctx, pp, C.byref(ok), None, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeBakedFrame(ctx, pp, C.byref(ok), b, a + 8) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    # the host twins: 0 and a message; count == 0 is fine
    assert lib.PTShadeTermsHost(None, a, a, 1, None, None, 0, b, None, None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTShadeTermsHost(a, a, a, 1, None, a, 0, b, None, None) == 0 and b"boxes without probes" in lib.PTGetBVHBuildError()
    assert lib.PTShadeTermsHost(a, a, a, 1, None, None, 3, b, None, None) == 0 and b"probes" in lib.PTGetBVHBuildError()
    assert lib.PTShadeComposeHost(a, a, a, 1, None, 16, b) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTBakeDFGHost(16, None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTShadeTermsHost(None, None, None, 0, None, None, 0, None, None, None) == 1
    assert plugin.shade_compose(np.zeros((0, 12), F), np.zeros((0, 4), F), np.zeros((0, 4), F), plugin.bake_dfg(16)).shape == (0, 4)
    with pytest.raises(plugin.PluginError):
        plugin.bake_dfg(48)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel resources and the sanitizer build
# ---------------------------------------------------------------------------------------------------------------------------
KERNELS = ["pt_shade_dfg", "pt_shade_surfaces", "pt_shade_compose", "pt_shade_baked", "pt_shade_baked_placed", "pt_shade_frame_rays"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_shade_kernel_resources():
    """no kernel of the compile unit has scratch or spills; the table of DESIGN.md 5.26 is this test's output"""
    res = resources("pt_shade_baked.hip")
    assert len(res) == len(KERNELS), sorted(res)
    for name in KERNELS:
        hits = [r for k, r in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1, (name, sorted(res))
        print(f"[resources] {name}: {hits[0]}")
        assert hits[0]["scratch"] == 0 and hits[0]["vgpr_spill"] == 0 and hits[0]["lds"] == 0, (name, hits[0])
        assert hits[0]["occupancy"] >= 4, (name, hits[0])


def test_shade_sanitize_target_runs_clean():
    """the host twins under AddressSanitizer + UBSan in a stand-alone program (csrc/shade_sanitize_main.cpp)"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", CSRC, "shade-sanitize", "SHADE_SANITIZE_OUT=" + os.path.join(d, "shade_sanitize")],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "shade ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
