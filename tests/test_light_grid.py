"""The light grid of the culled direct-light calls on the host (include/ptmi_plugin.h Part 25): the host twin
(csrc/light_grid_host.cpp) equals the numpy restatement (tests/light_grid_ref.py) byte for byte on the cases of
tests/light_grid_cases.py; the lists ascend and the overflow cell lists every light; the grid is conservative -- every pair that
PTDirectRaysHost says counts has its light in the list of the entry's cell, and a float64 evaluation says the same for points on
every cell's faces and corners --; it culls (a cap on the mean list length); refusals; the struct; the culled kernels' resources;
the sanitizer program."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin

from kernel_resources import resources
import direct_cases
import light_grid_cases as cases
import light_grid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
F = np.float32
U = np.uint32
CONTEXT_SYMBOLS = ["PTBuildLightGrid", "PTReadLightGrid", "PTLightGridInfo", "PTDirectLightCulled", "PTShadeMixedCulled", "PTShadeMixedFrameCulled"]
HOST_SYMBOLS = ["PTBuildLightGridHost"]


def _grid_cases():
    """name -> (lights, origin, cell size, dims)"""
    out = {}
    for scene, shift in (("lattice", (0.0, 0.0, 0.0)), ("instanced", cases.INSTANCED_SHIFT)):
        for g, (origin, size, dims) in cases.grids(shift).items():
            out[f"{scene}-{g}"] = (cases.lights(shift), origin, size, dims)
    L = cases.lights()
    out["odd"] = (L, (-1.3, 0.2, 0.7), 0.37, (5, 3, 4))
    out["far"] = (L + np.array([1000.0, 0, -3000.0] + [0] * 13, F)[None], (1000.0, -0.25, -3000.0), 0.75, (11, 3, 11))
    out["flat"] = (L, (0.0, 0.0, 0.0), 0.03125, (256, 1, 7))
    out["no lights"] = (np.zeros((0, 16), F), (0.0, 0.0, 0.0), 1.0, (3, 2, 1))
    for name, lights in direct_cases.light_sets().items():
        out[f"direct-{name}"] = (lights, (-3.0, -2.5, -3.0), 1.5, (4, 4, 4))
    return out


GRID_CASES = _grid_cases()


@pytest.fixture(scope="module")
def built():
    """name -> the restatement's (offsets, indices, rect_before), computed once"""
    return {name: ref.build(*c) for name, c in GRID_CASES.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_light_grid_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in CONTEXT_SYMBOLS + HOST_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 25: direct light over many lights" in header


def test_light_grid_structs_match_c_header():
    structs = {"PTLightGridParams": (abi.PTLightGridParams, ["structSize", "origin", "cellSize", "dims", "reserved"]),
               "PTLightGridStats": (abi.PTLightGridStats, ["structSize", "built", "cells", "lightCount", "longest", "stale", "entries", "generation"])}
    lines = ['printf("%zu %zu %u %u\\n", sizeof(PTLightGridParams), sizeof(PTLightGridStats), PT_LIGHT_GRID_MAX_DIM, PT_LIGHT_GRID_MAX_CELLS);']
    for s, (_, fields) in structs.items():
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fields]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = subprocess.check_output([exe]).decode().splitlines()
    assert [int(x) for x in got[0].split()] == [C.sizeof(abi.PTLightGridParams), C.sizeof(abi.PTLightGridStats), abi.PT_LIGHT_GRID_MAX_DIM,
                                                abi.PT_LIGHT_GRID_MAX_CELLS] == [36, 40, 256, 1 << 20]
    offs = dict(l.split(" ") for l in got[1:])
    for s, (ct, fields) in structs.items():
        for f in fields:
            assert int(offs[f"{s}.{f}"]) == getattr(ct, f).offset, (s, f)


# ---------------------------------------------------------------------------------------------------------------------------
# the twin against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRID_CASES))
def test_twin_equals_restatement(built, name):
    lights, origin, size, dims = GRID_CASES[name]
    offsets, indices, rect_before = plugin.build_light_grid(lights, origin, size, dims)
    want = built[name]
    assert offsets.dtype == indices.dtype == rect_before.dtype == np.uint32
    assert offsets.tobytes() == want[0].tobytes()
    assert indices.tobytes() == want[1].tobytes()
    assert rect_before.tobytes() == want[2].tobytes()


@pytest.mark.parametrize("name", sorted(GRID_CASES))
def test_lists_ascend_and_the_overflow_cell_lists_every_light(name):
    lights, origin, size, dims = GRID_CASES[name]
    offsets, indices, rect_before = plugin.build_light_grid(lights, origin, size, dims)
    cells, L = ref.cell_count(dims), lights.shape[0]
    assert offsets.shape == (cells + 2,) and offsets[0] == 0 and offsets[-1] == indices.size and (np.diff(offsets.astype(np.int64)) >= 0).all()
    assert (indices < max(L, 1)).all() or indices.size == 0
    inside = np.ones(indices.size, bool)
    inside[offsets[1:-1][offsets[1:-1] < indices.size]] = False                   # the first entry of a list has no predecessor in it
    assert (np.diff(indices.astype(np.int64))[inside[1:]] > 0).all()
    assert np.array_equal(indices[offsets[cells]:offsets[cells + 1]], np.arange(L, dtype=U))
    kinds = lights[:, 3].view(U)
    assert np.array_equal(rect_before, np.concatenate([[0], np.cumsum(kinds == cases.RECTANGLE)]).astype(U))
    listed = np.unique(indices[:offsets[cells]])
    assert np.isin(kinds[listed], (cases.POINT, cases.SPOT, cases.RECTANGLE)).all()          # a directional light has no pairs
    assert (lights[listed, 4:7] != 0).any(axis=1).all()


def test_special_lights(built):
    offsets, indices, _ = built["lattice-full"]
    cells = 8 * 2 * 8
    per_light = np.bincount(indices[:offsets[cells]], minlength=51)
    assert per_light[cases.DARK] == 0                                               # no emission: no list
    # a NaN x is never proven out of reach: whole rows of cells along x list the light, the rows its y and z reach
    assert per_light[cases.NAN_P] > 0 and per_light[cases.NAN_P] % 8 == 0
    assert per_light[cases.INF_R] == cells                                          # an infinite range, facing down from above the grid
    assert 0 < per_light[0] < 40 and per_light.max() == cells


# ---------------------------------------------------------------------------------------------------------------------------
# it culls, and never a pair that counts
# ---------------------------------------------------------------------------------------------------------------------------
def _lists_of(offsets, indices, L):
    """(cells + 1, L) bool"""
    m = np.zeros((offsets.size - 1, L), bool)
    m[np.repeat(np.arange(offsets.size - 1), np.diff(offsets.astype(np.int64))), indices] = True
    return m


@pytest.mark.parametrize("scene,shift", [("lattice", (0.0, 0.0, 0.0)), ("instanced", cases.INSTANCED_SHIFT)])
def test_every_pair_that_counts_is_listed(built, scene, shift):
    """the entries of the cases, the pairs PTDirectRaysHost says count: the pair's light is in the list of the cell of the entry's O"""
    lights = cases.lights(shift)
    rays, terms, recv = cases.entries(shift=shift)
    n, L = terms.shape[0], lights.shape[0]
    kinds = lights[:, 3].view(U)
    for strata, centered in ((1, True), (3, False)):
        pair_rays, contrib = plugin.direct_rays(lights, rays, terms, recv, strata, seed=5, centered=centered)
        pairs = pair_rays.shape[0] // n
        light_of_pair = np.repeat(np.arange(L), [1 if k in (cases.POINT, cases.SPOT) else strata * strata if k == cases.RECTANGLE else 0 for k in kinds])
        assert light_of_pair.size == pairs
        counts = (pair_rays[:, 6] > 0).reshape(n, pairs)
        assert counts.sum() > 2000
        e, p = np.nonzero(counts)
        O = pair_rays.reshape(n, pairs, 8)[e, p, 0:3]                              # a pair that counts carries the entry's O
        for g, (origin, size, dims) in cases.grids(shift).items():
            offsets, indices, _ = built[f"{scene}-{g}"]
            listed = _lists_of(offsets, indices, L)
            cell = ref.cell_of(origin, size, dims, O)
            assert listed[cell, light_of_pair[p]].all(), (g, strata)
            overflow = (cell == ref.cell_count(dims)).mean()
            print(f"[light grid] {scene} {g} S = {strata}: {e.size} pairs count, {overflow:.2f} of them in the overflow cell")
            assert (overflow > 0.2) == (g == "half") and (g != "one" or np.unique(cell).size <= 2)


def _could_count_f64(lights, X):
    """(points, L) bool in float64: the necessary conditions of a pair that counts at X -- emission, lsDistance <= range from some
    point of the light, the rectangle's front, the spot's outer cone"""
    X = X.astype(np.float64)
    out = np.zeros((X.shape[0], lights.shape[0]), bool)
    for l, row in enumerate(lights.astype(np.float64)):
        kind = int(lights[l, 3:4].view(U)[0])
        pos, emission, rng, u, v = row[0:3], row[4:7], row[7], row[8:11], row[12:15]
        if kind not in (cases.POINT, cases.SPOT, cases.RECTANGLE) or not (emission > 0).any() or not np.isfinite(pos).all():
            continue
        q = X - pos[None]
        if kind == cases.RECTANGLE:                                                 # the closest point of the rectangle (u and v are orthogonal here)
            a = np.clip(q @ u / (u @ u), 0, 1)
            b = np.clip(q @ v / (v @ v), 0, 1)
            dist = np.linalg.norm(q - a[:, None] * u[None] - b[:, None] * v[None], axis=1)
            normal = np.cross(u, v)
            ok = (dist <= rng) & (q @ normal >= 0)
        else:
            dist = np.linalg.norm(q, axis=1)
            ok = dist <= rng
            if kind == cases.SPOT:
                ok &= (q @ (u / np.linalg.norm(u))) >= v[0] * dist
        out[:, l] = ok
    return out


@pytest.mark.parametrize("name", ["lattice-full", "lattice-half", "lattice-one", "instanced-full", "odd", "far", "direct-all", "direct-spot"])
def test_faces_and_corners_in_float64(built, name):
    """27 points per cell -- corners, edge and face centres, the middle -- each pushed outwards from the cell's middle by the cell
    size times 2^-14, what the cell rule's two roundings (2^-22 relative at indices below 256) let a point of the cell lie
    outside it: a light that could count there is listed"""
    lights, origin, size, dims = GRID_CASES[name]
    offsets, indices, _ = built[name]
    cells, L = ref.cell_count(dims), lights.shape[0]
    listed = _lists_of(offsets, indices, L)[:cells]
    c = np.arange(cells)
    i = np.stack([c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1])], axis=1).astype(np.float64)
    o, s = np.asarray(origin, F).astype(np.float64), float(F(size))
    t = np.stack(np.meshgrid(*[[-1.0, 0.0, 1.0]] * 3, indexing="ij"), axis=-1).reshape(-1, 3)            # 27 offsets from the middle
    X = (o[None, None] + s * (i[:, None] + 0.5 + t[None] * (0.5 + 2.0 ** -14)))                          # (cells, 27, 3)
    could = _could_count_f64(lights, X.reshape(-1, 3)).reshape(cells, 27, L).any(axis=1)
    assert could.any() and (listed | ~could).all(), np.argwhere(could & ~listed)[:5]
    print(f"[light grid] {name}: {could.sum()} (cell, light) pairs could count, {listed.sum()} are listed")


def test_half_space_at_a_long_range():
    """A spot 5,000 units off with a range of 6,000 and an outer cone of 180 degrees, its plane through a grid of 128 x 128 x 32 cells
    of 0.0005: the entries lie within 1e-3 of the plane, where the pair rule's fp32 cosine decides many of them by its rounding.  Whatever it decides, a pair that counts has its light listed: the plane test's margin grows
    with the reach (a margin of the cell's `pad` alone would be some 1e-5 here against roundings of 5e-4)."""
    rng = np.random.default_rng(8)
    axis = np.array([0.3, -0.9, 0.2]) / np.linalg.norm([0.3, -0.9, 0.2])
    t1 = np.cross(axis, [1.0, 0.0, 0.0])
    t1 /= np.linalg.norm(t1)
    centre = np.array([0.032, 0.032, 0.008])
    spot = direct_cases.light(direct_cases.SPOT, centre + 5000.0 * t1, emission=(4e4, 4e4, 4e4), rng=6000.0, u=axis, v=(0.0, 0.9, 0.0))
    lights = spot[None]
    origin, size, dims = (0.0, 0.0, 0.0), 0.0005, (128, 128, 32)
    offsets, indices, _ = plugin.build_light_grid(lights, origin, size, dims)
    assert offsets.tobytes() == ref.build(lights, origin, size, dims)[0].tobytes()
    n = 16384
    t2 = np.cross(axis, t1)
    ab = rng.uniform(-0.005, 0.005, (n, 2))
    P = (centre[None] + ab[:, 0:1] * t1[None] + ab[:, 1:2] * t2[None] + rng.uniform(-1e-3, 1e-3, (n, 1)) * axis[None]).astype(F)      # within 1e-3 of the plane
    to_light = (spot[0:3].astype(np.float64) - P)
    N = (to_light / np.linalg.norm(to_light, axis=1, keepdims=True)).astype(F)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = P + N, -N, 1e30
    terms = np.zeros((n, 12), F)
    terms[:, 0:3], terms[:, 3], terms[:, 4:7], terms[:, 7], terms[:, 11] = 0.8, 0.7, 0.04, 1.0, 1.0
    recv = np.zeros((n, 8), F)
    recv[:, 0:3], recv[:, 4:7] = P, N
    pair_rays, _ = plugin.direct_rays(lights, rays, terms, recv, 1, centered=True)
    counts = pair_rays[:, 6] > 0
    print(f"[light grid] long range: {counts.sum()} of {n} pairs count")
    assert 0.2 < counts.mean() < 0.8                                                # the plane passes through the grid
    cell = ref.cell_of(origin, size, dims, pair_rays[counts, 0:3])
    listed = _lists_of(offsets, indices, 1)
    assert listed[cell, 0].all()


def test_the_grid_culls(built):
    """so that nothing here passes with every light in every list: over the cells of the 8 x 2 x 8 grid that hold entries, the mean
    list length is at most a quarter of the lights"""
    for scene, shift in (("lattice", (0.0, 0.0, 0.0)), ("instanced", cases.INSTANCED_SHIFT)):
        lights = cases.lights(shift)
        _, terms, recv = cases.entries(shift=shift)
        hit = terms[:, 7] > 0
        O = recv[hit, 0:3] + recv[hit, 4:7] * F(0.0001)
        origin, size, dims = cases.grids(shift)["full"]
        cell = ref.cell_of(origin, size, dims, O)
        offsets, _, _ = built[f"{scene}-full"]
        held = np.unique(cell[cell < ref.cell_count(dims)])
        lengths = np.diff(offsets.astype(np.int64))[held]
        print(f"[light grid] {scene}: {held.size} cells hold entries, mean list {lengths.mean():.2f}, longest {lengths.max()} of {lights.shape[0]} lights")
        assert held.size >= 64 and lengths.mean() <= lights.shape[0] / 4


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _bad_grids():
    def make(**over):
        p = abi.light_grid_params((0, 0, 0), 1.0, (2, 2, 2))
        for k, v in over.items():
            if k == "dims":
                p.dims[:] = v
            else:
                setattr(p, k, v)
        return p
    return [(make(dims=(0, 2, 2)), b"dims"), (make(dims=(2, 257, 2)), b"dims"), (make(dims=(2, 2, 0)), b"dims"), (make(dims=(128, 128, 128)), b"cells"),
            (make(dims=(256, 256, 17)), b"cells"), (make(cellSize=0.0), b"cellSize"), (make(cellSize=-1.0), b"cellSize"),
            (make(cellSize=float("inf")), b"cellSize"), (make(cellSize=float("nan")), b"cellSize"), (make(reserved=1), b"reserved"),
            (make(structSize=0), b"structSize"), (make(structSize=20), b"structSize")]


def test_light_grid_refusals():
    lib = plugin.load_library()
    ok = abi.light_grid_params((0, 0, 0), 1.0, (2, 2, 2))
    lights = cases.lights()
    offsets, rect_before, indices = np.zeros(10, U), np.zeros(52, U), np.zeros(600, U)
    total = C.c_uint64()
    stats = abi.PTLightGridStats()
    stats.structSize = C.sizeof(stats)
    p = abi.direct_params()
    buf = np.zeros(4096, np.uint8)
    a = buf.ctypes.data
    a += (-a) % 16
    b = a + 1024
    # a NULL context
    for name, call in {"PTBuildLightGrid": lambda c: lib.PTBuildLightGrid(c, C.byref(ok)), "PTReadLightGrid": lambda c: lib.PTReadLightGrid(c, None, None, 0, None),
                       "PTLightGridInfo": lambda c: lib.PTLightGridInfo(c, C.byref(stats)),
                       "PTDirectLightCulled": lambda c: lib.PTDirectLightCulled(c, C.byref(p), a, a, a, 1, b)}.items():
        assert call(None) == abi.PT_ERR_INVALID_ARG and b"ctx" in lib.PTGetLastError() and name.encode() in lib.PTGetLastError(), name
    ctx = C.c_void_p(1)         # never dereferenced: every call below is refused on its arguments alone
    assert lib.PTBuildLightGrid(ctx, None) == abi.PT_ERR_INVALID_ARG and b"params" in lib.PTGetLastError()
    assert lib.PTLightGridInfo(ctx, None) == abi.PT_ERR_INVALID_ARG
    unset = abi.PTLightGridStats()
    assert lib.PTLightGridInfo(ctx, C.byref(unset)) == abi.PT_ERR_INVALID_ARG and b"structSize" in lib.PTGetLastError()
    for g, word in _bad_grids():
        assert lib.PTBuildLightGrid(ctx, C.byref(g)) == abi.PT_ERR_INVALID_ARG and word in lib.PTGetLastError(), (word, lib.PTGetLastError())
        assert lib.PTBuildLightGridHost(C.byref(g), lights.ctypes.data, 51, offsets.ctypes.data, None, 0, rect_before.ctypes.data, None) == 0
        assert word in lib.PTGetBVHBuildError(), (word, lib.PTGetBVHBuildError())
    # the culled calls refuse what their counterparts refuse, on the arguments alone
    bad = abi.direct_params()
    bad.flags = 2
    assert lib.PTDirectLightCulled(ctx, C.byref(bad), a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"flag" in lib.PTGetLastError()
    assert lib.PTDirectLightCulled(ctx, None, a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"params" in lib.PTGetLastError()
    assert lib.PTDirectLightCulled(ctx, C.byref(p), None, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    assert lib.PTDirectLightCulled(ctx, C.byref(p), a, a + 8, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    assert lib.PTShadeMixedCulled(ctx, None, C.byref(p), a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"inputs" in lib.PTGetLastError()
    assert lib.PTShadeMixedFrameCulled(ctx, None, None, C.byref(bad), b, None) == abi.PT_ERR_INVALID_ARG and b"PTShadeMixedFrameCulled" in lib.PTGetLastError()
    # the host twin: 0 and a message
    okp = C.byref(ok)
    assert lib.PTBuildLightGridHost(None, lights.ctypes.data, 51, offsets.ctypes.data, None, 0, rect_before.ctypes.data, None) == 0 and b"params" in lib.PTGetBVHBuildError()
    assert lib.PTBuildLightGridHost(okp, None, 51, offsets.ctypes.data, None, 0, rect_before.ctypes.data, None) == 0 and b"lights" in lib.PTGetBVHBuildError()
    assert lib.PTBuildLightGridHost(okp, lights.ctypes.data, 51, None, None, 0, rect_before.ctypes.data, None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTBuildLightGridHost(okp, lights.ctypes.data, 51, offsets.ctypes.data, None, 0, None, None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTBuildLightGridHost(okp, lights.ctypes.data, 51, offsets.ctypes.data, None, 5, rect_before.ctypes.data, None) == 0 and b"indices" in lib.PTGetBVHBuildError()
    # a capacity below the total: the count comes back, no index is written; no lights: empty lists
    indices[:] = 0xABCD
    assert lib.PTBuildLightGridHost(okp, lights.ctypes.data, 51, offsets.ctypes.data, indices.ctypes.data, 3, rect_before.ctypes.data, C.byref(total)) == 1
    assert total.value == offsets[9] > 51 and (indices == 0xABCD).all()
    assert lib.PTBuildLightGridHost(okp, None, 0, offsets.ctypes.data, None, 0, rect_before.ctypes.data, C.byref(total)) == 1 and total.value == 0
    assert not offsets.any() and rect_before[0] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the culled kernels' resources and the sanitizer program
# ---------------------------------------------------------------------------------------------------------------------------
def test_light_grid_kernel_resources():
    """no scratch and no spill, of vector or of scalar registers, in the culled kernels and the build kernels; the culled kernels'
    LDS is the unculled ones' and their waves per SIMD as DESIGN.md 5.30 records them (5 flat, 4 with a TLAS); the unculled kernels
    keep DESIGN.md 5.29's figures with the culled ones beside them in the file"""
    rep = resources("pt_direct.hip")
    sgpr = {k: r["sgpr_spill"] for k, r in rep.items()}
    for k in ("pt_direct_light", "pt_direct_light_tlas", "pt_direct_light_grid", "pt_direct_light_grid_tlas"):
        r = rep[k]
        print(f"[light grid] {k}: {r}, scalar spill {sgpr[k]}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and sgpr[k] == 0, (k, r, sgpr[k])
    assert rep["pt_direct_light_grid"]["lds"] == rep["pt_direct_light"]["lds"] == 8 * 64 * 8 + 4
    assert rep["pt_direct_light_grid_tlas"]["lds"] == rep["pt_direct_light_tlas"]["lds"] == 8 * 64 * 8 + 32 * 64 * 4 + 4
    assert rep["pt_direct_light_grid"]["occupancy"] >= 5 and rep["pt_direct_light_grid_tlas"]["occupancy"] >= 4
    assert rep["pt_direct_light"]["occupancy"] >= 6 and rep["pt_direct_light_tlas"]["occupancy"] >= 4
    assert (rep["pt_direct_light"]["vgprs"], rep["pt_direct_light_tlas"]["vgprs"]) == (75, 110)         # as before the culled kernels stood beside them
    build = resources("pt_light_grid.hip")
    spills = {k: r["sgpr_spill"] for k, r in build.items()}
    for k in ("pt_lgrid_count", "pt_lgrid_scan", "pt_lgrid_emit"):
        r = build[k]
        print(f"[light grid] {k}: {r}, scalar spill {spills[k]}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and spills[k] == 0 and r["lds"] <= 128 and r["occupancy"] == 8, (k, r)


def test_light_grid_sanitize_program():
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", CSRC, "light-grid-sanitize", f"LIGHT_GRID_SANITIZE_OUT={os.path.join(d, 'light_grid_sanitize')}"], capture_output=True,
                             text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "light grid ok" in out.stdout
