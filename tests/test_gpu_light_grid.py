"""The light grid and the culled direct-light calls (PTBuildLightGrid / PTReadLightGrid / PTLightGridInfo, PTDirectLightCulled /
PTShadeMixedCulled / PTShadeMixedFrameCulled; include/ptmi_plugin.h Part 25) on the MI355X.

Everything here is held without a tolerance: the grid built on the GPU equals the host twin byte for byte; the culled calls equal
their unculled counterparts bit for bit -- on both scenes, on each of the three grids, centred and jittered, at every list length,
with sentinels past `count` untouched --; a stale grid is refused."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
from test_gpu_shade_baked import Baked, _box, _bits
import light_grid_cases as cases
import light_grid_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
W, H = cases.W, cases.H
MISS = 0xFFFFFFFF
CULLED = ["PTBuildLightGrid", "PTReadLightGrid", "PTLightGridInfo", "PTDirectLightCulled", "PTShadeMixedCulled", "PTShadeMixedFrameCulled"]
for _name in CULLED:
    getattr(plugin.load_library(), _name)               # before the feature exists the whole of this file fails here
SHIFT = {"lattice": (0.0, 0.0, 0.0), "instanced": cases.INSTANCED_SHIFT}


class _Lit(Baked):
    """a Baked tracer under the lattice of lights; `grid` names the light grid the context holds.  The bakes are made under ordinary
    lights -- a path that picks the light with a NaN position bakes a NaN --; the three special lights arrive with update_lights"""
    grid = None

    def __init__(self, which, scene, lo, hi):
        super().__init__(scene, lo, hi)
        self.pt.update_lights(cases.lights(SHIFT[which]))

    def use(self, which, name):
        if self.grid != name:
            origin, size, dims = cases.grids(SHIFT[which])[name]
            self.pt.build_light_grid(origin, size, dims)
            self.grid = name


@pytest.fixture(scope="module")
def lattice():
    b = _Lit("lattice", cases.scene(special=False), (0.5, 0.2, 0.5), (7.5, 1.8, 7.5))
    yield b
    b.close()


@pytest.fixture(scope="module")
def instanced():
    s = cases.instanced_scene(special=False)
    eye, target = np.asarray(s.camera.eye, F), np.asarray(s.camera.target, F)
    r = F(0.6) * np.linalg.norm(target - eye).astype(F)
    b = _Lit("instanced", s, target - r, target + r)
    yield b
    b.close()


def _list(b, n, seed=5):
    """n rays from the camera's eye into the scene around its view direction; every 7th ends before anything (a miss), so every
    wave of the list mixes hits and misses"""
    import torch
    rng = np.random.default_rng(seed)
    eye, target = np.asarray(b.scene.camera.eye, np.float64), np.asarray(b.scene.camera.target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    d = fwd + rng.normal(size=(n, 3)) * 0.45
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = eye
    rays[:, 3:6] = d * rng.uniform(0.5, 2.0, (n, 1))             # not of unit length
    rays[:, 6] = np.where(np.arange(n) % 7 == 3, 1e-6, 1e30)
    return torch.from_numpy(rays).to(b.pt._device)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the build
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lattice", "instanced"])
@pytest.mark.parametrize("grid", ["full", "half", "one"])
def test_build_equals_the_twin(request, which, grid):
    b = request.getfixturevalue(which)
    pt = b.pt
    origin, size, dims = cases.grids(SHIFT[which])[grid]
    info = pt.build_light_grid(origin, size, dims)
    b.grid = grid
    want = plugin.build_light_grid(pt.light_records(), origin, size, dims)
    got = pt.light_grid()
    for g, w in zip(got, want):
        assert g.dtype == np.uint32 and g.tobytes() == w.tobytes()
    cells = ref.cell_count(dims)
    lengths = np.diff(want[0].astype(np.int64))
    assert info == {"built": 1, "cells": cells, "lightCount": 51, "longest": int(lengths[:cells].max()), "stale": 0, "entries": int(want[0][-1]),
                    "generation": info["generation"]}
    assert (pt.light_grid()[1] == got[1]).all()                                     # reading twice reads the same
    again = pt.build_light_grid(origin, size, dims)                                 # and building twice builds the same
    assert again == info and all(g.tobytes() == w.tobytes() for g, w in zip(pt.light_grid(), want))


def test_a_stale_grid_is_refused_until_it_is_rebuilt(lattice):
    pt = lattice.pt
    lattice.use("lattice", "full")
    origin, size, dims = cases.grids()["full"]
    rays = _list(lattice, 300)
    hits, surf = pt.trace_rays(rays, surface=True)
    kw = dict(strata=2, seed=3)
    before = pt.direct_light(rays, hits, surf, culled=True, **kw)
    records = pt.light_records()
    moved = records.copy()
    moved[6, 0:3] += np.array([2.6, 0.1, 1.7], F)
    gen = pt.light_grid_info()["generation"]
    try:
        pt.update_lights(moved)
        info = pt.light_grid_info()
        assert info["stale"] == 1 and info["built"] == 1 and info["generation"] == gen
        args = (lattice.params, lattice.volume, lattice.reflections, lattice.dfg)
        for call in (lambda: pt.direct_light(rays, hits, surf, culled=True, **kw),
                     lambda: pt.shade_mixed(rays, hits, surf, *args[1:], culled=True, **kw), lambda: pt.render_mixed(*args, culled=True, **kw)):
            with pytest.raises(plugin.PluginError) as e:
                call()
            assert e.value.code == abi.PT_ERR_INVALID_ARG and "stale" in str(e.value)
        unculled = pt.direct_light(rays, hits, surf, **kw)                          # the unculled call does not care
        info = pt.build_light_grid(origin, size, dims)
        assert info["stale"] == 0 and info["generation"] == gen + 1
        want = plugin.build_light_grid(moved, origin, size, dims)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(pt.light_grid(), want))
        assert want[1].tobytes() != plugin.build_light_grid(records, origin, size, dims)[1].tobytes()
        after = pt.direct_light(rays, hits, surf, culled=True, **kw)
        assert (_bits(after) == _bits(unculled)).all() and (_bits(after) != _bits(before)).any()
    finally:
        pt.update_lights(records)
        lattice.grid = None
    lattice.use("lattice", "full")
    assert (_bits(pt.direct_light(rays, hits, surf, culled=True, **kw)) == _bits(before)).all()


def test_calls_need_a_scene_and_a_grid(lattice):
    import torch
    pt = lattice.pt
    lib = pt.lib
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(pt.device, C.byref(ctx)))
    try:
        rays = _list(lattice, 4)
        hits, surf = pt.trace_rays(rays, surface=True)
        out = torch.zeros((8, 4), dtype=torch.float32, device=rays.device)
        torch.cuda.synchronize()
        p, g = abi.direct_params(), abi.light_grid_params((0, 0, 0), 1.0, (2, 2, 2))
        a = (rays.data_ptr(), hits.data_ptr(), surf.data_ptr())
        assert lib.PTBuildLightGrid(ctx, C.byref(g)) == abi.PT_ERR_NO_SCENE
        assert lib.PTDirectLightCulled(ctx, C.byref(p), *a, 4, out.data_ptr()) == abi.PT_ERR_NO_SCENE
        assert lib.PTReadLightGrid(ctx, None, None, 0, None) == abi.PT_ERR_INVALID_ARG and b"no light grid" in lib.PTGetLastError()
        s = abi.PTLightGridStats()
        s.structSize = C.sizeof(s)
        assert lib.PTLightGridInfo(ctx, C.byref(s)) == abi.PT_OK and s.built == 0
        # a scene, no grid yet: refused, with a count of 0 too
        plugin.check(lib.PTSetScene(ctx, C.byref(pt._bvhScene.desc())))
        for n in (4, 0):
            assert lib.PTDirectLightCulled(ctx, C.byref(p), *a, n, out.data_ptr()) == abi.PT_ERR_INVALID_ARG and b"no light grid" in lib.PTGetLastError()
        plugin.check(lib.PTBuildLightGrid(ctx, C.byref(g)))
        assert lib.PTDirectLightCulled(ctx, C.byref(p), *a, 4, out.data_ptr()) == abi.PT_OK
        # PTSetScene makes it stale
        plugin.check(lib.PTSetScene(ctx, C.byref(pt._bvhScene.desc())))
        assert lib.PTDirectLightCulled(ctx, C.byref(p), *a, 4, out.data_ptr()) == abi.PT_ERR_INVALID_ARG and b"stale" in lib.PTGetLastError()
        few = np.zeros(3, U)
        assert lib.PTReadLightGrid(ctx, None, few.ctypes.data, 3, None) == abi.PT_ERR_INVALID_ARG and b"indexCapacity" in lib.PTGetLastError()
        plugin.check(lib.PTSynchronize(ctx))
    finally:
        lib.PTDestroy(ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the culled fused call
# ---------------------------------------------------------------------------------------------------------------------------
KWS = (dict(strata=1, centered=True), dict(strata=1, seed=11), dict(strata=3, centered=True, min_alpha=0.1), dict(strata=3, seed=12))


@pytest.mark.parametrize("which", ["lattice", "instanced"])
@pytest.mark.parametrize("grid", ["full", "half", "one"])
def test_culled_equals_unculled(request, which, grid):
    import torch
    b = request.getfixturevalue(which)
    pt = b.pt
    b.use(which, grid)
    for n in (1, 63, 64, 65, 257, 1500):
        rays = _list(b, n, seed=n)
        hits, surf = pt.trace_rays(rays, surface=True)
        for kw in KWS:
            p = abi.direct_params(**kw)
            out = torch.full((n + 3, 4), -7.0, dtype=torch.float32, device=rays.device)
            with pt._ordered(rays.device):
                plugin.check(pt.lib.PTDirectLightCulled(pt.ctx, C.byref(p), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr()))
            assert (out[n:].cpu().numpy() == -7.0).all()                            # nothing past count
            want = pt.direct_light(rays, hits, surf, **kw)
            assert (_bits(out[:n]) == _bits(want)).all(), (n, kw)
            assert (_bits(pt.direct_light(rays, hits, surf, culled=True, **kw)) == _bits(want)).all()
        if n == 1500:
            g = want.cpu().numpy()
            miss = hits.cpu().numpy().view(U)[:, 3] == MISS
            first_wave = miss[:64]
            assert first_wave.any() and not first_wave.all()                        # hits and misses within a wave
            assert miss.sum() >= 1500 // 7 and not g[miss].any() and (g[~miss, 3] == 1).all() and np.isfinite(g).all() and (g[:, 0:3] > 0).any()
            lit = (g[~miss, 0:3] > 0).any(axis=1).mean()
            print(f"[light grid] {which} {grid}: {lit:.2f} of the hits are lit")
            assert lit > 0.3


@pytest.mark.parametrize("which", ["lattice", "instanced"])
def test_a_wave_over_many_cells(request, which):
    """the list in a shuffled order: the entries of one wave lie in many cells with different lists, so the union merge has lanes
    that advance at different lights"""
    import torch
    b = request.getfixturevalue(which)
    pt = b.pt
    b.use(which, "full")
    origin, size, dims = cases.grids(SHIFT[which])["full"]
    rays = _list(b, 1500, seed=77)
    rays = rays[torch.from_numpy(np.random.default_rng(1).permutation(1500)).to(rays.device)].contiguous()
    hits, surf = pt.trace_rays(rays, surface=True)
    _, terms, recv, _ = (x.cpu().numpy() for x in pt.shade_surfaces(rays, hits, surf))
    O = recv[:, 0:3] + recv[:, 4:7] * F(0.0001)
    cell = ref.cell_of(origin, size, dims, O)
    offsets, indices, _ = pt.light_grid()
    hit = terms[:, 7] > 0
    different = []
    for w in range(0, 1500, 64):
        lists_of_wave = {indices[offsets[c]:offsets[c + 1]].tobytes() for c in cell[w:w + 64][hit[w:w + 64]]}
        different.append(len(lists_of_wave))
    print(f"[light grid] {which}: different lists per wave: min {min(different)}, max {max(different)}")
    assert min(different) >= 4
    for kw in KWS:
        assert (_bits(pt.direct_light(rays, hits, surf, culled=True, **kw)) == _bits(pt.direct_light(rays, hits, surf, **kw))).all(), kw


@pytest.mark.parametrize("which", ["lattice", "instanced"])
@pytest.mark.parametrize("cell", [None, 1.25])
def test_fitted_grid(request, which, cell):
    """fit_light_grid takes the box from the scene's bounds -- the instances' world boxes under a TLAS --: the grid covers the hits (none
    takes the overflow cell but those on the far faces), equals the twin for the same box, and the culled call equals the unculled one"""
    b = request.getfixturevalue(which)
    pt = b.pt
    info = pt.fit_light_grid(cell)
    b.grid = None
    lo, hi = pt._scene_bounds()
    size = float((hi - lo).max() / 32) if cell is None else cell
    dims = np.maximum(np.ceil((hi - lo).astype(np.float64) / size * (1 + 1e-6)), 1).astype(int)
    assert info["built"] == 1 and info["stale"] == 0 and info["cells"] == int(dims.prod()) and info["lightCount"] == 51
    want = plugin.build_light_grid(pt.light_records(), lo, size, dims)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(pt.light_grid(), want))
    rays = _list(b, 1500, seed=31)
    hits, surf = pt.trace_rays(rays, surface=True)
    _, terms, recv, _ = (x.cpu().numpy() for x in pt.shade_surfaces(rays, hits, surf))
    hit = terms[:, 7] > 0
    cell_of = ref.cell_of(lo, size, dims, recv[hit, 0:3] + recv[hit, 4:7] * F(0.0001))
    assert (cell_of < info["cells"]).mean() > 0.9                                   # the hits lie in the box: only a far face's can fall out
    assert info["longest"] < 51                                                     # it culls
    for kw in KWS:
        assert (_bits(pt.direct_light(rays, hits, surf, culled=True, **kw)) == _bits(pt.direct_light(rays, hits, surf, **kw))).all(), kw


def test_an_empty_list_still_meets_the_refusal(lattice):
    """the host layer makes the culled call for an empty list too: a stale grid is refused there as anywhere; a current one gives
    an empty result"""
    pt = lattice.pt
    lattice.use("lattice", "full")
    rays = _list(lattice, 4)
    hits, surf = pt.trace_rays(rays, surface=True)
    empty = pt.direct_light(rays[:0], hits[:0], surf[:0], culled=True)
    assert tuple(empty.shape) == (0, 4)
    assert tuple(pt.direct_light(np.zeros((0, 8), F), np.zeros((0, 4), F), np.zeros((0, 12), F), culled=True).shape) == (0, 4)
    records = pt.light_records()
    try:
        pt.update_lights(records)                                                   # the same lights, a new generation
        for call in (lambda: pt.direct_light(rays[:0], hits[:0], surf[:0], culled=True),
                     lambda: pt.shade_mixed(rays[:0], hits[:0], surf[:0], lattice.volume, lattice.reflections, lattice.dfg, culled=True)):
            with pytest.raises(plugin.PluginError) as e:
                call()
            assert e.value.code == abi.PT_ERR_INVALID_ARG and "stale" in str(e.value)
        assert tuple(pt.direct_light(rays[:0], hits[:0], surf[:0]).shape) == (0, 4)  # the unculled call is not made at all
    finally:
        lattice.grid = None


def test_no_lights_gives_zero_and_one():
    """the shade box has no lights: the grid's lists are empty, hits get {0, 0, 0, 1}"""
    import torch
    pt = PathTracer(_box(), width=W, height=H, samplesPerPass=1, maxRayBounces=2, schedule=1)
    try:
        info = pt.build_light_grid((-1.0, 0.0, -1.0), 0.5, (4, 4, 4))
        assert info["entries"] == 0 and info["longest"] == 0 and info["lightCount"] == 0 and info["cells"] == 64
        offsets, indices, rect_before = pt.light_grid()
        assert not offsets.any() and indices.size == 0 and rect_before.tolist() == [0]
        rng = np.random.default_rng(2)
        rays = np.zeros((300, 8), F)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6] = (0.0, 1.0, -0.9), np.array([0.0, -0.5, 1.0]) + rng.normal(size=(300, 3)) * 0.6, 1e30
        rays[::7, 6] = 1e-6
        rays = torch.from_numpy(rays).to(pt._device)
        hits, surf = pt.trace_rays(rays, surface=True)
        got = pt.direct_light(rays, hits, surf, strata=2, culled=True).cpu().numpy()
        miss = hits.cpu().numpy().view(U)[:, 3] == MISS
        assert miss.any() and not got[miss].any() and (got[~miss] == np.array([0, 0, 0, 1], F)).all()
        assert (_bits(got) == _bits(pt.direct_light(rays, hits, surf, strata=2))).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. mixed: the list call and a frame
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lattice", "instanced"])
def test_mixed_culled_equals_mixed(request, which):
    b = request.getfixturevalue(which)
    pt = b.pt
    b.use(which, "full")
    rays = _list(b, 1500)
    hits, surf = pt.trace_rays(rays, surface=True)
    kw = dict(strata=2, seed=9, min_alpha=0.05)
    want = pt.shade_mixed(rays, hits, surf, b.volume, b.reflections, b.dfg, **kw)
    got = pt.shade_mixed(rays, hits, surf, b.volume, b.reflections, b.dfg, culled=True, **kw)
    assert (_bits(got) == _bits(want)).all()
    assert (_bits(got) != _bits(pt.shade_lightmapped(rays, hits, surf, b.volume, b.reflections, b.dfg))).any()


@pytest.mark.parametrize("which", ["lattice", "instanced"])
def test_frame_culled_equals_frame(request, which):
    b = request.getfixturevalue(which)
    pt = b.pt
    b.use(which, "half")
    kw = dict(strata=2, seed=3)
    want, want_rays = pt.render_mixed(b.params, b.volume, b.reflections, b.dfg, return_rays=True, **kw)
    got, rays = pt.render_mixed(b.params, b.volume, b.reflections, b.dfg, return_rays=True, culled=True, **kw)
    assert got.shape == (H, W, 4) and (_bits(rays) == _bits(want_rays)).all()
    assert (_bits(got) == _bits(want)).all()
    assert (_bits(got) != _bits(pt.render_lightmapped(b.params, b.volume, b.reflections, b.dfg))).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the stress build
# ---------------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRESS = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib", "libpt-stress-small-stacks.so")
STRESS_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import light_grid_cases as cases
data, out = np.load(sys.argv[2]), {}
for name, s, shift in (("lattice", cases.scene(), (0.0, 0.0, 0.0)), ("instanced", cases.instanced_scene(), cases.INSTANCED_SHIFT)):
    pt = PathTracer(s, width=48, height=32, samplesPerPass=1, maxRayBounces=2, schedule=1)
    rays = data[name]
    hits, surf = pt.trace_rays(rays, surface=True)
    kw = dict(strata=3, seed=77, min_alpha=0.05)
    pt.build_light_grid(*cases.grids(shift)["full"])
    out[name + "_culled"] = pt.direct_light(rays, hits, surf, culled=True, **kw)
    _, terms, recv, _ = pt.shade_surfaces(rays, hits, surf)
    pair_rays, contrib = pt.direct_rays(rays, terms, recv, **kw)
    pair_hits = pt.trace_rays(pair_rays, any_hit=True)
    out[name + "_steps"] = pt.direct_accumulate(terms, contrib, pair_hits, pt.direct_pair_count(3))
    pt.close()
np.savez(sys.argv[3], **out)
'''


def test_grid_stride_and_slab_in_the_stress_build(lattice, instanced, tmp_path):
    """The stress build launches the culled kernels on at most 4 waves and keeps ONE CWBVH stack entry per lane in LDS: a list of
    1,500 entries makes every wave take six chunks, each with a cursor of its own, and every walk that descends goes through the slab.
    There the culled call equals the four-call composition, and both equal the product build's bits."""
    assert os.path.exists(STRESS), "the stress library is built with the product (make stress)"
    lists = {"lattice": _list(lattice, 1500, seed=21), "instanced": _list(instanced, 1500, seed=22)}
    src, out = str(tmp_path / "rays.npz"), str(tmp_path / "stress.npz")
    np.savez(src, **{k: v.cpu().numpy() for k, v in lists.items()})
    subprocess.check_call([sys.executable, "-c", STRESS_CHILD, ROOT, src, out], env=dict(os.environ, PT_PLUGIN=STRESS), timeout=300)
    got = np.load(out)
    for name, b in (("lattice", lattice), ("instanced", instanced)):
        rays = lists[name]
        b.use(name, "full")
        hits, surf = b.pt.trace_rays(rays, surface=True)
        want = b.pt.direct_light(rays, hits, surf, culled=True, strata=3, seed=77, min_alpha=0.05)
        assert (_bits(got[name + "_culled"]) == _bits(got[name + "_steps"])).all(), name
        assert (_bits(got[name + "_culled"]) == _bits(want)).all() and (got[name + "_culled"][:, 0:3] > 0).any(), name
