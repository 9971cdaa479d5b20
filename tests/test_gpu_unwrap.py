"""Lightmap UVs (PTUnwrapCharts / PTEmitChartUVs, include/ptmi_plugin.h Part 23) on the MI355X.

The rule is bit-exact and the kernels are held to the host twins without tolerances, for both corner sources, over the cases of
tests/unwrap_cases.py; then after geometry updates, with two meshes in one atlas, and end to end: unwrap, rasterise, resolve, bind,
look up at the first hits of a frame, and a real bake over the UVs."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import chart_cases
import lightmap_lookup_ref
import skin_cases
import unwrap_cases as cases

pytestmark = pytest.mark.gpu

F = np.float32
NO_CHART = abi.PT_UNWRAP_NO_CHART
SENTINEL = 0x5EA75EA7
CASES = {**cases.small_cases(), **cases.cut_cases(), **cases.scene_cases()}
ATLAS = {"material-zoo": (512, 512, 16.0, 2), "instanced-mesh-0": (256, 256, 12.0, 1), "strip-4096-permuted": (8192, 64, 2.0, 0), "strip-300": (1024, 16, 5.5, 3),
         "soup": (4096, 512, 4.0, 1), "grid-moved": (256, 256, 5.0, 2)}
MAX_SWEEPS = 32         # a condition of the issue: the sweep model reads 9 on the hardest case here (the permuted strip)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tracer(vertices, **kw):
    attrs = np.zeros(len(vertices) // 3, abi.TRI_ATTR)
    return PathTracer(chart_cases.flat_scene(np.ascontiguousarray(vertices, F), attrs), width=8, height=8, **kw)


def _span(pt, mesh):
    _, _, t0, nt = pt._bvhScene.blas_spans[0 if mesh is None else mesh]
    return t0, nt


def _rows(pt, mesh=None):
    """the BLAS's triangle rows as PTReadGeometry returns them now"""
    t0, nt = _span(pt, mesh)
    return pt.read_geometry()[1][t0 * 16:t0 * 16 + nt * 48]


def _device_charts(pt, vertices=None, mesh=None):
    """PTUnwrapCharts: the count-only form, then exactly sized arrays with sentinels behind them -> (chart_of_prim, charts, stats,
    the device tensors for the emit)"""
    import torch
    dev = pt._device
    nt = _span(pt, mesh)[1]
    d = abi.unwrap_desc(nt, pt._blas_offsets(mesh))
    d_verts = None if vertices is None else torch.from_numpy(np.ascontiguousarray(vertices, F)).to(dev)
    v_ptr = None if d_verts is None else d_verts.data_ptr()
    n, st0, st = C.c_uint32(), abi.PTUnwrapStats(), abi.PTUnwrapStats()
    with pt._ordered(dev):
        plugin.check(pt.lib.PTUnwrapCharts(pt.ctx, C.byref(d), v_ptr, None, None, 0, C.byref(n), C.byref(st0)))
    count = n.value
    of = torch.full((nt + 3,), SENTINEL, dtype=torch.int32, device=dev)
    charts = torch.full((count + 2, 8), SENTINEL, dtype=torch.int32, device=dev)
    with pt._ordered(dev):
        if count:
            n.value = 0
            rc = pt.lib.PTUnwrapCharts(pt.ctx, C.byref(d), v_ptr, of.data_ptr(), charts.data_ptr(), count - 1, C.byref(n), None)
            assert rc == abi.PT_ERR_INVALID_ARG and n.value == count                 # count > capacity: the count, and nothing written
            torch.cuda.synchronize()
            assert (of == SENTINEL).all() and (charts == SENTINEL).all()
        plugin.check(pt.lib.PTUnwrapCharts(pt.ctx, C.byref(d), v_ptr, of.data_ptr(), charts.data_ptr(), count, C.byref(n), C.byref(st)))
    assert n.value == count
    assert (of[nt:] == SENTINEL).all() and (charts[count:] == SENTINEL).all()
    # the sweeps are the one figure that depends on the order the hooks arrive in: two runs may differ in it
    same = lambda s: {k: v for k, v in s.as_dict().items() if k != "sweeps"}
    assert same(st) == same(st0) and 1 <= st.sweeps <= MAX_SWEEPS and 1 <= st0.sweeps <= MAX_SWEEPS, (st.as_dict(), st0.as_dict())
    h_charts = charts[:count].cpu().numpy().view(abi.UNWRAP_CHART_DTYPE).reshape(-1)
    return of[:nt].cpu().numpy().view(np.uint32), h_charts, st.as_dict(), (d, d_verts, of, charts)


def _device_uvs(pt, handles, count, origins, width, height, tpu, padding):
    import torch
    dev = pt._device
    d, d_verts, of, charts = handles
    nt = d.triangleCount
    uvs = torch.full((nt + 2, 6), 7.25, dtype=torch.float32, device=dev)
    d_origins = torch.from_numpy(np.ascontiguousarray(origins, np.int32).reshape(-1, 2)).to(dev) if count else torch.zeros((1, 2), dtype=torch.int32, device=dev)
    with pt._ordered(dev):
        plugin.check(pt.lib.PTEmitChartUVs(pt.ctx, C.byref(d), None if d_verts is None else d_verts.data_ptr(), of.data_ptr(), charts.data_ptr(),
                                           d_origins.data_ptr(), count, width, height, padding, tpu, uvs.data_ptr()))
    assert (uvs[nt:] == 7.25).all()
    return uvs[:nt]


def _check_against_twin(pt, vertices, name, mesh=None):
    """the device calls against the twins over the same corner source: the vertices, or the rows PTReadGeometry returns"""
    tris = None if vertices is not None else _rows(pt, mesh)
    of, charts, stats, handles = _device_charts(pt, vertices, mesh)
    want_of, want_charts, want_stats = plugin.unwrap_charts(tris, vertices, return_stats=True)
    assert np.array_equal(of, want_of), name
    assert charts.tobytes() == want_charts.tobytes(), name
    sweeps = stats.pop("sweeps")
    want_stats.pop("sweeps")
    assert stats == want_stats, (name, stats, want_stats)
    width, height, tpu, padding = ATLAS.get(name, (96, 80, 7.25, 2))
    origins, _ = plugin.pack_charts(want_charts, width, height, tpu, padding)
    assert origins is not None, name
    uvs = _device_uvs(pt, handles, len(charts), origins, width, height, tpu, padding)
    want_uvs = plugin.emit_chart_uvs(tris, want_of, want_charts, origins, width, height, tpu, padding, vertices=vertices)
    assert (_bits(uvs) == _bits(want_uvs)).all(), name
    return of, charts, sweeps


# ---------------------------------------------------------------------------------------------------------------------------
# 1. device against twin
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_twin(name):
    vertices, scene_vertices, expected = CASES[name]
    pt = _tracer(scene_vertices)
    try:
        _, charts, sweeps = _check_against_twin(pt, vertices, name)
        if expected is not None:
            assert len(charts) == expected, (len(charts), expected)
        _, _, sweeps_records = _check_against_twin(pt, None, name)
        print(f"[unwrap] {name}: {len(charts)} charts, sweeps {sweeps} (vertices) {sweeps_records} (records)")
    finally:
        pt.close()


def test_wrapper_fits_a_density_and_keeps_everything_on_the_device():
    import torch
    v = CASES["material-zoo"][0]
    pt = _tracer(v)
    try:
        u = pt.unwrap_lightmap(512, 512, vertices=torch.from_numpy(v).to(pt._device))
        of, charts = plugin.unwrap_charts(None, v)
        tpu, rejected = plugin.fit_chart_density(charts, 512, 512, 2)
        assert u.texels_per_unit == tpu and tpu > 16.0 and rejected > tpu
        origins, rows = plugin.pack_charts(charts, 512, 512, tpu, 2)
        assert np.array_equal(u.origins, origins) and u.rows_used == rows and u.charts.tobytes() == charts.tobytes()
        assert np.array_equal(u.chart_of_prim.cpu().numpy().view(np.uint32), of) and u.stats["single_charts"] == 13
        assert (_bits(u.uvs) == _bits(plugin.emit_chart_uvs(None, of, charts, origins, 512, 512, tpu, 2, vertices=v))).all()
        with pytest.raises(ValueError):
            pt.unwrap_lightmap(64, 64, texels_per_unit=64.0)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. after an update
# ---------------------------------------------------------------------------------------------------------------------------
def test_null_source_sees_updated_geometry():
    v = cases.grid(16, 9, cut=257)
    pt = _tracer(v)
    try:
        before = _rows(pt).copy()
        _, charts0, _ = _check_against_twin(pt, None, "grid-257")
        moved = v.copy()
        moved[:, 2] = v[:, 0] * F(3.0) + v[:, 1] * F(0.25)                         # steeper than 45 degrees: the class turns to x
        moved[: 3 * 40, 2] += F(0.5)                                               # and the first 40 triangles come off the rest
        pt.update_geometry(moved)
        assert not np.array_equal(_rows(pt), before)
        _, charts1, _ = _check_against_twin(pt, None, "grid-moved")
        assert (charts0["cls"] >> 1 == 2).all() and (charts1["cls"] >> 1 == 0).all() and len(charts1) > len(charts0)
    finally:
        pt.close()


def test_null_source_sees_skinned_geometry():
    from test_gpu_geometry_update import soup_scene
    from test_refit import soup
    ntri, joints_n = 300, 64
    rest = soup(ntri, 40 + ntri)
    pt = PathTracer(soup_scene(rest), width=8, height=8)
    try:
        joints, weights = skin_cases.skin_of(rest, joints_n, 3 * ntri + joints_n)
        pt.set_skin(rest, joints, weights, joint_count=joints_n)
        _, charts0, _ = _check_against_twin(pt, None, "soup")
        pt.skin_geometry(skin_cases.palette(joints_n, 5))
        _, charts1, _ = _check_against_twin(pt, None, "soup")
        assert charts0.tobytes() != charts1.tobytes()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. two meshes in one atlas
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_meshes_share_an_atlas():
    import torch
    scene = scenes.instanced_scene()
    pt = PathTracer(scene, width=8, height=8)
    try:
        size, tpu, padding = 256, 10.0, 2
        parts = []
        for mesh in (0, 1):
            t0, nt = scene.mesh_ranges[mesh]
            v = scene.vertices[t0 * 3:(t0 + nt) * 3]
            of, charts, _, handles = _device_charts(pt, v, mesh)
            want = plugin.unwrap_charts(None, v)
            assert np.array_equal(of, want[0]) and charts.tobytes() == want[1].tobytes()
            parts.append((mesh, v, of, charts, handles))
        both = np.concatenate([p[3] for p in parts])
        origins, rows = plugin.pack_charts(both, size, size, tpu, padding)
        assert origins is not None, rows
        seen = np.zeros(size * size, bool)
        first = 0
        for mesh, v, of, charts, handles in parts:
            mine = origins[first:first + len(charts)]
            first += len(charts)
            uvs = _device_uvs(pt, handles, len(charts), mine, size, size, tpu, padding)
            assert (_bits(uvs) == _bits(plugin.emit_chart_uvs(None, of, charts, mine, size, size, tpu, padding, vertices=v))).all()
            texels, _ = pt.chart_receivers(size, size, mesh=mesh, uvs=uvs.contiguous())
            texels = texels.cpu().numpy()
            assert len(texels) > 100 and not seen[texels].any(), mesh
            seen[texels] = True
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. end to end in the closed box
# ---------------------------------------------------------------------------------------------------------------------------
TPU, SIZE, FRAME = 32.0, 256, (48, 32)


def _taps_all_baked(image, x, y):
    """the four taps of the footprint at (x, y) lie in the image and have w == 1"""
    h, w = image.shape[:2]
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    inside = (x0 >= 0) & (y0 >= 0) & (x0 + 1 < w) & (y0 + 1 < h)
    cx, cy = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    ones = (image[cy, cx, 3] == 1) & (image[cy, cx + 1, 3] == 1) & (image[cy + 1, cx, 3] == 1) & (image[cy + 1, cx + 1, 3] == 1)
    return inside & ones


def test_end_to_end_positions_come_back_through_the_atlas():
    """The lightmap holds every receiver's own position, so a lookup at a first hit must return the hit point: within the bilinear
    filter's rounding where all four taps were baked, within three texels of the surface where a dilated tap takes part.
    The twins' chain over the same hits reads a largest interior deviation of 5.0741e-07 (positions up to 2 in a box of 2 x 2 x 2; DESIGN.md
    5.28); the device is held to twice what the twins read in this run."""
    import torch
    pt = PathTracer(chart_cases.lit_box(), width=FRAME[0], height=FRAME[1], samplesPerPass=1, maxRayBounces=2, schedule=1)
    try:
        dev = pt._device
        u = pt.unwrap_lightmap(SIZE, SIZE, texels_per_unit=TPU)
        assert len(u.charts) == 7 and u.stats["excluded"] == 0                       # six walls and the light patch
        texels, recv = pt.chart_receivers(SIZE, SIZE, uvs=u.uvs)
        irr = torch.zeros((recv.shape[0], 4), dtype=torch.float32, device=dev)
        irr[:, 0:3] = recv[:, 0:3]
        image = pt.resolve_lightmap(texels, irr, SIZE, SIZE, dilate=2)
        pt.bind_lightmaps([pt.lightmap_binding(image, uvs=u.uvs)])
        cam = pt.camera_rays()
        rays = np.zeros((cam.shape[0], 8), F)
        rays[:, 0:6], rays[:, 6] = cam[:, 0:6], 1e30
        d_rays = torch.from_numpy(rays).to(dev)
        hits, surf = pt.trace_rays(d_rays, surface=True)
        got, which = pt.lightmap_lookup(d_rays, hits, surf)
        got, which = got.cpu().numpy(), which.cpu().numpy().view(np.uint32)
        hits, surf = hits.cpu().numpy(), surf.cpu().numpy()
        assert (which == 0).all()                                                   # every hit finds the binding
        point = rays[:, 0:3].astype(np.float64) + hits[:, 0:1].astype(np.float64) * rays[:, 3:6].astype(np.float64)
        # the same chain through the host twins
        _, tris, attrs = pt.read_geometry()
        h_of, h_charts = plugin.unwrap_charts(tris)
        h_origins, _ = plugin.pack_charts(h_charts, SIZE, SIZE, TPU)
        h_uvs = plugin.emit_chart_uvs(tris, h_of, h_charts, h_origins, SIZE, SIZE, TPU)
        assert (_bits(h_uvs) == _bits(u.uvs)).all()
        h_texels, h_recv = plugin.rasterize_chart(tris, attrs, SIZE, SIZE, uvs=h_uvs)
        h_irr = np.zeros((len(h_texels), 4), F)
        h_irr[:, 0:3] = h_recv[:, 0:3]
        h_image = plugin.resolve_lightmap(h_texels, h_irr, SIZE, SIZE, dilate=2)
        assert (_bits(h_image) == _bits(image)).all()
        table = [{"image": h_image, "first_prim": 0, "prim_count": len(h_of), "instance": None, "uvs": h_uvs, "two_sided": False}]
        want, want_which = plugin.lightmap_lookup(table, attrs, pt._bvhScene.materials.reshape(-1, 32).shape[0], rays, hits, surf)
        assert (want_which == 0).all()
        _, _, x, y = lightmap_lookup_ref.lookup(table, attrs, pt._bvhScene.materials.reshape(-1, 32).shape[0], rays, hits, surf, details=True)
        interior = _taps_all_baked(h_image, x, y)
        twin_dev = np.abs(want[:, 0:3].astype(np.float64) - point).max(axis=1)
        gpu_dev = np.abs(got[:, 0:3].astype(np.float64) - point).max(axis=1)
        print(f"[unwrap] end to end: {interior.sum()} of {len(interior)} interior; largest deviation interior twin {twin_dev[interior].max():.4e} "
              f"gpu {gpu_dev[interior].max():.4e}; all entries twin {twin_dev.max():.4e} gpu {gpu_dev.max():.4e} (3 / tpu = {3 / TPU:.4e})")
        assert interior.sum() >= 0.9 * len(interior)
        assert gpu_dev[interior].max() <= 2 * twin_dev[interior].max()
        assert gpu_dev.max() <= 3 / TPU
    finally:
        pt.bind_lightmaps([])
        pt.close()


def test_a_real_bake_over_the_unwrapped_uvs():
    pt = PathTracer(chart_cases.lit_box(), width=8, height=8, samplesPerPass=1, maxRayBounces=2, schedule=1)
    try:
        u = pt.unwrap_lightmap(SIZE, SIZE)
        assert u.texels_per_unit > TPU and u.rows_used <= SIZE
        texels, _ = pt.chart_receivers(SIZE, SIZE, uvs=u.uvs)
        image = pt.bake_lightmap(SIZE, SIZE, spp=16, uvs=u.uvs)
        assert np.isfinite(image).all()
        baked = np.zeros(SIZE * SIZE, bool)
        baked[texels.cpu().numpy()] = True
        assert np.array_equal(image[:, :, 3].reshape(-1) == 1, baked) and baked.sum() > 0.3 * SIZE * SIZE
        assert image[baked.reshape(SIZE, SIZE)][:, 0:3].max() > 0
    finally:
        pt.close()
