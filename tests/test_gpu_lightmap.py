"""Lightmap charts (PTRasterizeChart / PTResolveLightmap / PathTracer.bake_lightmap, include/ptmi_plugin.h Part 14) on the MI355X.

The kernels are held to the host twins byte for byte (the twins to the numpy restatement by tests/test_lightmap.py): on the quad
and the zoo of chart_cases.py, flat and through a rotated, non-uniformly scaled instance, across many 256-texel blocks, and after
the geometry moved on the device.  A bake is the gather of its receivers, bit for bit; only the closed form under a point light has
a tolerance (5.18's 1e-5 relative, for the same arithmetic)."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import chart_cases as cases
import gather_ref
import skin_cases

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL_U32, SENTINEL_F = 0x5EA75EA7, 7.25


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tracer(scene, schedule=1, bounces=3):
    return PathTracer(scene, width=32, height=32, samplesPerPass=1, maxRayBounces=bounces, schedule=schedule)


def _device(pt, w, h, **kw):
    texels, recv = pt.chart_receivers(w, h, **kw)
    return texels.cpu().numpy().view(np.uint32), recv.cpu().numpy()


def _twin(pt, w, h, mesh=None, instance=None, uvs=None, seed=0):
    """PTRasterizeChartHost on what PTReadGeometry returns now"""
    bvh = pt._bvhScene
    _, tris, attrs = pt.read_geometry()
    _, _, t0, nt = bvh.blas_spans[0 if mesh is None else mesh]
    a0 = 0 if mesh is None else pt.scene.mesh_ranges[mesh][0]
    l2w = w2l = None
    if instance is not None and instance >= 0:
        l2w, w2l = bvh.gpu_instances[instance]["localToWorld"], bvh.gpu_instances[instance]["worldToLocal"]
    return plugin.rasterize_chart(tris[t0 * 16:t0 * 16 + nt * 48], attrs[a0:a0 + nt], w, h, uvs=uvs, local_to_world=l2w, world_to_local=w2l, seed=seed)


def _assert_same(got, want):
    assert np.array_equal(got[0], want[0]), (len(got[0]), len(want[0]))
    diff = np.nonzero((_bits(got[1]) != _bits(want[1])).any(axis=1))[0]
    assert len(diff) == 0, (len(diff), got[1][diff[:3]], want[1][diff[:3]])


# ---------------------------------------------------------------------------------------------------------------------------
# scenes, built once
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes():
    qv, qa = cases.quad_mesh()
    zv, za, caller = cases.zoo_mesh()
    return {"quad": (qv, qa), "zoo": (zv, za), "caller": caller}


@pytest.fixture(scope="module")
def flat_quad(meshes):
    pt = _tracer(cases.flat_scene(*meshes["quad"]))
    yield pt
    pt.close()


@pytest.fixture(scope="module")
def flat_zoo(meshes):
    pt = _tracer(cases.flat_scene(*meshes["zoo"]))
    yield pt
    pt.close()


@pytest.fixture(scope="module")
def instanced(meshes):
    scene, where = cases.instanced_with([meshes["quad"], meshes["zoo"]])
    pt = _tracer(scene)
    yield pt, dict(zip(("quad", "zoo"), where))
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. device against twin
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.QUAD_SIZES)
def test_quad_flat(flat_quad, size):
    w, h = size
    want = _twin(flat_quad, w, h, seed=cases.WRAP_SEED)
    assert len(want[0]) == w * h                                    # every texel once (test_lightmap.py shows the ties)
    _assert_same(_device(flat_quad, w, h, seed=cases.WRAP_SEED), want)


@pytest.mark.parametrize("size", cases.ZOO_SIZES)
@pytest.mark.parametrize("uvs", ["attr", "caller"])
def test_zoo_flat(flat_zoo, meshes, size, uvs):
    w, h = size
    u = meshes["caller"] if uvs == "caller" else None
    want = _twin(flat_zoo, w, h, uvs=u, seed=5)
    assert 0.3 * w * h < len(want[0]) < w * h
    _assert_same(_device(flat_zoo, w, h, uvs=u, seed=5), want)


@pytest.mark.parametrize("size", sorted(set(cases.QUAD_SIZES + cases.ZOO_SIZES)))
def test_through_an_instance(instanced, meshes, size):
    """instanced_scene with the quad and the zoo appended, each under a rotated, non-uniformly scaled instance"""
    pt, where = instanced
    w, h = size
    for name in [n for n, sizes in (("quad", cases.QUAD_SIZES), ("zoo", cases.ZOO_SIZES)) if size in sizes]:
        mesh, inst = where[name]
        want = _twin(pt, w, h, mesh=mesh, instance=inst, seed=9)
        local = _twin(pt, w, h, mesh=mesh, instance=-1, seed=9)
        assert np.array_equal(want[0], local[0]) and (_bits(want[1][:, 0:3]) != _bits(local[1][:, 0:3])).any(), "the instance must move the receivers"
        assert (_bits(want[1][:, 4:7]) != _bits(local[1][:, 4:7])).any(), "the instance must turn the normals"
        _assert_same(_device(pt, w, h, mesh=mesh, instance=inst, seed=9), want)
        _assert_same(_device(pt, w, h, mesh=mesh, seed=9), want)                        # the default: the mesh's first instance
        _assert_same(_device(pt, w, h, mesh=mesh, instance=-1, seed=9), local)
    if size == (64, 64):
        mesh, inst = where["zoo"]
        want = _twin(pt, w, h, mesh=mesh, instance=inst, uvs=meshes["caller"], seed=9)
        _assert_same(_device(pt, w, h, mesh=mesh, instance=inst, uvs=meshes["caller"], seed=9), want)


def test_compaction_across_blocks_and_capacity(flat_zoo):
    import torch
    w = h = 300
    want = _twin(flat_zoo, w, h, seed=1)
    n = len(want[0])
    occupied = np.zeros(w * h, np.int64)
    occupied[want[0]] = 1
    blocks = np.add.reduceat(occupied, np.arange(0, w * h, 256))
    assert (blocks == 0).sum() >= 1 and (blocks > 0).sum() >= 100 and ((blocks > 0) & (blocks < 256)).sum() >= 50, "the case must cross many blocks, partial and empty ones among them"
    _assert_same(_device(flat_zoo, w, h, seed=1), want)
    # the count-only call, a capacity of one less, and sentinels past the count
    lib, pt = plugin.load_library(), flat_zoo
    dev = torch.device(f"cuda:{pt.device}")
    d = pt._chart_desc(w, h, None, None, 1)
    count = C.c_uint64()
    plugin.check(lib.PTRasterizeChart(pt.ctx, C.byref(d), None, None, None, 0, C.byref(count)))
    assert count.value == n
    texels = torch.full((n + 64,), SENTINEL_U32, dtype=torch.int32, device=dev)
    recv = torch.full((n + 64, 8), SENTINEL_F, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    count.value = 0
    assert lib.PTRasterizeChart(pt.ctx, C.byref(d), None, texels.data_ptr(), recv.data_ptr(), n - 1, C.byref(count)) == abi.PT_ERR_INVALID_ARG
    assert count.value == n and str(n).encode() in lib.PTGetLastError()
    pt.synchronize()
    assert (texels == SENTINEL_U32).all().item() and (recv == SENTINEL_F).all().item(), "a refused call wrote something"
    plugin.check(lib.PTRasterizeChart(pt.ctx, C.byref(d), None, texels.data_ptr(), recv.data_ptr(), n + 64, C.byref(count)))
    pt.synchronize()
    assert count.value == n
    assert (texels[n:] == SENTINEL_U32).all().item() and (recv[n:] == SENTINEL_F).all().item(), "something past count was written"
    _assert_same((texels[:n].cpu().numpy().view(np.uint32), recv[:n].cpu().numpy()), want)


@pytest.mark.parametrize("size, blocks", [((16, 16), 1), ((512, 512), 1024), ((641, 409), 1025)])
def test_compaction_where_the_scan_changes_its_runs(flat_zoo, size, blocks):
    """Thread t of the scan's 1,024 owns the ceil(blocks / 1024) block counts from t times that number (csrc/pt_compact.h).  One
    block: threads 1 to 1,023 own nothing.  1,024 blocks: every thread owns exactly one.  1,025 blocks: two each, the threads
    from 513 up own nothing, and the last block holds 25 texels."""
    w, h = size
    want = _twin(flat_zoo, w, h, seed=1)
    occupied = np.zeros(w * h, np.int64)
    occupied[want[0]] = 1
    counts = np.add.reduceat(occupied, np.arange(0, w * h, 256))
    assert len(counts) == blocks and w * h - 256 * (blocks - 1) == {1: 256, 1024: 256, 1025: 25}[blocks]
    if blocks > 1:
        assert (counts == 0).sum() >= 1 and ((counts > 0) & (counts < 256)).sum() >= 50, "the case must hold partial and empty blocks"
    _assert_same(_device(flat_zoo, w, h, seed=1), want)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the current generation of the geometry
# ---------------------------------------------------------------------------------------------------------------------------
def test_chart_after_update_geometry(meshes):
    verts, attrs = meshes["zoo"]
    pt = _tracer(cases.flat_scene(verts, attrs))
    try:
        w, h = 64, 64
        before = _device(pt, w, h)
        _assert_same(before, _twin(pt, w, h))
        moved = verts.copy()
        moved[:, :3] += np.random.RandomState(5).uniform(-0.05, 0.05, (len(verts), 3)).astype(F)
        pt.update_geometry(moved)
        want = _twin(pt, w, h)
        assert np.array_equal(want[0], before[0]) and (_bits(want[1][:, :3]) != _bits(before[1][:, :3])).any(axis=1).mean() > 0.9
        _assert_same(_device(pt, w, h), want)
    finally:
        pt.close()


def test_chart_after_skin_geometry(meshes):
    verts, attrs = meshes["zoo"]
    pt = _tracer(cases.flat_scene(verts, attrs))
    try:
        w, h, J = 64, 64, 6
        before = _device(pt, w, h)
        joints, weights = skin_cases.skin_of(verts, J, seed=2)
        pt.set_skin(verts, joints, weights, rest_attrs=attrs, joint_count=J)
        pt.skin_geometry(skin_cases.palette(J, seed=3, amplitude=0.2))
        want = _twin(pt, w, h)
        assert np.array_equal(want[0], before[0])                                       # the chart is in UV space: the same texels
        assert (_bits(want[1][:, :3]) != _bits(before[1][:, :3])).any(axis=1).mean() > 0.9
        assert (_bits(want[1][:, 4:7]) != _bits(before[1][:, 4:7])).any(axis=1).mean() > 0.5      # the records' normals were skinned too
        _assert_same(_device(pt, w, h), want)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the bake is the gather
# ---------------------------------------------------------------------------------------------------------------------------
def _scatter(texels, irr, w, h):
    img = np.zeros((h * w, 4), F)
    img[texels, :3], img[texels, 3] = irr[:, :3], 1.0
    return img.reshape(h, w, 4)


@pytest.mark.parametrize("schedule", [1, 2, 3])
def test_bake_is_the_gather(schedule):
    scene = cases.lit_box()
    pt = _tracer(scene, schedule, bounces=3)
    try:
        w = h = 24
        uvs = cases.floor_only_uvs(len(scene.tri_attrs))
        p = pt.params(seed=0)
        assert p.MaxRayBounces == 3
        texels, recv = pt.chart_receivers(w, h, uvs=uvs, seed=77)
        assert texels.shape[0] == w * h                                                 # the floor fills its atlas
        irr = pt.irradiance(receivers=recv, spp=8, params=p)
        want = _scatter(texels.cpu().numpy().view(np.uint32), irr.cpu().numpy(), w, h)
        lit = (want[..., :3].max(axis=2) > 0).mean()
        print(f"[lightmap] schedule {schedule}: {lit:.2f} of the covered texels are lit")
        assert lit >= 0.1, "the emissive patch lights too little: the test would compare zeros"
        got = pt.bake_lightmap(w, h, spp=8, uvs=uvs, dilate=0, seed=77, params=p)
        assert got.shape == (h, w, 4) and (_bits(got) == _bits(want)).all()
        if schedule == 1:
            # a sample range in pieces: every bake is the fold (5.18: the sum in ascending j, over the count) of its one-sample bakes
            parts = [pt.bake_lightmap(w, h, spp=1, first_sample=j, uvs=uvs, dilate=0, seed=77, params=p) for j in range(8)]

            def fold(ps):
                rgb = ps[0][..., :3].copy()
                for e in ps[1:]:
                    rgb = rgb + e[..., :3]
                return (rgb / F(len(ps))).astype(F)
            assert (_bits(fold(parts)) == _bits(got[..., :3])).all()
            first = pt.bake_lightmap(w, h, spp=3, first_sample=0, uvs=uvs, dilate=0, seed=77, params=p)
            rest = pt.bake_lightmap(w, h, spp=5, first_sample=3, uvs=uvs, dilate=0, seed=77, params=p)
            assert (_bits(first[..., :3]) == _bits(fold(parts[:3]))).all() and (_bits(rest[..., :3]) == _bits(fold(parts[3:]))).all()
            t = pt.bake_lightmap(w, h, spp=8, uvs=uvs, dilate=0, seed=77, params=p, as_tensor=True)
            assert t.is_cuda and (_bits(t.cpu().numpy()) == _bits(want)).all()
    finally:
        pt.close()


def test_orientation_under_a_point_light():
    scene, light = cases.open_box()
    pt = _tracer(scene, 1, bounces=1)
    try:
        w = h = 16
        uvs = cases.floor_only_uvs(len(scene.tri_attrs))
        p = pt.params(seed=0)
        p.MaxRayBounces = 1
        texels, recv = pt.chart_receivers(w, h, uvs=uvs)
        recv = recv.cpu().numpy()
        assert texels.shape[0] == w * h
        got = pt.bake_lightmap(w, h, spp=4, uvs=uvs, dilate=0, params=p)
        want = np.stack([gather_ref.direct_irradiance(light, r[0:3], r[4:7]) for r in recv]).reshape(h, w, 3)
        assert (want > 0).all()
        rel = np.abs(got[..., :3].astype(np.float64) - want) / want
        print(f"[lightmap] point light over the floor: largest relative error {rel.max():.2e}")
        assert rel.max() <= 1e-5
        # the brightest texel is the one under the light: u along x, v along z, texel (0, 0) at the origin's corner
        lum = gather_ref.luminance(got[..., :3])
        y, x = np.unravel_index(lum.argmax(), lum.shape)
        lx, lz = cases.LIGHT_POS[0], cases.LIGHT_POS[2]
        assert (x, y) == (int((lx + 1) / 2 * w), int((lz + 1) / 2 * h)) == (11, 5)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. resolve
# ---------------------------------------------------------------------------------------------------------------------------
def test_resolve_device_equals_twin(flat_zoo):
    import torch
    dev = torch.device(f"cuda:{flat_zoo.device}")
    w, h = 37, 23
    texels = _twin(flat_zoo, w, h)[0]
    irr = np.random.RandomState(4).uniform(0, 4, (len(texels), 4)).astype(F)
    lists = [(w, h, texels, irr), (9, 9, np.array([40], np.uint32), np.array([[0.25, 1.5, 3.0, 9.0]], F))]
    for W, H, t, e in lists:
        dt, de = torch.from_numpy(t.view(np.int32)).to(dev), torch.from_numpy(e).to(dev)
        for dilate in (0, 1, 4):
            want = plugin.resolve_lightmap(t, e, W, H, dilate=dilate)
            got = flat_zoo.resolve_lightmap(dt, de, W, H, dilate=dilate).cpu().numpy()
            assert got.shape == (H, W, 4) and (_bits(got) == _bits(want)).all(), (W, H, dilate)
    # an index past the image is skipped on the device
    t = np.array([40, 81, 5], np.uint32)
    e = np.ones((3, 4), F)
    got = flat_zoo.resolve_lightmap(torch.from_numpy(t.view(np.int32)).to(dev), torch.from_numpy(e).to(dev), 9, 9, dilate=0).cpu().numpy()
    assert (_bits(got) == _bits(plugin.resolve_lightmap(t[[0, 2]], e[:2], 9, 9, dilate=0))).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors(instanced):
    import torch
    pt, where = instanced
    lib = plugin.load_library()
    dev = torch.device(f"cuda:{pt.device}")
    texels = torch.zeros(4096, dtype=torch.int32, device=dev)
    recv = torch.zeros((4096, 8), dtype=torch.float32, device=dev)
    image = torch.zeros((16, 16, 4), dtype=torch.float32, device=dev)
    count = C.c_uint64()
    mesh, inst = where["quad"]

    def raster(d, t=None, r=None, ctx=None):
        return lib.PTRasterizeChart(ctx or pt.ctx, C.byref(d), None, t or texels.data_ptr(), r or recv.data_ptr(), 4096, C.byref(count))

    good = pt._chart_desc(16, 16, mesh, inst, 0)
    assert raster(good) == abi.PT_OK and count.value == 256
    # no scene
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(pt.device, C.byref(ctx)))
    try:
        assert raster(good, ctx=ctx) == abi.PT_ERR_NO_SCENE
    finally:
        lib.PTDestroy(ctx)
    # offsets that name no BLAS; a wrong triangle count
    d = pt._chart_desc(16, 16, mesh, inst, 0)
    d.triOffset += 3
    assert raster(d) == abi.PT_ERR_INVALID_ARG and b"no BLAS" in lib.PTGetLastError()
    d = pt._chart_desc(16, 16, mesh, inst, 0)
    d.triangleCount += 1
    assert raster(d) == abi.PT_ERR_INVALID_ARG
    # an instance of another BLAS, and one out of range
    d = pt._chart_desc(16, 16, mesh, where["zoo"][1], 0)
    assert raster(d) == abi.PT_ERR_INVALID_ARG and b"another BLAS" in lib.PTGetLastError()
    d = pt._chart_desc(16, 16, mesh, len(pt.scene.instances), 0)
    assert raster(d) == abi.PT_ERR_INVALID_ARG
    # sizes, reserved fields, pointers
    for w, h in ((0, 16), (8193, 16), (16, 0), (16, 8193)):
        assert raster(pt._chart_desc(w, h, mesh, inst, 0)) == abi.PT_ERR_INVALID_ARG and b"8192" in lib.PTGetLastError()
    d = pt._chart_desc(16, 16, mesh, inst, 0)
    d.reserved[2] = 1
    assert raster(d) == abi.PT_ERR_INVALID_ARG and b"reserved" in lib.PTGetLastError()
    assert raster(good, r=recv.data_ptr() + 4) == abi.PT_ERR_INVALID_ARG and b"misaligned" in lib.PTGetLastError()
    assert lib.PTRasterizeChart(pt.ctx, C.byref(good), None, texels.data_ptr(), None, 4096, C.byref(count)) == abi.PT_ERR_INVALID_ARG
    assert lib.PTRasterizeChart(pt.ctx, C.byref(good), None, texels.data_ptr(), recv.data_ptr(), 4096, None) == abi.PT_ERR_INVALID_ARG
    # resolve
    args = (texels.data_ptr(), recv.data_ptr(), 4)
    assert lib.PTResolveLightmap(pt.ctx, *args, 16, 16, 17, image.data_ptr()) == abi.PT_ERR_INVALID_ARG and b"dilate" in lib.PTGetLastError()
    assert lib.PTResolveLightmap(pt.ctx, *args, 0, 16, 1, image.data_ptr()) == abi.PT_ERR_INVALID_ARG
    assert lib.PTResolveLightmap(pt.ctx, *args, 8193, 16, 1, image.data_ptr()) == abi.PT_ERR_INVALID_ARG
    assert lib.PTResolveLightmap(pt.ctx, *args, 16, 16, 1, image.data_ptr() + 4) == abi.PT_ERR_INVALID_ARG and b"misaligned" in lib.PTGetLastError()
    assert lib.PTResolveLightmap(pt.ctx, *args, 16, 16, 1, None) == abi.PT_ERR_INVALID_ARG
    # the context still works
    assert raster(good) == abi.PT_OK and count.value == 256
    pt.synchronize()
