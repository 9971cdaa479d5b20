"""Scene updates (PTUpdateInstances / Lights / Materials, PTReadTLAS, include/ptmi_plugin.h Part 5) on the MI355X.

Every update is checked against the path that already exists: BuildTLAS for the TLAS bytes, and a fresh PTSetScene of the
updated scene for frames, counters, ray queries and guides."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STRESS = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib", "libpt-stress-small-stacks.so")
W, H = 64, 48

_tracers = {}


def tracer_with(n):
    """A context holding a HAS_TLAS scene of n instances (the instances' boxes are then replaced by the test's)."""
    if n not in _tracers:
        _tracers[n] = PathTracer(scenes.instanced_scene(count=n - 1, detail=4), width=8, height=8)
    return _tracers[n]


def records(lo, hi):
    n = lo.shape[0]
    r = np.zeros(n, dtype=abi.BLAS_INSTANCE)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    r["localToWorld"] = eye
    r["worldToLocal"] = eye
    r["aabbMin"] = lo.astype(np.float32)
    r["aabbMax"] = hi.astype(np.float32)
    r["blasIndex"] = np.arange(n)
    return r


def gpu_tlas(rec, device=True):
    import torch
    n = rec.shape[0]
    pt = tracer_with(n)
    if device:
        t = torch.from_numpy(rec.view(np.uint8).copy()).to(f"cuda:{pt.device}")
        pt.update_instances_device(t)
    else:
        plugin.check(pt.lib.PTUpdateInstances(pt.ctx, rec.ctypes.data, n))
    return pt.read_tlas()


def assert_same_tlas(rec, device=True):
    want_nodes, want_idx = plugin.build_tlas(rec)
    got_nodes, got_idx = gpu_tlas(rec, device)
    assert got_nodes.nbytes == want_nodes.nbytes, (got_nodes.nbytes // 64, want_nodes.nbytes // 64)
    assert np.array_equal(got_nodes, want_nodes)
    assert np.array_equal(got_idx, want_idx)


def random_boxes(n, seed, spread=10.0, size=1.0):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-spread, spread, (n, 3))
    h = rng.uniform(0.01, size, (n, 3))
    return c - h, c + h


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "tlas_*.npz"))), ids=os.path.basename)
def test_tlas_bytes_goldens(path):
    g = np.load(path)
    rec = g["instances"].view(abi.BLAS_INSTANCE).copy()
    nodes, idx = gpu_tlas(rec)
    assert np.array_equal(nodes, g["nodes"]) and np.array_equal(idx, g["indices"])


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 201, 1000, 4096, 65536])
def test_tlas_bytes_random(n):
    for seed in (1, 2):
        assert_same_tlas(records(*random_boxes(n, seed + n)), device=seed == 1)


def test_tlas_bytes_degenerate():
    rng = np.random.RandomState(5)
    n = 300
    lo, hi = random_boxes(n, 9)
    assert_same_tlas(records(np.tile(lo[:1], (n, 1)), np.tile(hi[:1], (n, 1))))          # identical boxes
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[:, 1], hi2[:, 1] = 0.0, 0.0                                                         # zero extent on y
    assert_same_tlas(records(lo2, hi2))
    lo3, hi3 = lo.copy(), hi.copy()
    lo3[:, 1], hi3[:, 1] = -0.0, 0.0                                                        # signed zeros
    lo3[::3, 1] = 0.0
    hi3[1::3, 1] = -0.0
    assert_same_tlas(records(lo3, hi3))
    tiny = rng.uniform(0, 1, (n, 3)) * 1e-20                                                # extents near 1e-20 of the root's
    lo4, hi4 = tiny, tiny + 1e-21
    lo4[0], hi4[0] = (0, 0, 0), (1, 1, 1)
    assert_same_tlas(records(lo4, hi4))
    assert_same_tlas(records(hi, lo))                                                       # inverted boxes
    # 4096 boxes: the cooperative (whole-workgroup) path on shared coordinates
    lo5, hi5 = random_boxes(4096, 3)
    lo5[:, 1], hi5[:, 1] = 0.0, 2.0
    lo5[::2, 2] = -0.0
    assert_same_tlas(records(lo5, hi5))


def test_tlas_bytes_deep_chain():
    # boxes at x = 2^-i: every split peels the largest off, the rest goes left -- a chain of left edges.  BuildTLAS's
    # depth-first conversion keeps 128 stack words, so the chain stays within its 64 left edges.
    n = 60
    x = 2.0 ** -np.arange(n)
    lo = np.stack([x, np.zeros(n), np.zeros(n)], 1)
    hi = np.stack([x * 1.001, np.full(n, 1e-3), np.full(n, 1e-3)], 1)
    assert_same_tlas(records(lo, hi))


# ---------------------------------------------------------------------------------------------------------------------
# frames, counters, queries, guides against a fresh PTSetScene
# ---------------------------------------------------------------------------------------------------------------------
def moved(scene, seed):
    rng = np.random.RandomState(seed)
    out = []
    for k, (_, m, _) in enumerate(scene.instances):
        m = np.array(m, np.float64)
        if k:
            m = scenes._trs((rng.uniform(-3, 3), rng.uniform(0.5, 1.6), rng.uniform(-3, 3)), rng.uniform(0, 360), 0.0,
                            (rng.uniform(0.6, 1.4),) * 3)
        out.append(m)
    return out


def render(pt, passes=4, seed0=0x51):
    pt.set_stats_level(1)
    pt.reset_stats()
    pt.Reset()
    for k in range(passes):
        pt.OnRenderImage(seed=seed0 + k)
    return pt.readback(), pt.stats().as_dict()


def frames_case(schedule):
    base = scenes.instanced_scene()
    A, B = moved(base, 1), moved(base, 2)
    upd = PathTracer(scenes.with_transforms(base, A), width=W, height=H, schedule=schedule)
    render(upd, 1)
    assert upd.set_instance_transforms(B)
    assert not upd.set_instance_transforms(B)
    got, gst = render(upd)
    ref = PathTracer(scenes.with_transforms(base, B), width=W, height=H, schedule=schedule)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), schedule
    assert gst == wst, (gst, wst)
    upd.close()
    ref.close()


@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4])
def test_frames_after_update(schedule):
    frames_case(schedule)


def test_frames_after_update_stress_build():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests');"
            "import test_gpu_scene_update as m; [m.frames_case(s) for s in (1, 4)]")
    subprocess.check_call([sys.executable, "-c", code, ROOT], env=dict(os.environ, PT_PLUGIN=STRESS), timeout=900)


def test_ordering_with_passes_in_flight():
    import torch
    base = scenes.instanced_scene()
    T = [moved(base, s) for s in (3, 4, 5)]
    statics = []
    for t in T:
        ref = PathTracer(scenes.with_transforms(base, t), width=W, height=H)
        statics.append(render(ref, 1)[0])
        ref.close()
    for host in (False, True):
        pt = PathTracer(scenes.with_transforms(base, T[0]), width=W, height=H)
        pt.set_passes_in_flight(12)
        dev = f"cuda:{pt.device}"
        outs = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in T]
        torch.cuda.synchronize()
        p = pt.params(seed=0x51)
        pt.render_pass_to(p, outs[0].data_ptr())
        for k in (1, 2):
            rec = pt._bvhScene.blas_instances.copy()
            bvh = pt._bvhScene
            for i, m in enumerate(T[k]):
                t0, n = base.mesh_ranges[base.instances[i][0]]
                lo, hi = scenes.instance_world_bounds(base.vertices[t0 * 3:(t0 + n) * 3], m)
                rec[i]["localToWorld"] = m.T.reshape(16).astype(np.float32)
                rec[i]["worldToLocal"] = np.linalg.inv(m).T.reshape(16).astype(np.float32)
                rec[i]["aabbMin"], rec[i]["aabbMax"] = lo, hi
            if host:
                plugin.check(pt.lib.PTUpdateInstances(pt.ctx, rec.ctypes.data, rec.shape[0]))
                rec[:] = np.zeros(1, dtype=abi.BLAS_INSTANCE)            # the library copied the array before returning
            else:
                t = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
                pt.update_instances_device(t)
            del bvh
            pt.render_pass_to(p, outs[k].data_ptr())
        pt.synchronize()
        torch.cuda.synchronize()
        for k in range(3):
            got = outs[k].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), statics[k].view(np.uint32)), (host, k)
        pt.close()


def test_queries_and_guides_after_update():
    base = scenes.instanced_scene()
    A, B = moved(base, 6), moved(base, 7)
    upd = PathTracer(scenes.with_transforms(base, A), width=W, height=H)
    upd.set_instance_transforms(B)
    ref = PathTracer(scenes.with_transforms(base, B), width=W, height=H)
    rays = np.stack([upd.camera_ray(x, y) for y in range(0, H, 3) for x in range(0, W, 3)])
    h1, s1 = upd.trace_rays(rays, surface=True)
    h2, s2 = ref.trace_rays(rays, surface=True)
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    for pt in (upd, ref):
        pt.render_guides(4)
    g1, g2 = upd.guides(), ref.guides()
    for a, b in zip(g1, g2):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    upd.close()
    ref.close()


def test_lights_and_materials_after_update():
    from dataclasses import replace
    base = scenes.material_zoo()
    upd = PathTracer(base, width=W, height=H)
    lights = base.lights.copy()
    lights[:, 0:3] += np.float32(0.25)                 # move and recolour (first rows: position, colour)
    lights[:, 4:7] *= np.float32(0.7)
    mats = base.materials.copy()
    mats[:, 0:3] = mats[:, 0:3][::-1].copy() if len(mats) > 1 else mats[:, 0:3]
    upd.update_lights(lights)
    upd.update_materials(mats)
    got, gst = render(upd)
    ref = PathTracer(replace(base, lights=lights, materials=mats), width=W, height=H)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and gst == wst
    if base.texture_data.size:
        bad = mats.copy()
        bad[0, 22] = 1e6
        with pytest.raises(plugin.PluginError) as e:
            upd.update_materials(bad)
        assert e.value.code == abi.PT_ERR_INVALID_ARG
    upd.close()
    ref.close()


def test_bounce_animation():
    base = scenes.instanced_scene(count=20)
    pt = PathTracer(base, width=W, height=H)
    for f in range(8):
        t = f / 30.0
        T = scenes.bounce_transforms(base, t)
        pt.set_instance_transforms(T)
        got, _ = render(pt, 1, seed0=0x77 + f)
        ref = PathTracer(scenes.with_transforms(base, T), width=W, height=H)
        want, _ = render(ref, 1, seed0=0x77 + f)
        ref.close()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
    pt.close()


def test_argument_errors():
    lib = plugin.load_library()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    buf = np.zeros(4096, np.uint8)
    cnt = C.c_uint32()
    for rc in (lib.PTUpdateInstances(ctx, buf.ctypes.data, 1), lib.PTUpdateInstancesDevice(ctx, buf.ctypes.data, 1),
               lib.PTUpdateLights(ctx, buf.ctypes.data, 1), lib.PTUpdateMaterials(ctx, buf.ctypes.data, 1),
               lib.PTReadTLAS(ctx, buf.ctypes.data, buf.nbytes, buf.ctypes.data, 1, C.byref(cnt))):
        assert rc == abi.PT_ERR_NO_SCENE
    lib.PTDestroy(ctx)
    flat = PathTracer(scenes.cornell_box(), width=8, height=8)                     # no TLAS
    rec = np.zeros(1, dtype=abi.BLAS_INSTANCE)
    assert lib.PTUpdateInstances(flat.ctx, rec.ctypes.data, 1) == abi.PT_ERR_UNSUPPORTED
    assert lib.PTUpdateInstancesDevice(flat.ctx, rec.ctypes.data, 1) == abi.PT_ERR_UNSUPPORTED
    flat.close()
    s = scenes.instanced_scene(count=4, detail=4)
    pt = PathTracer(s, width=8, height=8)
    rec = pt._bvhScene.blas_instances.copy()
    n = rec.shape[0]
    assert lib.PTUpdateInstances(pt.ctx, None, n) == abi.PT_ERR_INVALID_ARG
    assert lib.PTUpdateInstancesDevice(pt.ctx, None, n) == abi.PT_ERR_INVALID_ARG
    assert lib.PTUpdateInstances(pt.ctx, rec.ctypes.data, n - 1) == abi.PT_ERR_INVALID_ARG
    assert lib.PTUpdateInstancesDevice(pt.ctx, rec.ctypes.data, n + 1) == abi.PT_ERR_INVALID_ARG
    for field, k in (("aabbMin", 1), ("localToWorld", 5), ("worldToLocal", 0)):
        bad = rec.copy()
        bad[2][field][k] = np.nan if k != 0 else np.inf
        assert lib.PTUpdateInstances(pt.ctx, bad.ctypes.data, n) == abi.PT_ERR_INVALID_ARG
    L = s.lights.astype(np.float32)
    assert lib.PTUpdateLights(pt.ctx, None, 1) == abi.PT_ERR_INVALID_ARG
    assert lib.PTUpdateLights(pt.ctx, L.ctypes.data, 0) == abi.PT_ERR_INVALID_ARG
    assert lib.PTUpdateLights(pt.ctx, L.ctypes.data, L.shape[0] + 1) == abi.PT_ERR_INVALID_ARG
    M = s.materials.astype(np.float32)
    assert lib.PTUpdateMaterials(pt.ctx, None, M.shape[0]) == abi.PT_ERR_INVALID_ARG
    assert lib.PTUpdateMaterials(pt.ctx, M.ctypes.data, M.shape[0] - 1) == abi.PT_ERR_INVALID_ARG
    small = np.zeros(64, np.uint8)
    idx = np.zeros(n, np.uint32)
    assert lib.PTReadTLAS(pt.ctx, small.ctypes.data, small.nbytes, idx.ctypes.data, n, C.byref(cnt)) == abi.PT_ERR_INVALID_ARG
    assert lib.PTReadTLAS(pt.ctx, None, 0, idx.ctypes.data, n, C.byref(cnt)) == abi.PT_ERR_INVALID_ARG
    # before any update PTReadTLAS returns what PTSetScene was given
    nodes, got = pt.read_tlas()
    assert np.array_equal(nodes.view(np.float32), pt._bvhScene.tlas_data[:pt._bvhScene.tlas_index_offset])
    assert np.array_equal(got.view(np.float32), pt._bvhScene.tlas_data[pt._bvhScene.tlas_index_offset:])
    pt.close()
    from dataclasses import replace
    dark = PathTracer(replace(scenes.instanced_scene(count=2, detail=4), lights=np.zeros((0, 16), np.float32)), width=8, height=8)
    assert lib.PTUpdateLights(dark.ctx, L.ctypes.data, 1) == abi.PT_ERR_UNSUPPORTED
    dark.close()
