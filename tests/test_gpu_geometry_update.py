"""Geometry updates (PTUpdateGeometry / PTUpdateGeometryDevice / PTReadGeometry, include/ptmi_plugin.h Part 9) on the MI355X.

The device refit is checked against the host refit (PTRefitBVH, itself pinned by tests/test_refit.py) byte for byte, and
everything rendered or queried after an update against a fresh PTSetScene of the host-refitted arrays, bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_refit import deformed, soup
from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRESS = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib", "libpt-stress-small-stacks.so")
W, H = 64, 64


def soup_scene(v):
    base = scenes.cornell_box()
    attrs = np.zeros(v.shape[0] // 3, dtype=abi.TRI_ATTR)
    return scenes.Scene("soup", v, attrs, base.materials, base.lights, base.texture_data, base.camera)


def new_attrs(attrs, seed):
    """The same records with other normals and tangents (materialIndex and uvs kept)."""
    rng = np.random.RandomState(seed)
    out = attrs.copy()
    f = out.view(np.float32).reshape(-1, 32)
    d = rng.normal(0, 1, (f.shape[0], 6, 3))
    f.reshape(-1, 8, 4)[:, :6, :3] = (d / np.linalg.norm(d, axis=2, keepdims=True)).astype(np.float32)     # rows 0-5: normals, tangents
    return out


def to_device(pt, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(f"cuda:{pt.device}").view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# bytes against the host refit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", [1, 2, 3, 4, 9, 64, 300, 5000, 100000])
def test_bytes_equal_the_host_refit(ntri):
    v = soup(ntri, 40 + ntri)
    pt = PathTracer(soup_scene(v), width=8, height=8)
    built = (pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris)
    got = pt.read_geometry()                                   # before any update: what PTSetScene was given
    assert np.array_equal(got[0], built[0]) and np.array_equal(got[1], built[1])
    assert np.array_equal(got[2].view(np.uint8), pt._bvhScene.tri_attrs.view(np.uint8))
    attrs = pt._bvhScene.tri_attrs
    for step, device in enumerate((False, True, False)):      # three updates: both generations are written, the first one twice
        w = deformed(v, 11 + step)
        give_attrs = step != 2
        if give_attrs:
            attrs = new_attrs(attrs, step)
        if device:
            pt.update_geometry(to_device(pt, w), tri_attrs=to_device(pt, attrs) if give_attrs else None)
        else:
            pt.update_geometry(w, tri_attrs=attrs if give_attrs else None)
        want_n, want_t = plugin.refit_cwbvh(built, w)
        got_n, got_t, got_a = pt.read_geometry()
        bad = np.nonzero((got_n.reshape(-1, 80) != want_n.reshape(-1, 80)).any(axis=1))[0]
        assert bad.size == 0, (ntri, step, bad[:8], got_n.size // 80)
        assert np.array_equal(got_t, want_t), (ntri, step)
        assert np.array_equal(got_a.view(np.uint8), attrs.view(np.uint8)), (ntri, step)
    pt.close()


def mesh_slices(scene):
    """Byte ranges of every mesh's BLAS in the node / triangle buffers, as BVHScene lays them out."""
    out, n_off, t_off = [], 0, 0
    for t0, n in scene.mesh_ranges:
        nb, tb = plugin.build_cwbvh(scene.vertices[t0 * 3:(t0 + n) * 3])
        out.append((n_off, n_off + nb.nbytes, t_off, t_off + tb.nbytes))
        n_off += nb.nbytes
        t_off += tb.nbytes
    return out


def compose(scene, slices, nodes, tris, mesh, w):
    """nodes / tris with mesh's BLAS refitted to w on the host"""
    n0, n1, t0, t1 = slices[mesh]
    rn, rt = plugin.refit_cwbvh((nodes[n0:n1], tris[t0:t1]), w)
    nodes, tris = nodes.copy(), tris.copy()
    nodes[n0:n1], tris[t0:t1] = rn, rt
    return nodes, tris


@pytest.mark.parametrize("ntri", [300, 5000])
def test_device_built_tree(ntri):
    """A tree of PTBuildBVHDevice passes the refit's walk too: PTRefitBVH on its handle, PTRefitBVHArrays on its arrays and
    PTUpdateGeometry on a scene built from it give the same bytes, and the boxes contain the deformed triangles."""
    import refit_ref
    lib = plugin.load_library()
    v = soup(ntri, 70 + ntri)
    w = deformed(v, 3)
    pt = PathTracer(soup_scene(v), width=8, height=8, build_device=0)
    built = (pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris)
    want_n, want_t = plugin.refit_cwbvh(built, w)
    assert refit_ref.decoded_boxes_contain(want_n, want_t, w) >= ntri // 3
    pt.update_geometry(w)
    got_n, got_t, _ = pt.read_geometry()
    assert np.array_equal(got_n, want_n) and np.array_equal(got_t, want_t)
    pt.close()
    h = lib.PTBuildBVHDevice(0, v.ctypes.data, ntri)              # a second build may order its nodes differently: its own arrays
    assert h >= 0
    try:
        def arrays():
            ok, pn, ptr = plugin.TinyBVH.GetCWBVHData(h)
            assert ok
            return (np.ctypeslib.as_array(C.cast(pn, C.POINTER(C.c_uint8)), shape=(lib.GetCWBVHNodesSize(h),)).copy(),
                    np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(lib.GetCWBVHTrisSize(h),)).copy())
        before = arrays()
        plugin.refit_cwbvh(h, w)
        after = arrays()
    finally:
        lib.DestroyBVH(h)
    want = plugin.refit_cwbvh(before, w)
    assert np.array_equal(after[0], want[0]) and np.array_equal(after[1], want[1])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_carry_over_between_generations(device):
    """Mesh 1, then mesh 0, then mesh 1 again: every update writes the generation that is not current, so what it does not
    rewrite must have been carried over -- after each step the WHOLE buffers equal the host-side composition."""
    s = scenes.instanced_scene(count=5, detail=6)
    pt = PathTracer(s, width=8, height=8)
    slices = mesh_slices(s)
    nodes, tris, attrs = pt._bvhScene.bvh_nodes.copy(), pt._bvhScene.bvh_tris.copy(), pt._bvhScene.tri_attrs.copy()
    for step, mesh in enumerate((1, 0, 1)):
        t0, n = s.mesh_ranges[mesh]
        w = deformed(s.vertices[t0 * 3:(t0 + n) * 3], 20 + step, amplitude=0.05)
        a = None
        if step != 1:                                          # the attribute generations flip less often than the geometry's
            a = new_attrs(attrs[t0:t0 + n], 30 + step)
            attrs[t0:t0 + n] = a
        if device:                                             # bytes only: the TLAS is not what this test is about
            k = next(i for i, inst in enumerate(s.instances) if inst[0] == mesh)
            off = [int(pt._bvhScene.gpu_instances[k][f]) for f in ("bvhOffset", "triOffset", "triAttributeOffset")]
            dw, da = to_device(pt, w), None if a is None else to_device(pt, a)
            import torch
            torch.cuda.synchronize()
            plugin.check(pt.lib.PTUpdateGeometryDevice(pt.ctx, *off, dw.data_ptr(), n, None if da is None else da.data_ptr()))
        else:
            pt.update_geometry(w, mesh=mesh, tri_attrs=a)
        nodes, tris = compose(s, slices, nodes, tris, mesh, w)
        got_n, got_t, got_a = pt.read_geometry()
        assert np.array_equal(got_n, nodes) and np.array_equal(got_t, tris), step
        assert np.array_equal(got_a.view(np.uint8), attrs.view(np.uint8)), step
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# frames, counters, queries, guides against a fresh PTSetScene of the host-refitted arrays
# ---------------------------------------------------------------------------------------------------------------------
def render(pt, passes=4, seed0=0x51):
    pt.set_stats_level(1)
    pt.reset_stats()
    pt.Reset()
    for k in range(passes):
        pt.OnRenderImage(seed=seed0 + k)
    return pt.readback(), pt.stats().as_dict()


def instance_bounds(pt, scene, mesh, w, blas):
    """blas with the world bounds of mesh's instances recomputed from the deformed local vertices w"""
    blas = blas.copy()
    for k, (m, _, _) in enumerate(scene.instances):
        if m == mesh:
            l2w = pt._bvhScene.gpu_instances[k]["localToWorld"].reshape(4, 4).T.astype(np.float64)
            blas[k]["aabbMin"], blas[k]["aabbMax"] = scenes.instance_world_bounds(w, l2w)
    return blas


def set_arrays(ref, nodes, tris, attrs=None, blas=None):
    """A fresh PTSetScene of ref's scene with these geometry arrays (and instance records)"""
    b = ref._bvhScene
    b.bvh_nodes, b.bvh_tris = np.ascontiguousarray(nodes), np.ascontiguousarray(tris)
    if attrs is not None:
        b.tri_attrs = np.ascontiguousarray(attrs)
    if blas is not None:
        b.blas_instances = blas
        tn, ti = plugin.build_tlas(blas)
        b.tlas_index_offset = tn.nbytes // 4
        b.tlas_data = np.concatenate([tn.view(np.float32), ti.view(np.float32)])
    b.PrepareShader(ref.ctx)


def flat_case(schedule, scene=None):
    s = scene or scenes.material_zoo()
    upd = PathTracer(s, width=W, height=H, schedule=schedule)
    ref = PathTracer(s, width=W, height=H, schedule=schedule)
    built = (ref._bvhScene.bvh_nodes, ref._bvhScene.bvh_tris)
    render(upd, 1)
    w = deformed(s.vertices, 5, amplitude=0.01)
    upd.update_geometry(w)
    got, gst = render(upd)
    set_arrays(ref, *plugin.refit_cwbvh(built, w))
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), schedule
    assert gst == wst, (gst, wst)
    upd.close()
    ref.close()


def tlas_case(schedule):
    s = scenes.instanced_scene()
    upd = PathTracer(s, width=W, height=H, schedule=schedule)
    ref = PathTracer(s, width=W, height=H, schedule=schedule)
    slices = mesh_slices(s)
    nodes, tris, blas = ref._bvhScene.bvh_nodes, ref._bvhScene.bvh_tris, ref._bvhScene.blas_instances
    render(upd, 1)
    for mesh in (0, 2):
        t0, n = s.mesh_ranges[mesh]
        w = deformed(s.vertices[t0 * 3:(t0 + n) * 3], 6 + mesh, amplitude=0.08)
        upd.update_geometry(w, mesh=mesh)                      # resends the instances' bounds
        nodes, tris = compose(s, slices, nodes, tris, mesh, w)
        blas = instance_bounds(ref, s, mesh, w, blas)
    got, gst = render(upd)
    set_arrays(ref, nodes, tris, blas=blas)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), schedule
    assert gst == wst, (gst, wst)
    upd.close()
    ref.close()


@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4])
def test_frames_after_update_flat(schedule):
    flat_case(schedule)


@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4])
def test_frames_after_update_tlas(schedule):
    tlas_case(schedule)


def test_frames_after_update_cornell():
    flat_case(None, scenes.cornell_box())                      # one node: the megakernel by default


def test_frames_after_update_stress_build():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests');"
            "import test_gpu_geometry_update as m; [(m.flat_case(s), m.tlas_case(s)) for s in (1, 4)]")
    subprocess.check_call([sys.executable, "-c", code, ROOT], env=dict(os.environ, PT_PLUGIN=STRESS), timeout=900)


def test_attributes_replaced_or_kept():
    s = scenes.material_zoo()
    upd = PathTracer(s, width=W, height=H)
    ref = PathTracer(s, width=W, height=H)
    built = (ref._bvhScene.bvh_nodes, ref._bvhScene.bvh_tris)
    w1, w2 = deformed(s.vertices, 8, amplitude=0.01), deformed(s.vertices, 9, amplitude=0.01)
    a1 = new_attrs(s.tri_attrs, 1)
    upd.update_geometry(w1, tri_attrs=a1)
    got, gst = render(upd)
    set_arrays(ref, *plugin.refit_cwbvh(built, w1), attrs=a1)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and gst == wst
    set_arrays(ref, *plugin.refit_cwbvh(built, w1), attrs=s.tri_attrs)          # ... and they matter: the old attributes give another frame
    assert not np.array_equal(render(ref)[0].view(np.uint32), want.view(np.uint32))
    upd.update_geometry(w2)                                    # NULL: the attributes of the update before stay
    got, gst = render(upd)
    set_arrays(ref, *plugin.refit_cwbvh(built, w2), attrs=a1)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and gst == wst
    bad = a1.copy()
    bad["materialIndex"][3] = s.materials.shape[0]             # a flat scene indexes the materials with it
    assert upd.lib.PTUpdateGeometry(upd.ctx, 0, 0, 0, w2.ctypes.data, w2.shape[0] // 3, bad.ctypes.data) == abi.PT_ERR_INVALID_ARG
    upd.close()
    ref.close()


def test_ordering_with_passes_in_flight():
    """Passes enqueued before an update see the old geometry, passes after it the new, with no host synchronisation between."""
    import torch
    s = scenes.material_zoo()
    ref = PathTracer(s, width=W, height=H)
    built = (ref._bvhScene.bvh_nodes, ref._bvhScene.bvh_tris)
    states = [None, deformed(s.vertices, 21, amplitude=0.01), deformed(s.vertices, 22, amplitude=0.02)]
    statics = []
    for w in states:
        if w is not None:
            set_arrays(ref, *plugin.refit_cwbvh(built, w))
        statics.append(render(ref, 1)[0])
    ref.close()
    for host in (False, True):
        pt = PathTracer(s, width=W, height=H)
        pt.set_passes_in_flight(12)
        dev = f"cuda:{pt.device}"
        outs = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in states]
        keep = [to_device(pt, w) for w in states[1:]]
        torch.cuda.synchronize()
        p = pt.params(seed=0x51)
        pt.render_pass_to(p, outs[0].data_ptr())
        for k in (1, 2):
            if host:
                w = states[k].copy()
                plugin.check(pt.lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, w.ctypes.data, w.shape[0] // 3, None))
                w[:] = np.nan                                  # the library copied the array before returning
            else:
                pt.update_geometry(keep[k - 1])
            pt.render_pass_to(p, outs[k].data_ptr())
        pt.synchronize()
        torch.cuda.synchronize()
        for k in range(3):
            assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), statics[k].view(np.uint32)), (host, k)
        pt.close()


def test_queries_and_guides_after_update():
    s = scenes.instanced_scene()
    upd = PathTracer(s, width=W, height=H)
    ref = PathTracer(s, width=W, height=H)
    slices = mesh_slices(s)
    t0, n = s.mesh_ranges[1]
    w = deformed(s.vertices[t0 * 3:(t0 + n) * 3], 31, amplitude=0.08)
    upd.update_geometry(w, mesh=1)
    set_arrays(ref, *compose(s, slices, ref._bvhScene.bvh_nodes, ref._bvhScene.bvh_tris, 1, w),
               blas=instance_bounds(ref, s, 1, w, ref._bvhScene.blas_instances))
    rays = np.stack([upd.camera_ray(x, y) for y in range(0, H, 3) for x in range(0, W, 3)])
    h1, s1 = upd.trace_rays(rays, surface=True)
    h2, s2 = ref.trace_rays(rays, surface=True)
    assert (h1.view(np.uint32)[:, 3] != abi.PT_MISS).sum() > rays.shape[0] // 4
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    for pt in (upd, ref):
        pt.render_guides(4)
    for a, b in zip(upd.guides(), ref.guides()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    upd.close()
    ref.close()


def test_animation():
    s = scenes.material_zoo()
    pt = PathTracer(s, width=W, height=H)
    ref = PathTracer(s, width=W, height=H)
    built = (ref._bvhScene.bvh_nodes, ref._bvhScene.bvh_tris)
    for f in range(8):
        w = deformed(s.vertices, 50, amplitude=0.004 * (f + 1))          # the same field, growing
        pt.update_geometry(w)
        got, _ = render(pt, 1, seed0=0x77 + f)
        set_arrays(ref, *plugin.refit_cwbvh(built, w))
        want, _ = render(ref, 1, seed0=0x77 + f)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
    pt.close()
    ref.close()


def test_argument_errors():
    lib = plugin.load_library()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    buf = np.zeros(4096, np.uint8)
    for rc in (lib.PTUpdateGeometry(ctx, 0, 0, 0, buf.ctypes.data, 1, None), lib.PTUpdateGeometryDevice(ctx, 0, 0, 0, buf.ctypes.data, 1, None),
               lib.PTReadGeometry(ctx, buf.ctypes.data, buf.nbytes, buf.ctypes.data, buf.nbytes, None, 0)):
        assert rc == abi.PT_ERR_NO_SCENE
    lib.PTDestroy(ctx)
    v = soup(9, 2)
    flat = PathTracer(soup_scene(v), width=8, height=8)
    p, n = v.ctypes.data, 9
    for fn in (lib.PTUpdateGeometry, lib.PTUpdateGeometryDevice):
        assert fn(None, 0, 0, 0, p, n, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 0, 0, 0, None, n, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 0, 0, 0, p, 0, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 0, 0, 0, p, n - 1, None) == abi.PT_ERR_INVALID_ARG            # count mismatch
        assert fn(flat.ctx, 0, 0, 0, p, n + 1, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 1, 0, 0, p, n, None) == abi.PT_ERR_INVALID_ARG                # offsets that name no BLAS
        assert fn(flat.ctx, 0, 3, 0, p, n, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 0, 0, -1, p, n, None) == abi.PT_ERR_INVALID_ARG
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[5, 2] = bad
        assert lib.PTUpdateGeometry(flat.ctx, 0, 0, 0, w.ctypes.data, n, None) == abi.PT_ERR_INVALID_ARG
    small = np.zeros(16, np.uint8)
    big = np.zeros(1 << 16, np.uint8)
    assert lib.PTReadGeometry(flat.ctx, small.ctypes.data, small.nbytes, big.ctypes.data, big.nbytes, None, 0) == abi.PT_ERR_INVALID_ARG
    assert lib.PTReadGeometry(flat.ctx, big.ctypes.data, big.nbytes, big.ctypes.data, big.nbytes, small.ctypes.data, small.nbytes) == abi.PT_ERR_INVALID_ARG
    assert lib.PTReadGeometry(flat.ctx, None, 0, big.ctypes.data, big.nbytes, None, 0) == abi.PT_ERR_INVALID_ARG
    # nothing above changed the scene
    got = flat.read_geometry()
    assert np.array_equal(got[0], flat._bvhScene.bvh_nodes) and np.array_equal(got[1], flat._bvhScene.bvh_tris)
    flat.close()
    s = scenes.instanced_scene(count=5, detail=4)               # meshes 0, 1, 2, 0, 1 behind the floor
    pt = PathTracer(s, width=8, height=8)
    gi = pt._bvhScene.gpu_instances
    k = next(i for i, inst in enumerate(s.instances) if inst[0] == 1)
    off = [int(gi[k][f]) for f in ("bvhOffset", "triOffset", "triAttributeOffset")]
    t0, n = s.mesh_ranges[1]
    w = np.ascontiguousarray(s.vertices[t0 * 3:(t0 + n) * 3])
    assert lib.PTUpdateGeometry(pt.ctx, *off, w.ctypes.data, n - 1, None) == abi.PT_ERR_INVALID_ARG         # not the BLAS's count
    assert lib.PTUpdateGeometry(pt.ctx, off[0], off[1], off[2] + 1, w.ctypes.data, n, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTUpdateGeometry(pt.ctx, off[0] + 1, off[1], off[2], w.ctypes.data, n, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTUpdateGeometry(pt.ctx, *off, w.ctypes.data, n, None) == abi.PT_OK
    # PTSetScene discards the update state: the scene's own arrays are current again
    pt._bvhScene.PrepareShader(pt.ctx)
    got = pt.read_geometry()
    assert np.array_equal(got[0], pt._bvhScene.bvh_nodes) and np.array_equal(got[1], pt._bvhScene.bvh_tris)
    # two instances that share mesh 1's nodes and records under different attribute offsets are two BLAS keys: refused
    users = [i for i, inst in enumerate(s.instances) if inst[0] == 1]
    assert len(users) == 2
    gi[users[1]]["triAttributeOffset"] = 0                     # mesh 0's records: 576 >= 48, still a valid scene
    pt._bvhScene.PrepareShader(pt.ctx)
    assert lib.PTUpdateGeometry(pt.ctx, *off, w.ctypes.data, n, None) == abi.PT_ERR_INVALID_ARG
    assert b"shares" in lib.PTGetLastError()
    pt.close()
