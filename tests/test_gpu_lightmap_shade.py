"""First hits shaded from baked lightmaps (PTBindLightmaps / PTLightmapLookup / PTShadeLightmapped / PTShadeLightmappedFrame,
include/ptmi_plugin.h Part 22) on the MI355X.

The rule is bit-exact and these tests hold it without tolerances: the lookup kernel equals the host twin, the fused call equals
the six-step composition and, with nothing bound, PTShadeBaked; a frame equals the query followed by the fused call.  The scenes
and their bakes are tests/test_gpu_shade_baked.py's.  The end-to-end test asserts orderings only."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer, ProbeVolume
import lightmap_lookup_cases as cases
from test_gpu_shade_baked import Baked, H, W, _bits, _box, _list, _scene_box

pytestmark = pytest.mark.gpu

F = np.float32
NONE = abi.PT_LIGHTMAP_NONE


@pytest.fixture(scope="module")
def box():
    b = Baked(_box(), (-0.9, 0.1, -0.9), (0.9, 1.9, 0.9))
    yield b
    b.close()


@pytest.fixture(scope="module")
def zoo():
    s = scenes.material_zoo()
    lo, hi = _scene_box(s)
    b = Baked(s, lo + (hi - lo) * F(0.1), hi - (hi - lo) * F(0.1))
    yield b
    b.close()


@pytest.fixture(scope="module")
def instanced():
    s = scenes.instanced_scene()
    eye, target = np.asarray(s.camera.eye, F), np.asarray(s.camera.target, F)
    r = F(0.6) * np.linalg.norm(target - eye).astype(F)
    b = Baked(s, target - r, target + r)
    yield b
    b.close()


def _attrs(pt):
    return pt._bvhScene.tri_attrs


def _materials(pt):
    return pt._bvhScene.materials.reshape(-1, 32).shape[0]


def _meshes(b):
    """the meshes a whole-scene table binds: None on a flat scene"""
    return [None] if b.pt._bvhScene.gpu_instances is None else sorted({rec[0] for rec in b.scene.instances})


def _host(bindings):
    """the dicts the twin takes, from lightmap_binding's entries"""
    return [{"image": e["image"].cpu().numpy(), "first_prim": e["record"].firstPrim, "prim_count": e["record"].primCount, "instance": e["instance"],
             "uvs": None if e["uvs"] is None else e["uvs"].cpu().numpy(), "two_sided": e["two_sided"]} for e in bindings]


def _span_binding(pt, d):
    """a lightmap_binding entry for an arbitrary span: from one of tests/lightmap_lookup_cases.py's dicts"""
    import torch
    dev = torch.device(f"cuda:{pt.device}")
    img = torch.from_numpy(np.ascontiguousarray(d["image"], F)).to(dev)
    uvs = None if d["uvs"] is None else torch.from_numpy(np.ascontiguousarray(d["uvs"], F)).to(dev)
    r = abi.PTLightmapBinding()
    r.firstPrim, r.primCount = d["first_prim"], d["prim_count"]
    r.instance = NONE if d["instance"] is None else d["instance"]
    r.flags = abi.PT_LIGHTMAP_TWO_SIDED if d["two_sided"] else 0
    r.height, r.width = img.shape[0], img.shape[1]
    r.dImage, r.dUvs = img.data_ptr(), None if uvs is None else uvs.data_ptr()
    return {"record": r, "image": img, "uvs": uvs, "mesh": None, "instance": d["instance"], "two_sided": d["two_sided"]}


def _whole(b, kind, size, uvs=False, two_sided=True, seed=0):
    """every mesh of the scene bound to a synthetic image of its own"""
    pt, out = b.pt, []
    for k, mesh in enumerate(_meshes(b)):
        count = pt._bvhScene.blas_spans[0 if mesh is None else mesh][3]
        u = np.random.default_rng(40 + k).uniform(-0.05, 1.05, (count, 6)).astype(F) if uvs else None
        out.append(pt.lightmap_binding(cases.image(kind, *size, seed=seed + k, poison=True), mesh=mesh, uvs=u, two_sided=two_sided))
    return out


def _hits(b, n=1500, seed=5):
    rays = _list(b, n, seed)
    hits, surf = b.pt.trace_rays(rays, surface=True)
    return rays, hits, surf


def _check_lookup(b, bindings, rays, hits, surf):
    pt = b.pt
    pt.bind_lightmaps(bindings)
    got, which = pt.lightmap_lookup(rays, hits, surf)
    want, want_which = plugin.lightmap_lookup(_host(bindings), _attrs(pt), _materials(pt), rays.cpu().numpy(), hits.cpu().numpy(), surf.cpu().numpy())
    which = which.cpu().numpy().view(np.uint32)
    assert (which == want_which).all()
    assert (_bits(got) == _bits(want)).all()
    assert np.isfinite(got.cpu().numpy()).all()                                  # the invalid texels' rgb is NaN
    return got.cpu().numpy(), which


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the lookup against the twin
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["box", "zoo", "instanced"])
@pytest.mark.parametrize("kind,size,uvs", [("full", (8, 8), False), ("checker", (24, 8), False), ("w-values", (24, 8), True), ("single", (2, 2), True),
                                           ("full", (1, 1), False), ("empty", (8, 8), False)])
def test_lookup_equals_the_twin_whole_scene(request, which, kind, size, uvs):
    b = request.getfixturevalue(which)
    rays, hits, surf = _hits(b)
    try:
        got, found = _check_lookup(b, _whole(b, kind, size, uvs), rays, hits, surf)
        miss = hits.cpu().numpy().view(np.uint32)[:, 3] == NONE
        assert miss.sum() >= 1500 // 7 and (found[miss] == NONE).all()
        if kind == "empty":
            assert (found == NONE).all()
        else:
            assert (found != NONE).sum() > 30, (found != NONE).sum()             # (the instanced scene's floor tiles its UVs: most hits fall outside)
    finally:
        b.pt.bind_lightmaps([])


def test_lookup_one_mesh_and_two_instances_of_one_mesh(instanced):
    b, pt = instanced, instanced.pt
    rays, hits, surf = _hits(b, 3000)
    inst = surf.cpu().numpy().view(np.uint32)[:, 10]
    hit = hits.cpu().numpy().view(np.uint32)[:, 3] != NONE
    seen = np.bincount(inst[hit & (inst != NONE)], minlength=len(b.scene.instances))
    by_mesh = {}
    for i, rec in enumerate(b.scene.instances):
        if seen[i]:
            by_mesh.setdefault(rec[0], []).append(i)
    mesh, users = max(by_mesh.items(), key=lambda kv: len(kv[1]))
    assert len(users) >= 2, by_mesh
    try:
        # one mesh, whichever instance
        got, found = _check_lookup(b, [pt.lightmap_binding(cases.image("full", 8, 8, constant=(1, 2, 3)), mesh=mesh, two_sided=True)], rays, hits, surf)
        meshes = np.array([rec[0] for rec in b.scene.instances])
        on_mesh = hit & (inst != NONE) & (meshes[np.minimum(inst, len(meshes) - 1)] == mesh)
        assert ((found != NONE) == on_mesh).all() and on_mesh.sum() > 20
        # two instances of it with different images; its other instances have none
        two = [pt.lightmap_binding(cases.image("full", 8, 8, constant=(1, 1, 1)), mesh=mesh, instance=users[0], two_sided=True),
               pt.lightmap_binding(cases.image("full", 24, 8, constant=(5, 5, 5)), mesh=mesh, instance=users[1], two_sided=True)]
        got, found = _check_lookup(b, two, rays, hits, surf)
        assert ((found == 0) == (on_mesh & (inst == users[0]))).all() and ((found == 1) == (on_mesh & (inst == users[1]))).all()
        assert (got[found == 0, 0] == 1).all() and (got[found == 1, 0] == 5).all() and (found == 0).any() and (found == 1).any()
    finally:
        pt.bind_lightmaps([])


@pytest.mark.parametrize("name", sorted(cases.tables(cases.tri_attrs())))
def test_lookup_equals_the_twin_on_the_case_tables(box, instanced, name):
    """the CPU test's hit list and binding tables (spans of the scene's first 80 primitives, explicit UVs with the edge cases) on
    the box; the tables that name instances on the instanced scene -- the flat box refuses them"""
    import torch
    attrs = cases.tri_attrs()
    table = cases.tables(attrs, poison=True)[name]
    for d in table:                                       # the records' UVs are the scene's on the device: give the generator's explicitly
        if d["uvs"] is None:
            d["uvs"] = cases.uvs_of(attrs, d["first_prim"], d["prim_count"])
    b = box
    if any(d["instance"] is not None for d in table):
        with pytest.raises(plugin.PluginError, match="instance"):
            box.pt.bind_lightmaps([_span_binding(box.pt, d) for d in table])
        b = instanced
    pt = b.pt
    rays, hits, surf = (torch.from_numpy(a).to(b.dfg.device) for a in cases.entries())
    assert _attrs(pt).shape[0] >= cases.PRIMS and (b is box or len(b.scene.instances) >= 3)
    try:
        got, found = _check_lookup(b, [_span_binding(pt, d) for d in table], rays, hits, surf)
        if name == "8x8-full":
            assert list(found[0:16] == NONE) == [True, True, False, False, True, False, False, True] * 2
        if name != "none" and "empty" not in name:
            assert (found != NONE).sum() > 10
    finally:
        pt.bind_lightmaps([])


@pytest.mark.parametrize("n", [1, 2, 65, 4097])
def test_lookup_list_lengths(box, n):
    import torch
    pt = box.pt
    rays, hits, surf = _hits(box, n, seed=n)
    bindings = _whole(box, "checker", (24, 8))
    try:
        pt.bind_lightmaps(bindings)
        out = torch.full((n + 3, 4), -7.0, dtype=torch.float32, device=rays.device)
        which = torch.full((n + 3,), 77, dtype=torch.int32, device=rays.device)
        with pt._ordered(rays.device):
            plugin.check(pt.lib.PTLightmapLookup(pt.ctx, rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr(), which.data_ptr()))
        assert (out[n:].cpu().numpy() == -7.0).all() and (which[n:].cpu().numpy() == 77).all()      # nothing past count
        want, want_which = plugin.lightmap_lookup(_host(bindings), _attrs(pt), _materials(pt), rays.cpu().numpy(), hits.cpu().numpy(), surf.cpu().numpy())
        assert (_bits(out[:n]) == _bits(want)).all() and (which[:n].cpu().numpy().view(np.uint32) == want_which).all()
        before = out.clone()
        with pt._ordered(rays.device):
            plugin.check(pt.lib.PTLightmapLookup(pt.ctx, rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr(), None))      # no binding words
            plugin.check(pt.lib.PTLightmapLookup(pt.ctx, rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), 0, out.data_ptr(), None))      # count 0 launches nothing
        assert (_bits(out) == _bits(before)).all()
    finally:
        pt.bind_lightmaps([])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fused call
# ---------------------------------------------------------------------------------------------------------------------------
def _composition(b, rays, hits, surf, placement=True, boxes=True, reflections=True):
    """PTShadeSurfaces, PTProbeGridIrradiance[Placed], PTLightmapLookup, the lightmap's irradiance where one was found else the
    volume's, PTReflectionLookup, PTShadeCompose"""
    import torch
    pt, vol, refl = b.pt, b.volume, b.reflections if reflections else None
    n = rays.shape[0]
    _, terms, recv, qr = pt.shade_surfaces(rays, hits, surf, None if refl is None else refl.probe_rows, None if refl is None or not boxes else refl.box_rows)
    v = vol if placement else ProbeVolume(pt, vol.grid, vol.sh, vol.m2, vol.depth, vol.max_distance, None)
    E = v.irradiance(receivers=recv)
    L, which = pt.lightmap_lookup(rays, hits, surf)
    E = torch.where((which != -1)[:, None], L, E)
    spec = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
    with pt._ordered(rays.device):
        if refl is None:
            plugin.check(pt.lib.PTReflectionLookup(pt.ctx, None, 0, 8, 2, None, None, qr.data_ptr(), n, spec.data_ptr()))
        else:
            plugin.check(pt.lib.PTReflectionLookup(pt.ctx, refl.maps.data_ptr(), refl.maps.shape[0], refl.res, refl.levels, refl.probe_rows.data_ptr(),
                                                   refl.box_rows.data_ptr() if boxes else None, qr.data_ptr(), n, spec.data_ptr()))
    return pt.shade_compose(terms, E, spec, b.dfg), which


def _half(b):
    """the first half of every mesh's primitives bound to a checker image: waves with lanes of both kinds; every other mesh with
    UVs of its own"""
    out = []
    for k, mesh in enumerate(_meshes(b)):
        count = b.pt._bvhScene.blas_spans[0 if mesh is None else mesh][3]
        u = np.random.default_rng(60 + k).uniform(-0.05, 1.05, (count, 6)).astype(F) if k % 2 else None
        e = b.pt.lightmap_binding(cases.image("checker", 24, 8, seed=70 + k, poison=True), mesh=mesh, uvs=u, two_sided=k % 2 == 0)
        e["record"].primCount = max(e["record"].primCount // 2, 1)
        out.append(e)
    return out


@pytest.mark.parametrize("which", ["box", "zoo", "instanced"])
@pytest.mark.parametrize("placement,boxes,reflections", [(True, True, True), (False, True, True), (True, False, True), (False, False, False)])
def test_fused_call_is_the_composition(request, which, placement, boxes, reflections):
    b = request.getfixturevalue(which)
    pt = b.pt
    rays, hits, surf = _hits(b)
    try:
        for bindings in (_whole(b, "w-values", (24, 8)), _half(b)):
            pt.bind_lightmaps(bindings)
            got = pt.shade_lightmapped(rays, hits, surf, b.volume, b.reflections if reflections else None, b.dfg, placement=placement, boxes=boxes)
            want, found = _composition(b, rays, hits, surf, placement, boxes, reflections)
            assert (_bits(got) == _bits(want)).all()
            found = found.cpu().numpy() != -1
            assert 30 < found.sum() < 1500 - 1500 // 7, found.sum()
            miss = hits.cpu().numpy().view(np.uint32)[:, 3] == NONE
            g = got.cpu().numpy()
            assert not g[miss].any() and (g[~miss, 3] == 1).all() and np.isfinite(g).all()
    finally:
        pt.bind_lightmaps([])


@pytest.mark.parametrize("which", ["box", "zoo", "instanced"])
def test_nothing_bound_is_the_baked_call_and_outside_a_binding_too(request, which):
    b = request.getfixturevalue(which)
    pt = b.pt
    rays, hits, surf = _hits(b, 2000, seed=9)
    baked = pt.shade_baked(rays, hits, surf, b.volume, b.reflections, b.dfg)
    assert pt.lightmaps == []
    assert (_bits(pt.shade_lightmapped(rays, hits, surf, b.volume, b.reflections, b.dfg)) == _bits(baked)).all()
    try:
        # half of the primitives bound: the entries outside the binding keep PTShadeBaked's bits, entry for entry
        pt.bind_lightmaps(_half(b))
        assert len(pt.lightmaps) == len(_meshes(b))
        got = pt.shade_lightmapped(rays, hits, surf, b.volume, b.reflections, b.dfg)
        found = pt.lightmap_lookup(rays, hits, surf)[1].cpu().numpy() != -1
        same = (_bits(got) == _bits(baked)).all(axis=1)
        assert same[~found].all() and found.sum() > 30 and (~same[found]).sum() > found.sum() // 2, found.sum()
    finally:
        pt.bind_lightmaps([])
    # ... and again after the table was unbound
    assert pt.lightmaps == []
    assert (_bits(pt.shade_lightmapped(rays, hits, surf, b.volume, b.reflections, b.dfg)) == _bits(baked)).all()
    assert (pt.lightmap_lookup(rays, hits, surf)[1].cpu().numpy() == -1).all()


@pytest.mark.parametrize("n", [1, 2, 65, 4097])
def test_fused_call_list_lengths(box, n):
    import torch
    pt = box.pt
    rays, hits, surf = _hits(box, n, seed=n)
    s, keep = pt._shade_inputs(box.volume, box.reflections, box.dfg)
    try:
        pt.bind_lightmaps(_half(box))
        out = torch.full((n + 3, 4), -7.0, dtype=torch.float32, device=rays.device)
        with pt._ordered(rays.device):
            plugin.check(pt.lib.PTShadeLightmapped(pt.ctx, C.byref(s), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr()))
        assert (out[n:].cpu().numpy() == -7.0).all()                                # nothing past count
        assert (_bits(out[:n]) == _bits(_composition(box, rays, hits, surf)[0])).all()
    finally:
        pt.bind_lightmaps([])
    del keep


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a frame
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["box", "zoo", "instanced"])
def test_frame_is_the_query_and_the_fused_call(request, which):
    b = request.getfixturevalue(which)
    pt = b.pt
    try:
        pt.bind_lightmaps(_half(b))
        frame, rays = pt.render_lightmapped(b.params, b.volume, b.reflections, b.dfg, return_rays=True)
        assert frame.shape == (H, W, 4) and rays.shape == (W * H, 8)
        hits, surf = pt.trace_rays(rays, surface=True)
        want = pt.shade_lightmapped(rays, hits, surf, b.volume, b.reflections, b.dfg)
        assert (_bits(frame.reshape(-1, 4)) == _bits(want)).all()
        assert (_bits(pt.render_lightmapped(b.params, b.volume, b.reflections, b.dfg)) == _bits(frame)).all()      # without the rays coming back
        assert (_bits(frame) != _bits(pt.render_baked(b.params, b.volume, b.reflections, b.dfg))).any()
        assert (_bits(rays) == _bits(b.frame_rays())).all()                         # the same ray kernel
    finally:
        pt.bind_lightmaps([])


def test_frame_keeps_the_table_across_update_geometry_and_loses_it_at_set_scene():
    """a tracer of its own: the box squeezed to 0.8 of its height with the table still bound; then PTSetScene again"""
    b = Baked(_box(), (-0.9, 0.1, -0.9), (0.9, 1.5, 0.9))
    try:
        pt = b.pt
        pt.bind_lightmaps(_half(b))
        before, rays = pt.render_lightmapped(b.params, b.volume, b.reflections, b.dfg, return_rays=True)
        w = b.scene.vertices.copy()
        w[:, 1] *= F(0.8)
        pt.update_geometry(w)
        after = pt.render_lightmapped(b.params, b.volume, b.reflections, b.dfg)
        hits, surf = pt.trace_rays(rays, surface=True)
        assert surf.cpu().numpy()[:, 1].max() <= 1.6 + 1e-5                      # the ceiling came down
        assert (_bits(after.reshape(-1, 4)) == _bits(pt.shade_lightmapped(rays, hits, surf, b.volume, b.reflections, b.dfg))).all()
        assert (_bits(after) != _bits(before)).any()
        assert (pt.lightmap_lookup(rays, hits, surf)[1].cpu().numpy() != -1).sum() > 100           # the table is still bound
        assert (_bits(after) != _bits(pt.render_baked(b.params, b.volume, b.reflections, b.dfg))).any()
        # PTSetScene unbinds: the spans named the old scene
        pt._bvhScene.PrepareShader(pt.ctx)
        again = pt.render_lightmapped(b.params, b.volume, b.reflections, b.dfg)
        assert (_bits(again) == _bits(pt.render_baked(b.params, b.volume, b.reflections, b.dfg))).all()
        hits, surf = pt.trace_rays(rays, surface=True)
        assert (pt.lightmap_lookup(rays, hits, surf)[1].cpu().numpy() == -1).all()
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_bind_refusals_leave_the_old_table_bound(box, instanced):
    import torch
    for b in (box, instanced):
        pt, lib = b.pt, b.pt.lib
        rays, hits, surf = _hits(b, 600, seed=11)
        flat = pt._bvhScene.gpu_instances is None
        prims = _attrs(pt).shape[0]
        try:
            pt.bind_lightmaps(_whole(b, "full", (8, 8)))
            before = pt.lightmap_lookup(rays, hits, surf)
            assert (before[1].cpu().numpy() != -1).sum() > 20
            img = torch.zeros((8, 8, 4), dtype=torch.float32, device=rays.device)
            a = img.data_ptr()

            def record(**over):
                t = (abi.PTLightmapBinding * 1)()
                r = t[0]
                r.firstPrim, r.primCount, r.instance, r.flags, r.width, r.height, r.dImage, r.dUvs = 0, prims, NONE, 0, 8, 8, a, None
                for k, v in over.items():
                    if k == "reserved":
                        r.reserved[0] = v
                    else:
                        setattr(r, k, v)
                return t

            bad = [{"dImage": None}, {"dImage": a + 4}, {"dUvs": a + 4}, {"width": 0}, {"width": 8193}, {"height": 0}, {"height": 8193}, {"primCount": 0},
                   {"firstPrim": 1}, {"firstPrim": prims, "primCount": 1}, {"flags": 2}, {"flags": 0x80000001}, {"reserved": 7},
                   {"instance": 0 if flat else len(b.scene.instances)}]
            torch.cuda.synchronize()
            for over in bad:
                assert lib.PTBindLightmaps(pt.ctx, record(**over), 1) == abi.PT_ERR_INVALID_ARG, over
                assert b"PTBindLightmaps" in lib.PTGetLastError()
            assert lib.PTBindLightmaps(pt.ctx, None, 1) == abi.PT_ERR_INVALID_ARG
            assert lib.PTBindLightmaps(pt.ctx, (abi.PTLightmapBinding * 65)(), 65) == abi.PT_ERR_INVALID_ARG
            if not flat:
                assert lib.PTBindLightmaps(pt.ctx, record(instance=len(b.scene.instances) - 1), 1) == abi.PT_OK
                pt.bind_lightmaps(pt.lightmaps)
            # every refused call left the old table in force
            after = pt.lightmap_lookup(rays, hits, surf)
            assert (_bits(after[0]) == _bits(before[0])).all() and (after[1] == before[1]).all()
        finally:
            pt.bind_lightmaps([])


def test_calls_need_a_scene(box):
    import torch
    pt, lib = box.pt, box.pt.lib
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(pt.device, C.byref(ctx)))
    try:
        rays, hits, surf = _hits(box, 4)
        s, keep = pt._shade_inputs(box.volume, box.reflections, box.dfg)
        out = torch.zeros((W * H, 4), dtype=torch.float32, device=rays.device)
        t = (abi.PTLightmapBinding * 1)()
        t[0].primCount, t[0].instance, t[0].width, t[0].height, t[0].dImage = 1, NONE, 8, 8, out.data_ptr()
        torch.cuda.synchronize()
        assert lib.PTBindLightmaps(ctx, t, 1) == abi.PT_ERR_NO_SCENE
        assert lib.PTBindLightmaps(ctx, None, 0) == abi.PT_ERR_NO_SCENE
        assert lib.PTLightmapLookup(ctx, rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), 4, out.data_ptr(), None) == abi.PT_ERR_NO_SCENE
        assert lib.PTShadeLightmapped(ctx, C.byref(s), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), 4, out.data_ptr()) == abi.PT_ERR_NO_SCENE
        assert lib.PTShadeLightmappedFrame(ctx, C.byref(box.params), C.byref(s), out.data_ptr(), None) == abi.PT_ERR_NO_SCENE
        del keep
    finally:
        lib.PTDestroy(ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_in_the_box():
    """orderings only: the box's lightmap over its own UVs (every quad covers the unit square and the floor, the first one, owns the
    texels), bound to the floor's two primitives; the floor under the patch against its far corner, and against render_baked"""
    pt = PathTracer(_box(), width=W, height=H, samplesPerPass=1, maxRayBounces=3, schedule=1)
    try:
        volume = pt.bake_probe_volume((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (3, 3, 3), spp=256, depth_spp=128)
        image = pt.bake_lightmap(32, 32, spp=64, as_tensor=True)
        w = image[..., 3].cpu().numpy()
        assert (w == 1).all()                                                   # the floor covers the unit square
        entry = pt.lightmap_binding(image)
        entry["record"].primCount = 2                                            # the floor
        pt.bind_lightmaps([entry])
        p = pt.params(seed=0)
        frame, rays = pt.render_lightmapped(p, volume, return_rays=True)
        baked = pt.render_baked(p, volume)
        hits, surf = pt.trace_rays(rays, surface=True)
        _, found = pt.lightmap_lookup(rays, hits, surf)
        found = found.cpu().numpy() != -1
        prim = hits.cpu().numpy().view(np.uint32)[:, 3]
        assert (found == (prim < 2)).all() and found.sum() > 50
        lum = frame.reshape(-1, 4).cpu().numpy()[:, 0:3] @ np.array([0.299, 0.587, 0.114])
        lum_baked = baked.reshape(-1, 4).cpu().numpy()[:, 0:3] @ np.array([0.299, 0.587, 0.114])
        P = surf.cpu().numpy()[:, 0:3]
        k = np.flatnonzero(found)
        under = k[np.argmin(np.abs(P[k, 0]) + np.abs(P[k, 2]))]
        corner = k[np.argmax(np.abs(P[k, 0]) + P[k, 2])]
        print(f"[lightmap] floor under the patch {lum[under]:.4f} (volume {lum_baked[under]:.4f}) at {P[under]}, far corner {lum[corner]:.4f} "
              f"(volume {lum_baked[corner]:.4f}) at {P[corner]}")
        assert lum[under] > lum[corner] > 0
        assert lum[under] != lum_baked[under]
        assert (_bits(frame.reshape(-1, 4)[~found]) == _bits(baked.reshape(-1, 4)[~found])).all()
    finally:
        pt.close()
