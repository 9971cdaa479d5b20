"""Shading from the bakes (PTBakeDFG / PTShadeSurfaces / PTShadeCompose / PTShadeBaked / PTShadeBakedFrame, include/ptmi_plugin.h
Part 21) on the MI355X.

The rule is bit-exact and these tests hold it without tolerances: the kernels equal their host twins, the material record equals
the render's own fetch (the albedo guide, the material array), the fused call equals the four-call composition, a frame equals
the query followed by the fused call.  The end-to-end test asserts orderings only."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer, ProbeVolume
import shade_cases as cases

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 48, 32
_EMISSION = (6.0, 5.0, 3.0)
_SPHERE = 4                     # the material index of the box's sphere


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _box():
    """tests/test_gpu_probe.py's box -- a CLOSED Cornell shell, every material of roughness 1, a 1.2 x 1.2 emissive ceiling patch, a
    black sky -- with a polished metal sphere standing in it"""
    sb, mats = scenes.SoupBuilder(), []
    scenes._cornell_shell(sb, mats)
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1), 1, 1, 0)           # front wall z = -1
    mats.append(scenes.pack_material(color=(0.5, 0.5, 0.5, 1.0), roughness=1.0, emission=_EMISSION))      # 3
    mats.append(scenes.pack_material(color=(0.9, 0.9, 0.9, 1.0), roughness=0.0, metallic=1.0))            # 4
    sb.quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0), 1, 1, 0)
    sb.quad((-0.6, 1.98, -0.6), (1.2, 0, 0), (0, 0, 1.2), (0, -1, 0), 1, 1, 3)
    sb.uv_sphere((0.35, 0.8, 0.3), 0.3, 24, 12, _SPHERE)
    verts, attrs = sb.finish()
    return scenes.Scene("shade_box", verts, attrs, np.stack(mats), np.zeros((0, 16), dtype=F), np.zeros(0, dtype=np.uint32),
                        scenes.Camera(eye=(0.0, 1.0, -0.9), target=(0.0, 0.3, 0.2), vfov_deg=60.0),
                        environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0), environment_intensity=0.0)


class Baked:
    """a tracer with its bakes: a probe volume around the camera's view (placed), two reflection probes with boxes, a DFG table"""

    def __init__(self, scene, lo, hi, counts=(2, 2, 2), spp=64):
        self.scene = scene
        self.pt = PathTracer(scene, width=W, height=H, samplesPerPass=1, maxRayBounces=2, schedule=1)
        pt = self.pt
        lo, hi = np.asarray(lo, F), np.asarray(hi, F)
        self.volume = pt.bake_probe_volume(lo, hi, counts, spp=spp, depth_spp=spp, relocate=True)
        mid = (lo + hi) / 2
        pos = np.stack([mid + (hi - lo) * F(0.2), mid - (hi - lo) * F(0.15)]).astype(F)
        half = (hi - lo) * F(0.45)
        self.reflections = pt.capture_reflection_probes(pos, res=8, spp=4, levels=2, boxes=(pos - half, pos + half))
        self.dfg = pt.bake_dfg(16)
        self.params = pt.params(seed=0)

    def frame_rays(self):
        _, rays = self.pt.render_baked(self.params, self.volume, self.reflections, self.dfg, return_rays=True)
        return rays

    def close(self):
        self.pt.close()


@pytest.fixture(scope="module")
def box():
    b = Baked(_box(), (-0.9, 0.1, -0.9), (0.9, 1.9, 0.9))
    yield b
    b.close()


def _scene_box(scene):
    v = scene.vertices[:, :3]
    return v.min(0), v.max(0)


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


def _composition(b, rays, hits, surf, placement=True, boxes=True, reflections=True, dfg=None):
    """PTShadeSurfaces, PTProbeGridIrradiancePlaced, PTReflectionLookup, PTShadeCompose"""
    import torch
    pt, vol, refl = b.pt, b.volume, b.reflections if reflections else None
    n = rays.shape[0]
    _, terms, recv, qr = pt.shade_surfaces(rays, hits, surf, None if refl is None else refl.probe_rows, None if refl is None or not boxes else refl.box_rows)
    v = vol if placement else ProbeVolume(pt, vol.grid, vol.sh, vol.m2, vol.depth, vol.max_distance, None)
    E = v.irradiance(receivers=recv)
    spec = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
    with pt._ordered(rays.device):
        if refl is None:
            plugin.check(pt.lib.PTReflectionLookup(pt.ctx, None, 0, 8, 2, None, None, qr.data_ptr(), n, spec.data_ptr()))
        else:
            plugin.check(pt.lib.PTReflectionLookup(pt.ctx, refl.maps.data_ptr(), refl.maps.shape[0], refl.res, refl.levels, refl.probe_rows.data_ptr(),
                                                   refl.box_rows.data_ptr() if boxes else None, qr.data_ptr(), n, spec.data_ptr()))
    return pt.shade_compose(terms, E, spec, b.dfg if dfg is None else dfg)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the table
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [16, 64])
def test_dfg_kernel_equals_the_twin(box, res):
    got = box.pt.bake_dfg(res)
    assert got.is_cuda and got.shape == (res, res, 2)
    assert (_bits(got) == _bits(plugin.bake_dfg(res))).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. surfaces
# ---------------------------------------------------------------------------------------------------------------------------
def test_material_record_is_the_renders_fetch_textured(zoo):
    """base colour = the albedo guide at one sample per pixel, bit for bit, where the frame's rays hit"""
    pt = zoo.pt
    rays = zoo.frame_rays()
    hits, surf = pt.trace_rays(rays, surface=True)
    mat = pt.shade_surfaces(rays, hits, surf)[0].cpu().numpy()
    pt.render_guides(1, zoo.params)
    albedo, normal_depth = pt.guides()
    hit = hits.cpu().numpy().view(np.uint32)[:, 3] != 0xFFFFFFFF
    assert 0.2 < hit.mean() <= 1.0
    assert (_bits(mat[hit, 0:3]) == _bits(albedo.reshape(-1, 4)[hit, 0:3])).all()
    flags = mat.view(np.uint32)[:, 11]
    assert (flags[hit] == 0).all() and (flags[~hit] == abi.PT_SHADE_MISS).all() and not mat[~hit, 0:10].any()
    words = np.ascontiguousarray(zoo.scene.materials).view(np.float32).reshape(-1, 32)
    seen = np.unique(mat.view(np.uint32)[hit, 10])
    assert (words[seen, 22] >= 0).any()                                  # materials with a base-colour texture are in view
    # the frame's rays are the guides': the hit distance is the depth guide's
    assert (_bits(hits.cpu().numpy()[hit, 0]) == _bits(normal_depth.reshape(-1, 4)[hit, 3])).all()


def test_material_record_is_the_material_array_untextured(box):
    pt = box.pt
    rays = box.frame_rays()
    hits, surf = pt.trace_rays(rays, surface=True)
    mat = pt.shade_surfaces(rays, hits, surf)[0].cpu().numpy()
    idx = surf.cpu().numpy().view(np.uint32)[:, 7]
    assert (mat.view(np.uint32)[:, 10] == idx).all() and set(np.unique(idx)) >= {0, _SPHERE}
    words = np.ascontiguousarray(box.scene.materials).view(np.float32).reshape(-1, 32)[idx]
    assert (_bits(mat[:, 0:3]) == _bits(words[:, 0:3])).all() and (_bits(mat[:, 9]) == _bits(words[:, 3])).all()          # base colour, opacity
    assert (_bits(mat[:, 4:7]) == _bits(words[:, 4:7])).all()                                                             # emission
    assert (_bits(mat[:, 3]) == _bits(words[:, 8])).all()                                                                 # metallic
    assert (_bits(mat[:, 7]) == _bits(np.maximum(words[:, 9], F(0.001)))).all()                                          # roughness (alpha)
    assert (mat[:, 8] == 1).all()


@pytest.mark.parametrize("which", ["box", "zoo", "instanced"])
@pytest.mark.parametrize("probes", ["none", "probes", "boxes"])
def test_terms_equal_the_twin(request, which, probes):
    b = request.getfixturevalue(which)
    pt = b.pt
    rays = b.frame_rays()
    hits, surf = pt.trace_rays(rays, surface=True)
    pr = None if probes == "none" else b.reflections.probe_rows
    bx = b.reflections.box_rows if probes == "boxes" else None
    mat, terms, recv, qr = (x.cpu().numpy() for x in pt.shade_surfaces(rays, hits, surf, pr, bx))
    want = plugin.shade_terms(mat, rays.cpu().numpy(), surf.cpu().numpy(), None if pr is None else pr.cpu().numpy()[:, 0:3],
                              None if bx is None else bx.cpu().numpy())
    for g, w, what in zip((terms, recv, qr), want, ("terms", "receivers", "queries")):
        assert (_bits(g) == _bits(w)).all(), what
    if probes == "boxes":
        chosen = qr.view(np.uint32)[:, 7]
        print(f"[shade] {which}: probe 0 x {(chosen == 0).sum()}, probe 1 x {(chosen == 1).sum()}, none x {(chosen == 0xFFFFFFFF).sum()}")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. compose
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [16, 64])
def test_compose_kernel_equals_the_twin(box, res):
    dfg = plugin.bake_dfg(res)
    T, E, R = cases.compose_rows(res)
    got = box.pt.shade_compose(T, E, R, dfg)
    assert (_bits(got) == _bits(plugin.shade_compose(T, E, R, dfg))).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the fused call
# ---------------------------------------------------------------------------------------------------------------------------
def _list(b, n, seed=5):
    """n rays from the camera's eye into the scene around its view direction; every 7th ends before anything (a miss)"""
    import torch
    rng = np.random.default_rng(seed)
    eye, target = np.asarray(b.scene.camera.eye, np.float64), np.asarray(b.scene.camera.target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    d = fwd + rng.normal(size=(n, 3)) * 0.6
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = eye
    rays[:, 3:6] = d * rng.uniform(0.5, 2.0, (n, 1))             # not of unit length
    rays[:, 6] = np.where(np.arange(n) % 7 == 3, 1e-6, 1e30)
    return torch.from_numpy(rays).to(b.reflections.maps.device)


@pytest.mark.parametrize("which", ["box", "zoo", "instanced"])
@pytest.mark.parametrize("placement,boxes,reflections", [(True, True, True), (False, True, True), (True, False, True), (False, False, False)])
def test_fused_call_is_the_composition(request, which, placement, boxes, reflections):
    b = request.getfixturevalue(which)
    pt = b.pt
    rays = _list(b, 1500)
    hits, surf = pt.trace_rays(rays, surface=True)
    got = pt.shade_baked(rays, hits, surf, b.volume, b.reflections if reflections else None, b.dfg, placement=placement, boxes=boxes)
    want = _composition(b, rays, hits, surf, placement, boxes, reflections)
    assert (_bits(got) == _bits(want)).all()
    miss = hits.cpu().numpy().view(np.uint32)[:, 3] == 0xFFFFFFFF
    g = got.cpu().numpy()
    assert miss.sum() >= 1500 // 7 and not g[miss].any() and (g[~miss, 3] == 1).all() and np.isfinite(g).all()
    if which == "box" and placement and boxes:
        st = b.volume.placement.cpu().numpy()
        print(f"[shade] box volume: {np.count_nonzero(st[:, 0:3].any(axis=1))} of 8 probes moved, {np.count_nonzero(st.view(np.uint32)[:, 3])} inside")


@pytest.mark.parametrize("n", [1, 2, 65, 4097])
def test_fused_call_list_lengths(box, n):
    import torch
    pt = box.pt
    rays = _list(box, n, seed=n)
    hits, surf = pt.trace_rays(rays, surface=True)
    s, keep = pt._shade_inputs(box.volume, box.reflections, box.dfg)
    out = torch.full((n + 3, 4), -7.0, dtype=torch.float32, device=rays.device)
    with pt._ordered(rays.device):
        plugin.check(pt.lib.PTShadeBaked(pt.ctx, C.byref(s), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr()))
    assert (out[n:].cpu().numpy() == -7.0).all()                                # nothing past count
    assert (_bits(out[:n]) == _bits(_composition(box, rays, hits, surf))).all()
    before = out.clone()
    with pt._ordered(rays.device):
        plugin.check(pt.lib.PTShadeBaked(pt.ctx, C.byref(s), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), 0, out.data_ptr()))     # count 0 launches nothing
    assert (_bits(out) == _bits(before)).all()
    del keep


def test_calls_need_a_scene_and_refuse_bad_arguments(box):
    import torch
    pt = box.pt
    lib = pt.lib
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(pt.device, C.byref(ctx)))
    try:
        rays = _list(box, 4)
        hits, surf = pt.trace_rays(rays, surface=True)
        s, keep = pt._shade_inputs(box.volume, box.reflections, box.dfg)
        out = torch.zeros((W * H, 4), dtype=torch.float32, device=rays.device)
        torch.cuda.synchronize()
        assert lib.PTShadeSurfaces(ctx, rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), 4, None, None, 0, out.data_ptr(), None, None, None) == abi.PT_ERR_NO_SCENE
        assert lib.PTShadeBaked(ctx, C.byref(s), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), 4, out.data_ptr()) == abi.PT_ERR_NO_SCENE
        assert lib.PTShadeBakedFrame(ctx, C.byref(box.params), C.byref(s), out.data_ptr(), None) == abi.PT_ERR_NO_SCENE
        # the table and the compose step need none
        dfg = torch.zeros((16, 16, 2), dtype=torch.float32, device=rays.device)
        torch.cuda.synchronize()
        plugin.check(lib.PTBakeDFG(ctx, 16, dfg.data_ptr()))
        torch.cuda.synchronize()
        assert (_bits(dfg) == _bits(box.dfg)).all()
        del keep
    finally:
        lib.PTDestroy(ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a frame
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["box", "zoo", "instanced"])
def test_frame_is_the_query_and_the_fused_call(request, which):
    b = request.getfixturevalue(which)
    pt = b.pt
    frame, rays = pt.render_baked(b.params, b.volume, b.reflections, b.dfg, return_rays=True)
    assert frame.shape == (H, W, 4) and rays.shape == (W * H, 8)
    hits, surf = pt.trace_rays(rays, surface=True)
    want = pt.shade_baked(rays, hits, surf, b.volume, b.reflections, b.dfg)
    assert (_bits(frame.reshape(-1, 4)) == _bits(want)).all()
    # without the rays coming back, and with the context's own table (32 x 32, baked once)
    assert (_bits(pt.render_baked(b.params, b.volume, b.reflections, b.dfg)) == _bits(frame)).all()
    own = pt.render_baked(b.params, b.volume, b.reflections)
    assert (_bits(pt._dfg) == _bits(plugin.bake_dfg(32))).all()
    assert (_bits(own.reshape(-1, 4)) == _bits(_composition(b, rays, hits, surf, dfg=pt._dfg))).all()
    # the rays are the guides': every hit distance is the depth guide's
    pt.render_guides(1, b.params)
    _, normal_depth = pt.guides()
    h = hits.cpu().numpy()
    hit = h.view(np.uint32)[:, 3] != 0xFFFFFFFF
    assert hit.any() and (_bits(h[hit, 0]) == _bits(normal_depth.reshape(-1, 4)[hit, 3])).all()
    assert (normal_depth.reshape(-1, 4)[~hit, 3] == 0).all()


def test_frame_sees_updated_geometry():
    """a second frame after update_geometry shows the new surface: a tracer of its own, the box squeezed to 0.8 of its height"""
    b = Baked(_box(), (-0.9, 0.1, -0.9), (0.9, 1.5, 0.9))
    try:
        pt = b.pt
        before, rays = pt.render_baked(b.params, b.volume, b.reflections, b.dfg, return_rays=True)
        w = b.scene.vertices.copy()
        w[:, 1] *= F(0.8)
        pt.update_geometry(w)
        after = pt.render_baked(b.params, b.volume, b.reflections, b.dfg)
        hits, surf = pt.trace_rays(rays, surface=True)
        assert surf.cpu().numpy()[:, 1].max() <= 1.6 + 1e-5                      # the ceiling came down
        assert (_bits(after.reshape(-1, 4)) == _bits(pt.shade_baked(rays, hits, surf, b.volume, b.reflections, b.dfg))).all()
        assert (_bits(after) != _bits(before)).any()
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_in_the_box():
    """orderings only: the floor under the patch against the floor's far corner; on the polished sphere, the pixel that reflects
    the ceiling patch most directly against the one that reflects the floor"""
    pt = PathTracer(_box(), width=W, height=H, samplesPerPass=1, maxRayBounces=3, schedule=1)
    try:
        volume = pt.bake_probe_volume((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (3, 3, 3), spp=256, depth_spp=128)
        pos = np.array([(-0.3, 1.2, -0.2), (0.35, 1.45, 0.3)], F)
        refl = pt.capture_reflection_probes(pos, res=8, spp=32, levels=2)
        p = pt.params(seed=0)
        frame, rays = pt.render_baked(p, volume, refl, return_rays=True)
        hits, surf = pt.trace_rays(rays, surface=True)
        mat, _, recv, qr = (x.cpu().numpy() for x in pt.shade_surfaces(rays, hits, surf, refl.probe_rows))
        lum = frame.reshape(-1, 4).cpu().numpy()[:, 0:3] @ np.array([0.299, 0.587, 0.114])
        idx = mat.view(np.uint32)[:, 10]
        P, N = recv[:, 0:3], recv[:, 4:7]
        floor = (idx == 0) & (N[:, 1] > 0.99) & (P[:, 1] < 1e-3)
        assert floor.sum() > 50
        k = np.flatnonzero(floor)
        under = k[np.argmin(np.abs(P[k, 0]) + np.abs(P[k, 2]))]
        corner = k[np.argmax(np.abs(P[k, 0]) + P[k, 2])]
        print(f"[shade] floor under the patch {lum[under]:.4f} at {P[under]}, far corner {lum[corner]:.4f} at {P[corner]}")
        assert lum[under] > lum[corner] > 0
        k = np.flatnonzero(idx == _SPHERE)
        assert k.size > 20
        up, down = k[np.argmax(qr[k, 5])], k[np.argmin(qr[k, 5])]              # the reflection direction's y
        print(f"[shade] sphere towards the patch {lum[up]:.4f} (R.y {qr[up, 5]:.2f}), towards the floor {lum[down]:.4f} (R.y {qr[down, 5]:.2f})")
        assert qr[up, 5] > 0.5 and qr[down, 5] < -0.2 and lum[up] > lum[down] > 0
    finally:
        pt.close()
