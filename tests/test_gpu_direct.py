"""Direct light at first hits (PTDirectRays / PTDirectAccumulate / PTDirectLight / PTShadeMixed / PTShadeMixedFrame,
include/ptmi_plugin.h Part 24) on the MI355X.

The rule is bit-exact and these tests hold it without tolerances: the kernels equal their host twins, the fused call equals the
four-call composition, the mixed call equals the lightmapped one plus the direct light, a frame equals the query followed by the
mixed call; shadows are exact zeros and exact bits; updates of lights and geometry are seen.  The jitter test asserts orderings;
the one comparison with a tolerance is the float64 formula, within the bound tests/test_direct.py established."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
from test_gpu_shade_baked import Baked, _box, _list, _bits
import direct_cases as cases
import direct_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 48, 32
MISS = 0xFFFFFFFF


def _scene_box(scene):
    v = scene.vertices[:, :3]
    return v.min(0), v.max(0)


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


def _composition(pt, rays, hits, surf, **kw):
    """PTShadeSurfaces, PTDirectRays, PTTraceRays(ANY_HIT), PTDirectAccumulate"""
    _, terms, recv, _ = pt.shade_surfaces(rays, hits, surf)
    pair_rays, contrib = pt.direct_rays(rays, terms, recv, **kw)
    pairs = pt.direct_pair_count(kw.get("strata", 1))
    assert pair_rays.shape[0] == rays.shape[0] * pairs
    pair_hits = pt.trace_rays(pair_rays, any_hit=True) if pair_rays.shape[0] else pair_rays[:, 0:4]
    return pt.direct_accumulate(terms, contrib, pair_hits, pairs)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the pairs' rays and the sum against the twins
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["zoo", "instanced"])
@pytest.mark.parametrize("strata,centered", [(1, True), (1, False), (3, True), (3, False)])
def test_rays_and_accumulate_equal_the_twins(request, which, strata, centered):
    b = request.getfixturevalue(which)
    pt = b.pt
    rays = _list(b, 1500)
    hits, surf = pt.trace_rays(rays, surface=True)
    _, terms, recv, _ = pt.shade_surfaces(rays, hits, surf)
    kw = dict(strata=strata, seed=41, centered=centered, min_alpha=0.05)
    pair_rays, contrib = pt.direct_rays(rays, terms, recv, **kw)
    lights = pt._bvhScene.lights                                        # read from the scene object
    assert pt.direct_pair_count(strata) == plugin.direct_pair_count(lights, strata) == pair_rays.shape[0] // 1500 > 0
    want_rays, want_c = plugin.direct_rays(lights, rays.cpu().numpy(), terms.cpu().numpy(), recv.cpu().numpy(), **kw)
    assert (_bits(pair_rays) == _bits(want_rays)).all() and (_bits(contrib) == _bits(want_c)).all()
    counting = want_rays[:, 6] > 0
    assert 0.05 < counting.mean() < 1.0
    pair_hits = pt.trace_rays(pair_rays, any_hit=True)
    pairs = pt.direct_pair_count(strata)
    got = pt.direct_accumulate(terms, contrib, pair_hits, pairs)
    want = plugin.direct_accumulate(terms.cpu().numpy(), want_c, pair_hits.cpu().numpy(), pairs)
    assert (_bits(got) == _bits(want)).all()
    occluded = pair_hits.cpu().numpy().view(np.uint32)[:, 3] != MISS
    print(f"[direct] {which} S = {strata}: {pairs} pairs per entry, {counting.mean():.2f} count, {occluded[counting].mean():.2f} of those occluded")
    assert occluded[counting].any() and not occluded[~counting].any() and (~occluded[counting]).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fused call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["zoo", "instanced"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1500])
def test_direct_light_is_the_composition(request, which, n):
    import torch
    b = request.getfixturevalue(which)
    pt = b.pt
    rays = _list(b, n, seed=n)
    hits, surf = pt.trace_rays(rays, surface=True)
    for kw in (dict(strata=1, centered=True), dict(strata=3, seed=n, min_alpha=0.1)):
        p = abi.direct_params(**kw)
        out = torch.full((n + 3, 4), -7.0, dtype=torch.float32, device=rays.device)
        with pt._ordered(rays.device):
            plugin.check(pt.lib.PTDirectLight(pt.ctx, C.byref(p), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr()))
        assert (out[n:].cpu().numpy() == -7.0).all()                            # nothing past count
        want = _composition(pt, rays, hits, surf, **kw)
        assert (_bits(out[:n]) == _bits(want)).all(), kw
        assert (_bits(pt.direct_light(rays, hits, surf, **kw)) == _bits(want)).all()
        before = out.clone()
        with pt._ordered(rays.device):
            plugin.check(pt.lib.PTDirectLight(pt.ctx, C.byref(p), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), 0, out.data_ptr()))   # count 0 launches nothing
        assert (_bits(out) == _bits(before)).all()
    if n == 1500:
        g = want.cpu().numpy()
        miss = hits.cpu().numpy().view(np.uint32)[:, 3] == MISS
        assert miss.sum() >= 1500 // 7 and not g[miss].any() and (g[~miss, 3] == 1).all() and np.isfinite(g).all() and (g[:, 0:3] > 0).any()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRESS = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib", "libpt-stress-small-stacks.so")
STRESS_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from unity_webgpu_pathtracer_amd import scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
data, out = np.load(sys.argv[2]), {}
for name, s in (("zoo", scenes.material_zoo()), ("instanced", scenes.instanced_scene())):
    pt = PathTracer(s, width=48, height=32, samplesPerPass=1, maxRayBounces=2, schedule=1)
    rays = data[name]
    hits, surf = pt.trace_rays(rays, surface=True)
    kw = dict(strata=3, seed=77, min_alpha=0.05)
    out[name + "_fused"] = pt.direct_light(rays, hits, surf, **kw)
    _, terms, recv, _ = pt.shade_surfaces(rays, hits, surf)
    pair_rays, contrib = pt.direct_rays(rays, terms, recv, **kw)
    pair_hits = pt.trace_rays(pair_rays, any_hit=True)
    out[name + "_steps"] = pt.direct_accumulate(terms, contrib, pair_hits, pt.direct_pair_count(3))
    pt.close()
np.savez(sys.argv[3], **out)
'''


def test_grid_stride_and_slab_in_the_stress_build(zoo, instanced, tmp_path):
    """The stress build launches the fused kernels on at most 4 waves and keeps ONE CWBVH stack entry per lane in LDS: a list of 1,500
    entries makes every wave take six chunks, the last of them partly filled, and every walk that descends goes through the slab.
    There the fused call still equals the four-call composition, and both equal the default build's bits."""
    if not os.path.exists(STRESS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc"), "stress"], stdout=subprocess.DEVNULL)
    lists = {"zoo": _list(zoo, 1500, seed=21), "instanced": _list(instanced, 1500, seed=22)}
    src, out = str(tmp_path / "rays.npz"), str(tmp_path / "stress.npz")
    np.savez(src, **{k: v.cpu().numpy() for k, v in lists.items()})
    subprocess.check_call([sys.executable, "-c", STRESS_CHILD, ROOT, src, out], env=dict(os.environ, PT_PLUGIN=STRESS), timeout=300)
    got = np.load(out)
    for name, b in (("zoo", zoo), ("instanced", instanced)):
        rays = lists[name]
        hits, surf = b.pt.trace_rays(rays, surface=True)
        want = b.pt.direct_light(rays, hits, surf, strata=3, seed=77, min_alpha=0.05)
        assert (_bits(got[name + "_fused"]) == _bits(got[name + "_steps"])).all(), name
        assert (_bits(got[name + "_fused"]) == _bits(want)).all() and (got[name + "_fused"][:, 0:3] > 0).any(), name


def test_no_lights_no_pairs(box):
    """the shade box has no lights: no pairs, hits get {0, 0, 0, 1}, the mixed call is the lightmapped one"""
    pt = box.pt
    rays = _list(box, 300)
    hits, surf = pt.trace_rays(rays, surface=True)
    assert pt.direct_pair_count(1) == 0 and pt.direct_pair_count(4) == 0
    got = pt.direct_light(rays, hits, surf, strata=2).cpu().numpy()
    miss = hits.cpu().numpy().view(np.uint32)[:, 3] == MISS
    assert miss.any() and not got[miss].any() and (got[~miss] == np.array([0, 0, 0, 1], F)).all()
    mixed = pt.shade_mixed(rays, hits, surf, box.volume, box.reflections, box.dfg, strata=2)
    assert (_bits(mixed) == _bits(pt.shade_lightmapped(rays, hits, surf, box.volume, box.reflections, box.dfg))).all()
    _, terms, recv, _ = pt.shade_surfaces(rays, hits, surf)
    pair_rays, contrib = pt.direct_rays(rays, terms, recv)
    assert pair_rays.shape == (0, 8) and contrib.shape == (0, 4)
    assert (_bits(pt.direct_accumulate(terms, contrib, pair_rays[:, 0:4], 0)) == _bits(got)).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. mixed: the list call and a frame
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["zoo", "instanced"])
def test_mixed_is_lightmapped_plus_direct(request, which):
    b = request.getfixturevalue(which)
    pt = b.pt
    rays = _list(b, 1500)
    hits, surf = pt.trace_rays(rays, surface=True)
    kw = dict(strata=2, seed=9, min_alpha=0.05)
    base = pt.shade_lightmapped(rays, hits, surf, b.volume, b.reflections, b.dfg).cpu().numpy()
    direct = pt.direct_light(rays, hits, surf, **kw).cpu().numpy()
    want = base.copy()
    want[:, 0:3] = base[:, 0:3] + direct[:, 0:3]                                # one float32 add per channel; w is the lightmapped call's
    got = pt.shade_mixed(rays, hits, surf, b.volume, b.reflections, b.dfg, **kw)
    assert (_bits(got) == _bits(want)).all()
    assert (direct[:, 0:3] > 0).any() and not np.array_equal(_bits(got), _bits(base))


@pytest.mark.parametrize("which", ["zoo", "instanced"])
def test_frame_is_the_query_and_the_mixed_call(request, which):
    b = request.getfixturevalue(which)
    pt = b.pt
    kw = dict(strata=2, seed=3)
    frame, rays = pt.render_mixed(b.params, b.volume, b.reflections, b.dfg, return_rays=True, **kw)
    assert frame.shape == (H, W, 4) and rays.shape == (W * H, 8)
    lm, lm_rays = pt.render_lightmapped(b.params, b.volume, b.reflections, b.dfg, return_rays=True)
    assert (_bits(rays) == _bits(lm_rays)).all()
    hits, surf = pt.trace_rays(rays, surface=True)
    assert (_bits(frame.reshape(-1, 4)) == _bits(pt.shade_mixed(rays, hits, surf, b.volume, b.reflections, b.dfg, **kw))).all()
    assert (_bits(pt.render_mixed(b.params, b.volume, b.reflections, b.dfg, **kw)) == _bits(frame)).all()
    assert (_bits(frame) != _bits(lm)).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. shadows without tolerances
# ---------------------------------------------------------------------------------------------------------------------------
_EYE_Y = 6.0
_VFOV = 40.0
_FOOT = 2 * _EYE_Y * np.tan(np.radians(_VFOV) / 2) / H               # a pixel's footprint on the floor


def _shadow_scene(blocker=True, blocker_y=1.0, rect=False):
    """a 4 x 4 floor at y = 0, a light at (0, 2, 0) -- a point light, or a 1 x 1 rectangle facing down --, a 1 x 1 blocker halfway,
    seen from above"""
    sb = scenes.SoupBuilder()
    sb.quad((-2, 0, -2), (0, 0, 4), (4, 0, 0), (0, 1, 0), 1, 1, 0)
    if blocker:
        sb.quad((-0.5, blocker_y, -0.5), (0, 0, 1), (1, 0, 0), (0, 1, 0), 1, 1, 1)
    verts, attrs = sb.finish()
    mats = np.stack([scenes.pack_material(color=(0.8, 0.7, 0.6, 1.0), roughness=0.6), scenes.pack_material(color=(0.2, 0.3, 0.9, 1.0), roughness=0.8)])
    if rect:
        lights = scenes.pack_rect_light(center=(0.0, 2.0, 0.0), right=(1, 0, 0), up=(0, 0, 1), size=(1.0, 1.0), color=(30, 30, 30), rng=30.0)[None]
    else:
        lights = scenes.pack_point_light((0.0, 2.0, 0.0), (1.0, 0.9, 0.8), intensity=20.0, rng=30.0)[None]
    return scenes.Scene("direct_shadow", verts, attrs, mats, lights, np.zeros(0, dtype=np.uint32),
                        scenes.Camera(eye=(0.0, _EYE_Y, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), vfov_deg=_VFOV),
                        environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0), environment_intensity=0.0)


class _Shadow:
    def __init__(self, **scene):
        self.scene = _shadow_scene(**scene)
        self.pt = PathTracer(self.scene, width=W, height=H, samplesPerPass=1, maxRayBounces=2, schedule=1)

    def frame(self, rays=None, **kw):
        """(direct (n, 4), surface records (n, 12), hit mask, rays) of the frame's centre rays"""
        pt = self.pt
        if rays is None:
            rays = _frame_rays(pt)
        hits, surf = pt.trace_rays(rays, surface=True)
        direct = pt.direct_light(rays, hits, surf, **kw).cpu().numpy()
        return direct, surf.cpu().numpy(), hits.cpu().numpy().view(np.uint32)[:, 3] != MISS, rays


def _frame_rays(pt):
    """the W * H rays of Part 21 step 5, computed on the host from the frame parameters in float64 and rounded: the tests below
    compare frames of the SAME rays, so the rays need not be the kernel's bits"""
    import torch
    p = pt.params(seed=0)
    c2w = np.array(p.CamToWorld[:], np.float64).reshape(4, 4).T
    inv = np.array(p.CamInvProj[:], np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:H, 0:W]
    u = (xs.reshape(-1) + 0.5) / W * 2 - 1
    v = (ys.reshape(-1) + 0.5) / H * 2 - 1
    d = (inv @ np.stack([u, v, np.zeros_like(u), np.ones_like(u)]))[0:3]
    d = (c2w[0:3, 0:3] @ d).T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((W * H, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = c2w[0:3, 3], d, 100000.0
    return torch.from_numpy(rays).to(f"cuda:{pt.device}")


def test_point_light_shadow_is_exact():
    with_b, without = _Shadow(), _Shadow(blocker=False)
    try:
        direct, surf, hit, rays = with_b.frame(strata=1, centered=True)
        free, surf_free, hit_free, _ = without.frame(rays=rays, strata=1, centered=True)
        P = surf[:, 0:3].astype(np.float64)
        floor = hit & (P[:, 1] < 0.5)
        assert floor.sum() > 600 and (hit & ~floor).sum() > 20                  # the blocker is in view
        # the segment from (x, 0, z) to the light at (0, 2, 0) crosses y = 1 at (x / 2, z / 2): inside the blocker when both < 0.5
        m = _FOOT                                                                # leave out what lies within a pixel of the shadow's edge
        ax, az = np.abs(P[:, 0]), np.abs(P[:, 2])
        shadowed = floor & (ax < 1 - m) & (az < 1 - m)
        lit = floor & ((ax > 1 + m) | (az > 1 + m))
        print(f"[direct] point light: {shadowed.sum()} floor pixels in shadow, {lit.sum()} lit, {(floor & ~shadowed & ~lit).sum()} at the edge")
        assert shadowed.sum() >= 12 and lit.sum() > 400
        assert not direct[shadowed, 0:3].any() and (direct[shadowed, 3] == 1).all()
        assert (_bits(surf[lit]) == _bits(surf_free[lit])).all()
        assert (_bits(direct[lit]) == _bits(free[lit])).all() and (free[lit, 0:3] > 0).all()
        assert (free[shadowed, 0:3] > 0).all()
        # the unblocked floor against the float64 formula, within the bound tests/test_direct.py established
        pt = without.pt
        hits_t, surf_t = pt.trace_rays(rays, surface=True)
        _, terms, recv, _ = (x.cpu().numpy() for x in pt.shade_surfaces(rays, hits_t, surf_t))
        ok64, c64 = ref.contributions_f64(pt._bvhScene.lights, rays.cpu().numpy(), terms, recv, 1, 0, abi.PT_DIRECT_CENTERED, 0.0)
        k = np.flatnonzero(floor & hit_free)
        assert ok64[k].all()
        dev = (np.abs(free[k, 0:3] - c64[k]).max(axis=1) / np.abs(c64[k]).max(axis=1)).max()
        print(f"[direct] unblocked floor against float64: {dev:.3e} (cap {cases.F64_CAP:.3e})")
        assert dev <= cases.F64_CAP
    finally:
        with_b.pt.close()
        without.pt.close()


def _penumbra(P, floor):
    """floor pixels beside the +x edge of the blocker's shadow under the 1 x 1 rectangle light: light samples at lx < 1 - x are hidden"""
    return floor & (np.abs(P[:, 2]) < 0.35) & (P[:, 0] > 0.55) & (P[:, 0] < 1.45)


def test_rectangle_light_penumbra_and_jitter():
    with_b, without = _Shadow(rect=True), _Shadow(rect=True, blocker=False)
    try:
        rays = _frame_rays(with_b.pt)
        s3, surf, hit, _ = with_b.frame(rays=rays, strata=3, centered=True)
        free3 = without.frame(rays=rays, strata=3, centered=True)[0]
        P = surf[:, 0:3].astype(np.float64)
        floor = hit & (P[:, 1] < 0.5)
        # x in (0.72, 0.95): the columns at lx = -1/3 and 0 are hidden (their edges lie at 1.33 and 1.0), the one at 1/3 is not (0.67)
        pen = _penumbra(P, floor) & (P[:, 0] > 0.67 + 0.05) & (P[:, 0] < 1.0 - 0.05)
        assert pen.sum() >= 2
        assert (s3[pen, 0] > 0).all() and (s3[pen, 0] < free3[pen, 0]).all()
        # jitter: two seeds differ, one seed repeats
        a = with_b.frame(rays=rays, strata=2, seed=1)[0]
        assert (_bits(a) == _bits(with_b.frame(rays=rays, strata=2, seed=1)[0])).all()
        assert (_bits(a) != _bits(with_b.frame(rays=rays, strata=2, seed=2)[0])).any()
        # the mean over 64 seeds of a penumbra pixel lies between the centred S = 1 and S = 4 values.  The pixel is the one where the
        # hidden share of the light, 1 - (x - 0.5), lies furthest inside the interval the two centred grids span
        s1 = with_b.frame(rays=rays, strata=1, centered=True)[0][:, 0]
        s4 = with_b.frame(rays=rays, strata=4, centered=True)[0][:, 0]
        cand = np.flatnonzero(_penumbra(P, floor))
        x = P[cand, 0]
        lit_share = np.clip(x - 0.5, 0, 1)
        share1 = (x > 1.0).astype(np.float64)
        share4 = np.mean([(x > 1.0 - lx) for lx in (-0.375, -0.125, 0.125, 0.375)], axis=0)
        margin = np.minimum(lit_share - np.minimum(share1, share4), np.maximum(share1, share4) - lit_share)
        k = cand[margin.argmax()]
        assert margin.max() > 0.05, margin.max()
        mean = np.mean([with_b.frame(rays=rays, strata=4, seed=100 + s)[0][k, 0] for s in range(64)], dtype=np.float64)
        print(f"[direct] penumbra pixel x = {P[k, 0]:.3f}: S = 1 {s1[k]:.4f}, S = 4 {s4[k]:.4f}, jittered mean {mean:.4f}, unblocked {free3[k, 0]:.4f}")
        assert min(s1[k], s4[k]) <= mean <= max(s1[k], s4[k]) and s1[k] != s4[k]
    finally:
        with_b.pt.close()
        without.pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. updates are seen
# ---------------------------------------------------------------------------------------------------------------------------
def test_light_update_moves_the_mixed_frame_only():
    s = scenes.material_zoo()
    lo, hi = _scene_box(s)
    b = Baked(s, lo + (hi - lo) * F(0.1), hi - (hi - lo) * F(0.1))
    try:
        pt = b.pt
        args = (b.params, b.volume, b.reflections, b.dfg)
        mixed, baked = pt.render_mixed(*args, strata=2, centered=True), pt.render_lightmapped(*args)
        lights = pt.light_records()
        point = int(np.flatnonzero(lights[:, 3].view(np.uint32) == cases.POINT)[0])
        lights[point, 0:3] += F(1.5)
        pt.update_lights(lights)
        assert (_bits(pt.render_lightmapped(*args)) == _bits(baked)).all()
        moved = pt.render_mixed(*args, strata=2, centered=True)
        assert (_bits(moved) != _bits(mixed)).any()
        # ... and it is the frame of a scene built with the light there
        s2 = scenes.material_zoo()
        s2.lights[point, 0:3] += F(1.5)
        pt2 = PathTracer(s2, width=W, height=H, samplesPerPass=1, maxRayBounces=2, schedule=1)
        try:
            rays = b.frame_rays()
            hits, surf = pt.trace_rays(rays, surface=True)
            hits2, surf2 = pt2.trace_rays(rays, surface=True)
            assert (_bits(pt.direct_light(rays, hits, surf, strata=2, centered=True)) == _bits(pt2.direct_light(rays, hits2, surf2, strata=2, centered=True))).all()
        finally:
            pt2.close()
    finally:
        b.close()


def test_geometry_update_moves_the_shadow():
    low, high = _Shadow(), _Shadow(blocker_y=1.5)
    try:
        rays = _frame_rays(low.pt)
        before = low.frame(rays=rays, centered=True)[0]
        low.pt.update_geometry(high.scene.vertices)
        after = low.frame(rays=rays, centered=True)[0]
        fresh = high.frame(rays=rays, centered=True)[0]
        assert (_bits(after) == _bits(fresh)).all() and (_bits(after) != _bits(before)).any()
        # the blocker at 1.5 of 2 casts a shadow of half-width 2: floor pixels at |x| = 1.5 went dark
        surf = high.frame(rays=rays, centered=True)[1]
        moved = (surf[:, 1] < 0.5) & (np.abs(surf[:, 0]) > 1.2) & (np.abs(surf[:, 0]) < 1.8) & (np.abs(surf[:, 2]) < 1.0)
        assert moved.sum() > 10 and not after[moved, 0:3].any() and (before[moved, 0:3] > 0).all()
    finally:
        low.pt.close()
        high.pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. muted lights
# ---------------------------------------------------------------------------------------------------------------------------
def test_muted_lights_bake_like_a_scene_without_emission():
    s = scenes.material_zoo()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=1, maxRayBounces=2, schedule=1)
    dark_scene = scenes.material_zoo()
    dark_scene.lights[:, 4:7] = 0
    dark = PathTracer(dark_scene, width=W, height=H, samplesPerPass=1, maxRayBounces=2, schedule=1)
    try:
        p = pt.params(seed=7)
        pt.render_pass(p)
        before = pt.readback()
        with pt.muted_lights():
            assert not pt.light_records()[:, 4:7].any()
            muted = pt.bake_lightmap(32, 32, spp=8)
        want = dark.bake_lightmap(32, 32, spp=8)
        assert (_bits(muted) == _bits(want)).all() and (muted[..., 3] > 0).any()
        assert (_bits(pt.light_records()) == _bits(s.lights)).all()
        assert not np.array_equal(_bits(pt.bake_lightmap(32, 32, spp=8)), _bits(muted))            # the lights are back
        pt.render_pass(p)
        assert (_bits(pt.readback()) == _bits(before)).all()
    finally:
        pt.close()
        dark.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. a context without a scene
# ---------------------------------------------------------------------------------------------------------------------------
def test_calls_need_a_scene(zoo):
    import torch
    pt = zoo.pt
    lib = pt.lib
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(pt.device, C.byref(ctx)))
    try:
        rays = _list(zoo, 4)
        hits, surf = pt.trace_rays(rays, surface=True)
        s, keep = pt._shade_inputs(zoo.volume, zoo.reflections, zoo.dfg)
        out = torch.zeros((W * H, 4), dtype=torch.float32, device=rays.device)
        torch.cuda.synchronize()
        p, n = abi.direct_params(), C.c_uint32()
        a = (rays.data_ptr(), hits.data_ptr(), surf.data_ptr())
        assert lib.PTDirectPairCount(ctx, 1, C.byref(n)) == abi.PT_ERR_NO_SCENE
        assert lib.PTDirectRays(ctx, C.byref(p), *a, 4, out.data_ptr(), out.data_ptr()) == abi.PT_ERR_NO_SCENE
        assert lib.PTDirectLight(ctx, C.byref(p), *a, 4, out.data_ptr()) == abi.PT_ERR_NO_SCENE
        assert lib.PTShadeMixed(ctx, C.byref(s), C.byref(p), *a, 4, out.data_ptr()) == abi.PT_ERR_NO_SCENE
        assert lib.PTShadeMixedFrame(ctx, C.byref(zoo.params), C.byref(s), C.byref(p), out.data_ptr(), None) == abi.PT_ERR_NO_SCENE
        del keep
    finally:
        lib.PTDestroy(ctx)
