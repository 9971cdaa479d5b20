"""Reflection probes (PTReflectionRays / Capture / Prefilter / Lookup, include/ptmi_plugin.h Part 20) on the MI355X.

The rule is bit-exact and these tests hold it without tolerances, with two exceptions that the rule itself explains: a capture is
the host twin's fold of the radiance queries of its own rays; a list's results depend neither on its order, its length, the
schedule nor on how it is cut into chunks and slabs; the prefilter and lookup kernels equal their host twins.  The sky test allows
1e-5 relative on the prefiltered levels (a weighted mean of equal values, up to 256 terms of rounding in acc and sw), and the
end-to-end test asserts orderings only."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer, ReflectionProbes
import reflection_cases as cases

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
_EMISSION = (6.0, 5.0, 3.0)
_BOX_PROBES = np.array([(0.0, 1.0, 0.0), (-0.7, 0.3, 0.6), (0.55, 1.6, -0.4), (0.8, 0.15, -0.8), (-0.2, 1.9, 0.3)], F)
_SEEDS = (np.arange(5, dtype=np.uint32) * 7919 + 0xFFFFF000).astype(np.uint32)


def _box():
    """tests/test_gpu_probe.py's box: a CLOSED Cornell shell, every material of roughness 1, a 1.2 x 1.2 ceiling patch with an
    emissive material, a black sky"""
    sb, mats = scenes.SoupBuilder(), []
    scenes._cornell_shell(sb, mats)
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1), 1, 1, 0)           # front wall z = -1
    mats.append(scenes.pack_material(color=(0.5, 0.5, 0.5, 1.0), roughness=1.0, emission=_EMISSION))      # 3
    sb.quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0), 1, 1, 0)
    sb.quad((-0.6, 1.98, -0.6), (1.2, 0, 0), (0, 0, 1.2), (0, -1, 0), 1, 1, 3)
    verts, attrs = sb.finish()
    return scenes.Scene("reflection_box", verts, attrs, np.stack(mats), np.zeros((0, 16), dtype=F), np.zeros(0, dtype=np.uint32),
                        scenes.Camera(eye=(0.0, 1.0, -0.9), target=(0.0, 1.0, 0.0), vfov_deg=40.0),
                        environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0), environment_intensity=0.0)


def _ground_under_a_sky():
    """one floor quad at y = -0.5 under a uniform sky"""
    sb, mats = scenes.SoupBuilder(), [scenes.pack_material(color=(0.5, 0.5, 0.5, 1.0), roughness=1.0)]
    sb.quad((-4, -0.5, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0), 2, 2, 0)
    verts, attrs = sb.finish()
    return scenes.Scene("reflection_sky", verts, attrs, np.stack(mats), np.zeros((0, 16), dtype=F), np.zeros(0, dtype=np.uint32),
                        scenes.Camera(eye=(0.0, 1.0, -3.0), target=(0.0, 0.0, 0.0), vfov_deg=40.0),
                        environment_mode=0, environment_color=(0.6, 0.7, 1.0, 1.0), environment_intensity=0.75)


def _tracer(scene, schedule=1, bounces=3):
    return PathTracer(scene, width=64, height=48, samplesPerPass=1, maxRayBounces=bounces, schedule=schedule)


def _with_bounces(pt, bounces):
    p = pt.params(seed=0)
    p.MaxRayBounces = bounces
    return p


def _camera_probes(scene, n):
    eye, target = np.asarray(scene.camera.eye, np.float64), np.asarray(scene.camera.target, np.float64)
    rng = np.random.default_rng(n)
    t = rng.uniform(0.0, 0.5, (n, 1))
    return (eye + t * (target - eye) + rng.uniform(-0.15, 0.15, (n, 3)) * np.linalg.norm(target - eye)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. rays
# ---------------------------------------------------------------------------------------------------------------------------
def test_rays_equal_the_host_twin():
    import torch
    pt = _tracer(_box())
    try:
        pos, seeds = _BOX_PROBES[:3], _SEEDS[:3]
        rays = pt.reflection_rays(pos, res=8, spp=3, first_sample=0xFFFFFFFE, seeds=seeds)
        want = plugin.reflection_directions(pos, 8, 3, first_sample=0xFFFFFFFE, seeds=seeds)
        assert rays.shape == (3 * 64 * 3, 8) and (_bits(rays) == _bits(want)).all()
        dev = f"cuda:{pt.device}"
        d = pt.reflection_rays(torch.from_numpy(pos).to(dev), res=8, spp=3, first_sample=0xFFFFFFFE, seeds=torch.from_numpy(seeds.astype(np.int64)).to(dev))
        assert d.is_cuda and (_bits(d.cpu().numpy()) == _bits(want)).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. a capture is the fold of the radiance queries of its own rays
# ---------------------------------------------------------------------------------------------------------------------------
def _composition(pt, pos, seeds, res, samples, first, p, tag):
    n = len(pos)
    rays = pt.reflection_rays(pos, res=res, spp=samples, first_sample=first, seeds=seeds, params=p)
    rad = pt.radiance(rays, spp=1, params=p)
    want = plugin.reflection_fold(rad, n, res)
    got = pt.capture_reflection_base(pos, res=res, spp=samples, first_sample=first, seeds=seeds, params=p)
    lit = float((rad[:, :3].max(axis=1) > 0).mean())
    bad = int((_bits(got) != _bits(want)).any(axis=2).sum())
    print(f"[reflection] {tag}, {samples} samples from {first:#x}: {bad} of {n * res * res} texels differ from the fold of their rays' radiance; "
          f"{lit:.2f} of the samples are lit")
    assert got.shape == (n, res * res, 4) and bad == 0
    assert lit > 0.1, "the test would compare zeros"
    return got


@pytest.mark.parametrize("schedule", [1, 2, 3])
def test_capture_is_the_composition(schedule):
    pt = _tracer(_box(), schedule, bounces=3)
    try:
        p = _with_bounces(pt, 3)
        for samples, first in ((1, 0), (5, 0), (5, 0xFFFFFFF0), (1, 0xFFFFFFF0)):
            base = _composition(pt, _BOX_PROBES, _SEEDS, 8, samples, first, p, f"schedule {schedule}")
        assert (base[..., :3].max(axis=(1, 2)) > 0).all() and (base[..., 3] >= 0).all()
    finally:
        pt.close()


def test_capture_is_the_composition_instanced():
    scene = scenes.instanced_scene()
    pt = _tracer(scene, 1, bounces=3)
    try:
        _composition(pt, _camera_probes(scene, 5), np.arange(5, dtype=np.uint32) + 77, 8, 5, 0, pt.params(seed=0), "instanced")
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. list properties
# ---------------------------------------------------------------------------------------------------------------------------
def test_list_properties():
    import torch
    pt = _tracer(_box(), 1, bounces=3)
    try:
        p = _with_bounces(pt, 3)
        res, samples, n = 8, 3, 5
        pt.set_stats_level(1)
        pt.reset_stats()
        full = pt.capture_reflection_base(_BOX_PROBES, res=res, spp=samples, seeds=_SEEDS, params=p)
        pt.synchronize()
        st = pt.stats().as_dict()
        assert st["paths"] == n * res * res * samples and st["pixelsWritten"] == 0 and st["pixelsRead"] == 0, st
        pt.set_stats_level(0)
        # a permuted list gives permuted results; a shorter list gives its own probes' results
        perm = np.random.default_rng(7).permutation(n)
        got = pt.capture_reflection_base(_BOX_PROBES[perm], res=res, spp=samples, seeds=_SEEDS[perm], params=p)
        assert (_bits(got) == _bits(full[perm])).all()
        for k in (1, 2):
            got = pt.capture_reflection_base(_BOX_PROBES[:k], res=res, spp=samples, seeds=_SEEDS[:k], params=p)
            assert (_bits(got) == _bits(full[:k])).all(), k
        # the device variant equals the host variant; nothing past count is written
        dev = f"cuda:{pt.device}"
        d = pt.capture_reflection_base(torch.from_numpy(_BOX_PROBES).to(dev), res=res, spp=samples, seeds=torch.from_numpy(_SEEDS.astype(np.int64)).to(dev), params=p)
        assert d.is_cuda and (_bits(d.cpu().numpy()) == _bits(full)).all()
        rows = torch.from_numpy(plugin.probe_rows(_BOX_PROBES, _SEEDS)).to(dev)
        out = torch.full((n, res * res, 4), -123.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        plugin.check(pt.lib.PTReflectionCapture(pt.ctx, C.byref(pt._radiance_params(p)), rows.data_ptr(), 3, res, 0, samples, out.data_ptr()))
        pt.synchronize()
        out = out.cpu().numpy()
        assert (_bits(out[:3]) == _bits(full[:3])).all() and (out[3:] == F(-123.25)).all()
        # errors that need a context
        with pytest.raises(plugin.PluginError) as e:
            pt.prefilter_reflection(d, res, 3)
        assert e.value.code == abi.PT_ERR_INVALID_ARG
        assert pt.lib.PTReflectionPrefilter(pt.ctx, d.data_ptr(), n, res, 2, d.data_ptr()) == abi.PT_ERR_INVALID_ARG and b"alias" in pt.lib.PTGetLastError()
        for schedule in (0, 4):
            pt.set_schedule(schedule)
            with pytest.raises(plugin.PluginError) as e:
                pt.capture_reflection_base(_BOX_PROBES, res=res, spp=samples, params=p)
            assert e.value.code == abi.PT_ERR_UNSUPPORTED and f"schedule {schedule}" in str(e.value)
            assert pt.reflection_rays(_BOX_PROBES, res=res, spp=2, params=p).shape == (n * res * res * 2, 8)      # needs no scene and no schedule
        pt.set_schedule(1)
        assert pt.capture_reflection_base(_BOX_PROBES[:0], res=res, spp=samples, params=p).shape == (0, res * res, 4)      # count == 0 -> PT_OK
    finally:
        pt.close()
    lib = plugin.load_library()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    try:
        rows = plugin.probe_rows(_BOX_PROBES)
        out = np.empty((5, 64, 4), F)
        assert lib.PTReflectionCaptureHost(ctx, C.byref(p), rows.ctypes.data, 5, 8, 0, 2, out.ctypes.data) == abi.PT_ERR_NO_SCENE
    finally:
        lib.PTDestroy(ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. chunks and slabs
# ---------------------------------------------------------------------------------------------------------------------------
def test_chunks_and_slabs():
    """17 probes x 16 x 16 texels x 1,024 samples = 4,456,448 slots: a slab of 2^22 slots (two chunks of 2^21) and a slab of
    262,144, against the same probes captured one call each (one slab of one chunk each)"""
    n, res, samples = 17, 16, 1024
    assert n * res * res * samples > 1 << 22
    rng = np.random.default_rng(17)
    pos = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(0.2, 1.8, n), rng.uniform(-0.8, 0.8, n)], axis=1).astype(F)
    seeds = np.arange(n, dtype=np.uint32) + 1000
    pt = _tracer(_box(), 1, bounces=2)
    try:
        p = _with_bounces(pt, 2)
        whole = pt.capture_reflection_base(pos, res=res, spp=samples, seeds=seeds, params=p)
        parts = np.concatenate([pt.capture_reflection_base(pos[k:k + 1], res=res, spp=samples, seeds=seeds[k:k + 1], params=p) for k in range(n)])
        assert (_bits(whole) == _bits(parts)).all()
        assert np.isfinite(whole).all() and (whole[..., :3].max(axis=(1, 2)) > 0).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a uniform sky
# ---------------------------------------------------------------------------------------------------------------------------
def test_uniform_sky():
    res, levels = 16, 3
    pt = _tracer(_ground_under_a_sky(), 1, bounces=3)
    try:
        p = _with_bounces(pt, 3)
        P = np.array([(0.1, 1.0, -0.2)], F)
        up = np.zeros((1, 8), F)
        up[0, 0:3], up[0, 3:6] = P[0], (0.0, 1.0, 0.0)
        sky = pt.radiance(up, spp=1, params=p)[0, :3]
        assert (sky > 0).all()
        base = pt.capture_reflection_base(P, res=res, spp=2, seeds=[3], params=p)
        # The floor ends 4 away and 1.5 below the probe: only directions with y < -0.3 reach it.  A texel is less than 0.4 wide in
        # direction space at this size, so both samples of a texel whose centre has y > 0.1 see the sky; c + c and / 2 are exact
        t = np.arange(res * res)
        a, b = ((t % res + 0.5) / res) * 2 - 1, ((t // res + 0.5) / res) * 2 - 1
        z = 1 - np.abs(a) - np.abs(b)
        y = np.where(z < 0, (1 - np.abs(a)) * np.where(b < 0, -1.0, 1.0), b)
        x = np.where(z < 0, (1 - np.abs(b)) * np.where(a < 0, -1.0, 1.0), a)
        centre_y = y / np.sqrt(x * x + y * y + z * z)
        above = centre_y > 0.1
        assert above.sum() > res * res // 4
        assert (_bits(base[0, above, :3]) == _bits(np.tile(sky, (int(above.sum()), 1)))).all()
        assert (base[0, centre_y < -0.7, :3] != sky).any()                 # the ground is something else
        # Every level keeps the sky where a texel's whole support is sky.  The up-facing lookup of each level has it: a lobe around
        # +y weighs only directions with y > 0.  To 1e-5 relative: acc / sw of up to 256 equal values with their roundings
        maps = pt.prefilter_reflection(base, res, levels)
        for k in range(levels):
            got = plugin.reflection_lookup(maps, res, levels, np.array([(0.0, 1.0, 0.0)], F), k / (levels - 1), 0)[0, :3]
            rel = float(np.abs(got.astype(np.float64) - sky).max() / sky.max())
            print(f"[reflection] uniform sky, level {k}: up-facing lookup off the sky by {rel:.2e} relative")
            assert rel <= 1e-5
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6, 7. the prefilter and lookup kernels against their twins
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,levels,n", [(8, 2, 3), (16, 3, 3), (32, 4, 2), (64, 5, 1)])
def test_prefilter_kernel_equals_the_twin(res, levels, n):
    """32 / 4 has four source tiles; at 64 / 5 level 1 has four output blocks and level 4 sixteen lanes of 256"""
    pt = _tracer(_box())
    try:
        base = cases.random_base(n, res, seed=res + 1)
        got = pt.prefilter_reflection(base, res, levels)
        want = plugin.reflection_prefilter(base, res, levels)
        assert got.shape == want.shape and (_bits(got) == _bits(want)).all(), np.argwhere(_bits(got) != _bits(want))[:5]
    finally:
        pt.close()


def _lookup_dev(pt, maps, res, levels, q, Q=None, boxes=None):
    import torch
    dev = f"cuda:{pt.device}"
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    d_maps, d_q, d_Q, d_b = t(maps), t(q), t(None if Q is None else plugin.probe_rows(Q)), t(boxes)
    out = torch.full((len(q) + 1, 4), -7.5, dtype=torch.float32, device=dev)
    with pt._ordered(dev):
        plugin.check(pt.lib.PTReflectionLookup(pt.ctx, d_maps.data_ptr(), maps.shape[0], res, levels, None if d_Q is None else d_Q.data_ptr(),
                                               None if d_b is None else d_b.data_ptr(), d_q.data_ptr(), len(q), out.data_ptr()))
    out = out.cpu().numpy()
    assert (out[-1] == F(-7.5)).all()                                       # nothing past count
    return out[:-1]


@pytest.mark.parametrize("res,levels", [(8, 2), (16, 3), (32, 4)])
def test_lookup_kernel_equals_the_twin(res, levels):
    n = 3
    maps = cases.random_maps(n, res, levels, seed=levels)
    q = cases.query_set(n)
    Q, boxes = cases.probe_boxes(n)
    pt = _tracer(_box())
    try:
        got = _lookup_dev(pt, maps, res, levels, q)
        want = plugin.reflection_lookup(maps, res, levels, queries=q)
        assert (_bits(got) == _bits(want)).all(), np.argwhere(_bits(got) != _bits(want))[:5]
        assert (_bits(_lookup_dev(pt, maps, res, levels, q, Q)) == _bits(want)).all()          # probes without boxes: no projection
        got_b = _lookup_dev(pt, maps, res, levels, q, Q, boxes)
        want_b = plugin.reflection_lookup(maps, res, levels, queries=q, probe_positions=Q, boxes=boxes)
        assert (_bits(got_b) == _bits(want_b)).all(), np.argwhere(_bits(got_b) != _bits(want_b))[:5]
        assert (_bits(want_b) != _bits(want)).any()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_in_the_box():
    import torch
    pt = _tracer(_box(), 1, bounces=3)
    try:
        p = _with_bounces(pt, 3)
        probes = pt.capture_reflection_probes(_BOX_PROBES[:2], res=16, spp=16, levels=3, seeds=_SEEDS[:2], boxes=((-1, 0, -1), (1, 2, 1)), params=p)
        assert isinstance(probes, ReflectionProbes) and probes.maps.is_cuda and probes.maps.shape == (2, 256 + 64 + 16, 4)
        assert probes.level(1).shape == (2, 8, 8, 4) and probes.level(2).shape == (2, 4, 4, 4)
        # the maps are the composition of the steps
        base = pt.capture_reflection_base(_BOX_PROBES[:2], res=16, spp=16, seeds=_SEEDS[:2], params=p)
        assert (_bits(probes.level(0).cpu().numpy().reshape(2, 256, 4)) == _bits(base)).all()
        assert (_bits(probes.maps.cpu().numpy()) == _bits(plugin.reflection_prefilter(base, 16, 3))).all()
        d = np.array([(0.0, 1.0, 0.0), (0.0, -1.0, 0.0)], F)
        lum = {}
        for r in (0.0, 1.0):
            got = probes.lookup(d, r, 0)
            assert got.shape == (2, 4) and (got[:, 3] == 1).all()
            lum[r] = got[:, :3] @ np.array([0.299, 0.587, 0.114])
            print(f"[reflection] roughness {r}: towards the ceiling patch {lum[r][0]:.4f}, towards the floor {lum[r][1]:.4f}")
        assert lum[0.0][0] > lum[0.0][1] > 0
        assert lum[1.0][0] / lum[1.0][1] < lum[0.0][0] / lum[0.0][1]
        # device tensors in, a device tensor out; with positions the box projection moves a lookup
        dev = probes.maps.device
        t_d = torch.from_numpy(d).to(dev)
        t_got = probes.lookup(t_d, 0.0, torch.zeros(2, dtype=torch.int64, device=dev))
        assert t_got.is_cuda and (_bits(t_got.cpu().numpy()) == _bits(probes.lookup(d, 0.0, 0))).all()
        side = np.array([(0.6, 0.5, 0.64)], F)
        at = np.array([(0.5, 0.4, -0.3)], F)
        assert (_bits(probes.lookup(side, 0.0, 0, positions=at)) != _bits(probes.lookup(side, 0.0, 0))).any()
        want = plugin.reflection_lookup(probes.maps.cpu().numpy(), 16, 3, side, 0.0, 0, positions=at, probe_positions=_BOX_PROBES[:2],
                                        boxes=probes.box_rows.cpu().numpy())
        assert (_bits(probes.lookup(side, 0.0, 0, positions=at)) == _bits(want)).all()
    finally:
        pt.close()
