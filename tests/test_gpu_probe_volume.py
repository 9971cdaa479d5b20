"""Probe volumes (PTProbeDepth / PTProbeDepthHost / PTProbeGridIrradiance, include/ptmi_plugin.h Part 16) on the MI355X.

The rule is bit-exact and most of these tests hold it without tolerances: a depth record is the host twin's projection of the
closest-hit distances of the probe's own rays, and a lookup is the host twin's.  Two tests have tolerances, both from outside the
code under test: the closed form of the box's distances (1e-5 relative, what the gather and probe tests allow a closed form reached
through the traversal) and the leak test's ratio (1e-3, a condition of the feature; a numpy evaluation of the rule on the two rooms
with closed-form distances gave 8e-7 at most)."""
import ctypes as C
import math

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import chart_cases
import volume_ref

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def _box(emission=(0.0, 0.0, 0.0), occluder=None, ceiling=True):
    """tests/test_gpu_probe.py's box: a CLOSED Cornell shell (x, z in [-1, 1], y in [0, 2]), every material of roughness 1, a black
    sky.  emission: a 1.2 x 1.2 ceiling patch with an emissive material.  ceiling=False leaves the ceiling and its patch off."""
    sb, mats = scenes.SoupBuilder(), []
    scenes._cornell_shell(sb, mats)
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1), 1, 1, 0)           # front wall z = -1
    mats.append(scenes.pack_material(color=(0.5, 0.5, 0.5, 1.0), roughness=1.0, emission=emission))      # 3
    if ceiling:
        sb.quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0), 1, 1, 0)
        sb.quad((-0.6, 1.98, -0.6), (1.2, 0, 0), (0, 0, 1.2), (0, -1, 0), 1, 1, 3)
    if occluder is not None:
        sb.quad(*occluder, 1, 1, 0)
    verts, attrs = sb.finish()
    return scenes.Scene("volume_box", verts, attrs, np.stack(mats), np.zeros((0, 16), dtype=F), np.zeros(0, dtype=np.uint32),
                        scenes.Camera(eye=(0.0, 1.0, -0.9), target=(0.0, 1.0, 0.0), vfov_deg=40.0),
                        environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0), environment_intensity=0.0)


_EMISSION = (6.0, 5.0, 3.0)
_BOX_PROBES = np.array([(0.0, 1.0, 0.0), (-0.7, 0.3, 0.6), (0.55, 1.6, -0.4), (0.8, 0.15, -0.8), (-0.2, 1.9, 0.3)], F)
_INSTANCED_PROBES = np.array([(0.0, 1.0, 0.0), (-1.5, 0.5, 1.0), (2.0, 2.2, -1.0), (0.5, 0.3, -2.5), (-2.5, 1.5, 2.0)], F)


def _tracer(scene, bounces=3):
    return PathTracer(scene, width=64, height=48, samplesPerPass=1, maxRayBounces=bounces, schedule=1)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a depth record is the projection of the closest-hit distances of the probe's own rays
# ---------------------------------------------------------------------------------------------------------------------------
def _composition(pt, pos, seeds, samples, max_d, first, tag):
    n = len(pos)
    pr = pt.probe_rays(pos, spp=samples, first_sample=first, seeds=seeds)                   # PTProbeRays: origin, direction, rng, 0
    rays = np.zeros((n * samples, 8), F)
    rays[:, 0:6], rays[:, 6] = pr[:, 0:6], F(max_d)
    t = pt.trace_rays(rays)[:, 0]
    below, equal = float((t < F(max_d)).mean()), int((t == F(max_d)).sum())
    want = plugin.probe_depth_project(pos, t.reshape(n, samples), max_d, first_sample=first, seeds=seeds)
    got = pt.probe_depth(pos, spp=samples, max_distance=max_d, first_sample=first, seeds=seeds)
    bad = int((_bits(got) != _bits(want)).reshape(n, -1).any(axis=1).sum())
    print(f"[volume] {tag}, {samples} samples from {first:#x}: {bad} of {n} records differ from the projection of their rays' distances; "
          f"{below:.2f} of the rays end before maxDistance, {equal} at it")
    assert got.shape == (n, 64, 2) and bad == 0
    return rays, t, got, below, equal


def test_depth_is_the_ray_querys():
    import torch
    seeds = (np.arange(5, dtype=np.uint32) * 7919 + 0x1234).astype(np.uint32)
    max_d = 0.8
    pt = _tracer(_box())
    try:
        # 70: a partial last tile; 1: one entry in the only tile; 64: one whole tile.  count = 5: the second workgroup's last three
        # waves have no probe
        rays, t, full, below, equal = _composition(pt, _BOX_PROBES, seeds, 70, max_d, 0, "box")
        assert below > 0.1 and equal >= 1, "the test would compare trivia"
        _composition(pt, _BOX_PROBES, seeds, 1, max_d, 3, "box")
        _composition(pt, _BOX_PROBES, seeds, 64, max_d, 0xFFFFFFF0, "box")
        # the device entry point equals the host one; nothing past count is written
        dev = f"cuda:{pt.device}"
        d = pt.probe_depth(torch.from_numpy(_BOX_PROBES).to(dev), spp=70, max_distance=max_d, seeds=torch.from_numpy(seeds.astype(np.int64)).to(dev))
        assert d.is_cuda and (_bits(d.cpu().numpy()) == _bits(full)).all()
        rows = torch.from_numpy(plugin.probe_rows(_BOX_PROBES, seeds)).to(dev)
        out = torch.full((8, 64, 2), -123.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        plugin.check(pt.lib.PTProbeDepth(pt.ctx, rows.data_ptr(), 3, 0, 70, max_d, out.data_ptr()))
        pt.synchronize()
        out = out.cpu().numpy()
        assert (_bits(out[:3]) == _bits(full[:3])).all() and (out[3:] == F(-123.25)).all()
        assert pt.probe_depth(_BOX_PROBES[:0], spp=70, max_distance=max_d).shape == (0, 64, 2)         # count == 0 -> PT_OK
        # PTStats moves as the PTTraceRays call of the same rays moves it
        pt.set_stats_level(1)
        counted = []
        for call in (lambda: pt.probe_depth(_BOX_PROBES, spp=70, max_distance=max_d, seeds=seeds), lambda: pt.trace_rays(rays)):
            pt.reset_stats()
            call()
            pt.synchronize()
            counted.append(pt.stats().as_dict())
        pt.set_stats_level(0)
        assert counted[0] == counted[1] and counted[0]["closestHitRays"] == 5 * 70, counted
    finally:
        pt.close()


def test_depth_instanced():
    pt = _tracer(scenes.instanced_scene())
    try:
        _, _, _, below, equal = _composition(pt, _INSTANCED_PROBES, np.arange(5, dtype=np.uint32) + 77, 70, 3.0, 0, "instanced")
        assert below > 0.1 and equal >= 1, "the test would compare trivia"
    finally:
        pt.close()


def test_depth_chunks():
    """33 probes x 65,536 samples = two chunks of 32 and 1 probes through the same scratch, against two calls"""
    n, samples, max_d = 33, 65536, 0.8
    rng = np.random.default_rng(33)
    pos = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(0.1, 1.9, n), rng.uniform(-0.9, 0.9, n)], axis=1).astype(F)
    seeds = np.arange(n, dtype=np.uint32) + 1000
    pt = _tracer(_box())
    try:
        whole = pt.probe_depth(pos, spp=samples, max_distance=max_d, seeds=seeds)
        parts = [pt.probe_depth(pos[a:b], spp=samples, max_distance=max_d, seeds=seeds[a:b]) for a, b in ((0, 20), (20, 33))]
        assert (_bits(whole) == _bits(np.concatenate(parts))).all()
        assert np.isfinite(whole).all() and (whole[..., 0] > 0).all() and (whole[..., 0] <= F(max_d) * F(1.001)).all() and (whole[..., 0] < F(max_d)).any()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. closed form: one probe at the centre of the box without its ceiling
# ---------------------------------------------------------------------------------------------------------------------------
def test_depth_closed_form():
    """The walls are 1 away in x and z, the floor 1 below.  A ray that leaves through the open top has w_y > max(|w_x|, |w_z|), so
    the wall planes lie at least sqrt(2) along it: with maxDistance = 1.2 the formula's min(...) is maxDistance for it too."""
    samples, max_d = 256, 1.2
    pos = np.array([(0.0, 1.0, 0.0)], F)
    pt = _tracer(_box(ceiling=False))
    try:
        got = pt.probe_depth(pos, spp=samples, max_distance=max_d, seeds=[4242])[0].astype(np.float64)
    finally:
        pt.close()
    w = plugin.probe_directions(pos, samples, seeds=[4242])[:, 3:6].astype(np.float64)
    with np.errstate(divide="ignore"):
        dist = np.minimum(np.minimum(1.0 / np.abs(w[:, 0]), 1.0 / np.abs(w[:, 2])), np.where(w[:, 1] < 0, 1.0 / np.abs(w[:, 1]), np.inf))
    dist = np.minimum(dist, float(F(max_d)))
    assert 0.1 < (dist < float(F(max_d))).mean() < 0.95
    # the rule in float64
    l = np.arange(64)
    a, b = ((l % 8) + 0.5) * 0.25 - 1.0, ((l // 8) + 0.5) * 0.25 - 1.0
    z = 1.0 - np.abs(a) - np.abs(b)
    x = np.where(z < 0, (1.0 - np.abs(b)) * np.sign(a), a)
    y = np.where(z < 0, (1.0 - np.abs(a)) * np.sign(b), b)
    d = np.stack([x, y, z], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    wt = np.maximum(d @ w.T, 0.0) ** 32                                  # (64, samples)
    sw = wt.sum(axis=1)
    assert (sw > 1e-6).all()
    mean, mean2 = (wt @ dist) / sw, (wt @ (dist * dist)) / sw
    e1, e2 = np.abs(got[:, 0] - mean) / mean, np.abs(got[:, 1] - mean2) / mean2
    print(f"[volume] closed form, {samples} samples: largest relative error of mean {e1.max():.2e}, of mean2 {e2.max():.2e}; "
          f"means from {mean.min():.3f} to {mean.max():.3f}")
    assert e1.max() <= 1e-5 and e2.max() <= 1e-5
    assert mean.max() - mean.min() > 0.1


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the lookup is its host twin's
# ---------------------------------------------------------------------------------------------------------------------------
def test_lookup_equals_the_host_twin():
    import torch
    lib = plugin.load_library()
    scene = _box(emission=_EMISSION)
    pt = _tracer(scene)
    try:
        dev = f"cuda:{pt.device}"
        vol = pt.bake_probe_volume((-0.6, 0.5, -0.5), (0.6, 1.5, 0.5), (3, 2, 2), spp=64, depth_spp=64)
        assert vol.counts == (3, 2, 2)
        sh, depth = vol.sh.cpu().numpy(), vol.depth.cpu().numpy()
        assert (sh[:, 0, :] > 0).all() and (depth[..., 0] < F(vol.max_distance)).any()
        rng = np.random.default_rng(16)
        P = rng.uniform((-1.0, 0.0, -1.0), (1.0, 2.0, 1.0), (200, 3)).astype(F)
        P[0] = vol.positions()[4]                           # on a probe
        P[1] = (math.nan, 1.0, 0.0)
        P[2] = (0.6, 1.0, 0.5)                              # on the last planes
        N = _unit(rng.normal(0, 1, (200, 3)))
        bias = 0.05
        cut = 0
        for flags in range(4):
            g = plugin.probe_grid_desc(vol.grid.origin, vol.grid.spacing, vol.counts, wrap=bool(flags & 1), visibility=bool(flags & 2), normal_bias=bias)
            want = plugin.probe_grid_irradiance(g, sh, depth, P, N)
            for count in (1, 63, 64, 65, 200):
                got = vol.irradiance(P[:count], N[:count], wrap=bool(flags & 1), visibility=bool(flags & 2), normal_bias=bias)
                assert got.shape == (count, 4) and (_bits(got) == _bits(want[:count])).all(), (flags, count)
            assert (want[[0, 2], 3] > 0).all() and (np.abs(want[:, :3]).max(axis=1) > 0).sum() >= 150
            if flags == 0:
                assert np.abs(want[:, 3] - 1.0).max() <= 4 * EPS
            if flags == 3:
                cut = int((want[:, 3] < 0.5).sum())
        print(f"[volume] both flags: {cut} of 200 queries keep less than half of their support")
        assert cut > 0
        # device tensors in, a device tensor out; nothing past count is written
        g = plugin.probe_grid_desc(vol.grid.origin, vol.grid.spacing, vol.counts, normal_bias=bias)
        want = plugin.probe_grid_irradiance(g, sh, depth, P, N)
        d = vol.irradiance(torch.from_numpy(P).to(dev), torch.from_numpy(N).to(dev), normal_bias=bias)
        assert d.is_cuda and (_bits(d.cpu().numpy()) == _bits(want)).all()
        recv = torch.from_numpy(plugin.receiver_rows(P, N)).to(dev)
        out = torch.full((200, 4), -123.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        plugin.check(lib.PTProbeGridIrradiance(pt.ctx, C.byref(g), vol._rows.data_ptr(), vol._depth.data_ptr(), recv.data_ptr(), 130, out.data_ptr()))
        pt.synchronize()
        out = out.cpu().numpy()
        assert (_bits(out[:130]) == _bits(want[:130])).all() and (out[130:] == F(-123.25)).all()
        # visibility needs the depth
        out = torch.empty((200, 4), dtype=torch.float32, device=dev)
        assert lib.PTProbeGridIrradiance(pt.ctx, C.byref(g), vol._rows.data_ptr(), None, recv.data_ptr(), 130, out.data_ptr()) == abi.PT_ERR_INVALID_ARG
        assert b"depth" in lib.PTGetLastError()
        g.flags = abi.PT_GRID_WRAP
        plugin.check(lib.PTProbeGridIrradiance(pt.ctx, C.byref(g), vol._rows.data_ptr(), None, recv.data_ptr(), 200, out.data_ptr()))
        pt.synchronize()
        assert (_bits(out.cpu().numpy()) == _bits(plugin.probe_grid_irradiance(g, sh, None, P, N))).all()
        # a chart's receivers go in unchanged
        texels, recv = pt.chart_receivers(24, 24, uvs=chart_cases.floor_only_uvs(len(scene.tri_attrs)), seed=77)
        assert recv.shape == (24 * 24, 8)
        got = vol.irradiance(receivers=recv, normal_bias=bias)
        g = plugin.probe_grid_desc(vol.grid.origin, vol.grid.spacing, vol.counts, normal_bias=bias)
        assert got.is_cuda and (_bits(got.cpu().numpy()) == _bits(plugin.probe_grid_irradiance(g, sh, depth, receivers=recv.cpu().numpy()))).all()
        assert (got[:, :3].max(dim=1).values > 0).all()
    finally:
        pt.close()


def test_errors_with_a_context():
    lib = plugin.load_library()
    rows = plugin.probe_rows(_BOX_PROBES)
    out = np.empty((5, 64, 2), F)
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    try:
        assert lib.PTProbeDepthHost(ctx, rows.ctypes.data, 5, 0, 4, 1.0, out.ctypes.data) == abi.PT_ERR_NO_SCENE
        assert lib.PTProbeDepth(ctx, 16, 5, 0, 4, 1.0, 32) == abi.PT_ERR_NO_SCENE
        # the lookup needs no scene
        import torch
        dev = "cuda:0"
        g = plugin.probe_grid_desc((0, 0, 0), (1, 1, 1), (1, 1, 1), wrap=True, visibility=False)
        sh = torch.zeros((1, 28), dtype=torch.float32, device=dev)
        sh[0, :3] = 2.0 * math.sqrt(math.pi)
        recv = torch.from_numpy(plugin.receiver_rows([(0.2, 0.3, 0.4)], [(0.0, 1.0, 0.0)])).to(dev)
        e = torch.zeros((1, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        plugin.check(lib.PTProbeGridIrradiance(ctx, C.byref(g), sh.data_ptr(), None, recv.data_ptr(), 1, e.data_ptr()))
        plugin.check(lib.PTSynchronize(ctx))
        assert np.abs(e.cpu().numpy()[0, :3] - math.pi).max() <= 1e-6 * math.pi
    finally:
        lib.PTDestroy(ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. no leak: two rooms, a probe in each, light in one
# ---------------------------------------------------------------------------------------------------------------------------
def test_no_leak_through_a_wall():
    occluder = ((0.0, 0.0, -1.0), (0.0, 2.0, 0.0), (0.0, 0.0, 2.0), (1.0, 0.0, 0.0))          # the plane x = 0, floor to ceiling
    pos = np.array([(-0.5, 1.0, 0.0), (0.5, 1.0, 0.0)], F)
    pt = _tracer(_box(occluder=occluder))
    try:
        depth = pt.probe_depth(pos, spp=256, max_distance=1.5)
        sh = np.zeros((2, 9, 3), F)
        sh[0, 0] = 2.0 * math.sqrt(math.pi)                                                 # constant radiance 1 in probe 0's room
        P = np.array([(0.1, 1.0, 0.0), (-0.1, 1.0, 0.0)], F)
        N = np.array([(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)], F)
        grids = {on: plugin.probe_grid_desc((-0.5, 1.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1), wrap=on, visibility=on) for on in (False, True)}
        assert (_bits(plugin.probe_grid_positions(grids[True])) == _bits(pos)).all()
        import torch
        dev = f"cuda:{pt.device}"
        d_sh = torch.from_numpy(plugin.probe_coeff_rows(sh)).to(dev)
        d_depth = torch.from_numpy(depth).to(dev)
        recv = torch.from_numpy(plugin.receiver_rows(P, N)).to(dev)
        E = {}
        for on, g in grids.items():
            out = torch.empty((2, 4), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            plugin.check(pt.lib.PTProbeGridIrradiance(pt.ctx, C.byref(g), d_sh.data_ptr(), d_depth.data_ptr(), recv.data_ptr(), 2, out.data_ptr()))
            pt.synchronize()
            E[on] = out.cpu().numpy()
            assert (_bits(E[on]) == _bits(plugin.probe_grid_irradiance(g, sh, depth, P, N))).all()
        leak, kept = float(E[True][0, 0] / E[False][0, 0]), float(E[True][1, 0] / E[False][1, 0])
        print(f"[volume] behind the wall: {leak:.2e} of the unweighted value; in the lit room: {kept:.2f} of it")
        assert abs(float(E[False][0, 0]) - 0.4 * math.pi) < 1e-5 and abs(float(E[False][1, 0]) - 0.6 * math.pi) < 1e-5
        assert leak <= 1e-3
        assert kept >= 0.3
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_bake_probe_volume():
    pt = _tracer(_box(emission=_EMISSION))
    try:
        vol = pt.bake_probe_volume((-0.7, 0.3, -0.7), (0.7, 1.7, 0.7), (3, 3, 3), spp=64, depth_spp=64)
        pos = plugin.probe_grid_positions(vol.grid)
        assert pos.shape == (27, 3) and (_bits(pos) == _bits(volume_ref.grid_positions(vol.grid.origin, vol.grid.spacing, (3, 3, 3)))).all()
        assert np.abs(pos - pt.probe_grid((-0.7, 0.3, -0.7), (0.7, 1.7, 0.7), (3, 3, 3))).max() < 1e-6
        assert abs(vol.max_distance - 1.5 * 0.7 * math.sqrt(3.0)) < 1e-5
        sh, m2 = pt.probe_sh(pos, spp=64)
        assert (_bits(vol.sh.cpu().numpy()) == _bits(sh)).all() and (_bits(vol.m2.cpu().numpy()) == _bits(m2)).all()
        depth = pt.probe_depth(pos, spp=64, max_distance=vol.max_distance)
        assert (_bits(vol.depth.cpu().numpy()) == _bits(depth)).all()
        assert (sh[:, 0, :] > 0).all() and (depth[..., 0] < F(vol.max_distance)).any()
        # at a probe's own position, unweighted, the volume gives that probe's irradiance
        # Tolerance: with one live corner of weight 1 the lookup rounds twice (w * E, then the division); where g = (Q - origin) /
        # spacing misses the integer by a rounding, a neighbour enters with a weight of that size.  Both stay within 4 x 2^-23 of
        # the largest irradiance the volume holds; 64 samples leave single components of E near zero, so the error is taken
        # against that scale, not against each component
        N = _unit(np.random.default_rng(2).normal(0, 1, (27, 3)))
        own = pt.probe_irradiance(sh, N, np.arange(27))[:, :3].astype(np.float64)
        got = vol.irradiance(pos, N, wrap=False, visibility=False)
        scale = np.abs(own).max()
        err = np.abs(got[:, :3] - own).max() / scale
        print(f"[volume] at the probes: largest difference to the probe's own irradiance {err:.2e} of the largest irradiance {scale:.3f}")
        assert scale > 1.0 and err <= 4 * EPS and np.abs(got[:, 3] - 1.0).max() <= 4 * EPS
    finally:
        pt.close()
