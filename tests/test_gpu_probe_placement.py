"""Probe placement (PTProbePlace / PTProbePlaceHost / PTProbeGridIrradiancePlaced, include/ptmi_plugin.h Part 18) on the MI355X.

The rule is bit-exact and most of these tests hold it without tolerances: a placement is the host twin's, step for step, over the
surface queries of the probe's own rays, and a placed lookup is the host twin's.  One test has a tolerance from outside the code
under test: the closed form of the box's and the cube's plane distances (1e-5 relative, what the gather, probe and volume tests
allow a closed form reached through the traversal)."""
import ctypes as C
import math

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import placement_cases

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
EPS = 2.0 ** -23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def _box(emission=(0.0, 0.0, 0.0), cube=True):
    """tests/test_gpu_probe_volume.py's box, restated: a CLOSED Cornell shell (x, z in [-1, 1], y in [0, 2]), every material of
    roughness 1, a black sky, a 1.2 x 1.2 ceiling patch of material 3 (emission).  cube: a closed cube of side 0.4 centred at
    (0, 0.5, 0) whose normals point out of it.  tests/placement_cases.py is the same scene in closed form."""
    sb, mats = scenes.SoupBuilder(), []
    scenes._cornell_shell(sb, mats)
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1), 1, 1, 0)           # front wall z = -1
    mats.append(scenes.pack_material(color=(0.5, 0.5, 0.5, 1.0), roughness=1.0, emission=emission))      # 3
    sb.quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0), 1, 1, 0)
    sb.quad((-0.6, 1.98, -0.6), (1.2, 0, 0), (0, 0, 1.2), (0, -1, 0), 1, 1, 3)
    if cube:
        lo, s = placement_cases.CUBE_LO, 0.4
        sb.quad(lo, (s, 0, 0), (0, s, 0), (0, 0, -1), 1, 1, 0)
        sb.quad(lo + (0, 0, s), (s, 0, 0), (0, s, 0), (0, 0, 1), 1, 1, 0)
        sb.quad(lo, (0, 0, s), (0, s, 0), (-1, 0, 0), 1, 1, 0)
        sb.quad(lo + (s, 0, 0), (0, 0, s), (0, s, 0), (1, 0, 0), 1, 1, 0)
        sb.quad(lo, (s, 0, 0), (0, 0, s), (0, -1, 0), 1, 1, 0)
        sb.quad(lo + (0, s, 0), (s, 0, 0), (0, 0, s), (0, 1, 0), 1, 1, 0)
    verts, attrs = sb.finish()
    return scenes.Scene("placement_box", verts, attrs, np.stack(mats), np.zeros((0, 16), dtype=F), np.zeros(0, dtype=np.uint32),
                        scenes.Camera(eye=(0.0, 1.0, -0.9), target=(0.0, 1.0, 0.0), vfov_deg=40.0),
                        environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0), environment_intensity=0.0)


_EMISSION = (6.0, 5.0, 3.0)
_PROBES, _SEEDS = placement_cases.PROBES, placement_cases.SEEDS
_INSTANCED_PROBES = np.array([(0.0, 1.0, 0.0), (-1.5, 0.5, 1.0), (2.0, 2.2, -1.0), (0.5, 0.3, -2.5), (-2.5, 1.5, 2.0)], F)


def _tracer(scene, bounces=3):
    return PathTracer(scene, width=64, height=48, samplesPerPass=1, maxRayBounces=bounces, schedule=1)


def _same_stats(a, b):
    return all((a[name].view(U) == b[name].view(U)).all() for name in a.dtype.names)


def _args(q):
    return dict(spacing=[q.spacing[a] for a in range(3)], iterations=q.iterations, max_distance=q.maxDistance, min_front_distance=q.minFrontDistance,
                backface_share=q.backfaceShare, max_offset=q.maxOffset)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a placement is the host twin's over the surface queries of the probe's own rays, step for step
# ---------------------------------------------------------------------------------------------------------------------------
def _host_loop(pt, pos, seeds, samples, q, first):
    """PTProbeRays' directions from P + o, PTTraceRays with PT_QUERY_SURFACE, PTProbePlaceStepHost: iterations + 1 times"""
    n = len(pos)
    w = pt.probe_rays(pos, spp=samples, first_sample=first, seeds=seeds)[:, 3:6]
    rays = np.zeros((n * samples, 8), F)
    rays[:, 3:6], rays[:, 6] = w, F(q.maxDistance)
    o = np.zeros((n, 3), F)
    for step in range(q.iterations + 1):
        rays[:, 0:3] = np.repeat((pos + o).astype(F), samples, axis=0)
        hits, surf = pt.trace_rays(rays, surface=True)
        o, states, stats = plugin.probe_place_step(pos, hits, surf, q, move=step < q.iterations, offsets=o, first_sample=first, seeds=seeds)
    return o, states, stats


def _composition(pt, pos, seeds, samples, q, first, tag):
    want = _host_loop(pt, pos, seeds, samples, q, first)
    got = pt.place_probes(pos, spp=samples, first_sample=first, seeds=seeds, stats=True, **_args(q))
    print(f"[placement] {tag}, {samples} samples from {first:#x}, {q.iterations} iterations: states {got[1]}, |offset| {np.linalg.norm(got[0], axis=1)}, "
          f"back {got[2]['back']}, front {got[2]['front']}")
    assert (_bits(got[0]) == _bits(want[0])).all(), (got[0], want[0])
    assert (got[1] == want[1]).all() and _same_stats(got[2], want[2]), (got, want)
    return got


def test_placement_is_the_ray_querys_and_the_twins():
    import torch
    pt = _tracer(_box())
    try:
        # 70: a partial last round; 1: one sample; 64: one whole round.  count = 5: the second workgroup's last three waves have no probe
        q = abi.probe_place_params(0.5, min_front_distance=0.1, iterations=3)
        off, states, st = _composition(pt, _PROBES, _SEEDS, 70, q, 0, "box")
        moved = (off != 0).any(axis=1)
        assert (states == abi.PT_PROBE_INSIDE).any() and moved.any() and (~moved & (states == 0)).any(), "the test would compare trivia"
        _composition(pt, _PROBES, _SEEDS, 1, abi.probe_place_params(0.5, min_front_distance=0.1, iterations=1), 3, "box")
        _composition(pt, _PROBES, _SEEDS, 64, abi.probe_place_params(0.5, min_front_distance=0.1, iterations=1), 0xFFFFFFF0, "box")
        off0, states0, st0 = _composition(pt, _PROBES, _SEEDS, 70, abi.probe_place_params(0.5, min_front_distance=0.1, iterations=0), 0, "box")
        assert (off0 == 0).all() and states0[0] == abi.PT_PROBE_INSIDE and st0["back"][0] == 70
        # the device entry point equals the host one; nothing past count is written
        dev = f"cuda:{pt.device}"
        d_seeds = torch.from_numpy(_SEEDS.astype(np.int64)).to(dev)
        d_off, d_states = pt.place_probes(torch.from_numpy(_PROBES).to(dev), spp=70, seeds=d_seeds, **_args(q))
        assert d_off.is_cuda and (_bits(d_off.cpu().numpy()) == _bits(off)).all() and (d_states.cpu().numpy().astype(U) == states).all()
        rows = torch.from_numpy(plugin.probe_rows(_PROBES, _SEEDS)).to(dev)
        out = torch.full((8, 4), -123.25, dtype=torch.float32, device=dev)
        dst = torch.full((8, 8), -123.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        plugin.check(pt.lib.PTProbePlace(pt.ctx, rows.data_ptr(), 3, 0, 70, C.byref(q), 0, out.data_ptr(), dst.data_ptr()))
        pt.synchronize()
        out, dst = out.cpu().numpy(), dst.cpu().numpy()
        assert (_bits(out[:3, :3]) == _bits(off[:3])).all() and (_bits(out[:3, 3]) == states[:3]).all() and (out[3:] == F(-123.25)).all()
        assert _same_stats(np.ascontiguousarray(dst[:3]).view(abi.PLACE_STATS_DTYPE).reshape(3), st[:3]) and (dst[3:] == F(-123.25)).all()
        # PT_PLACE_KEEP_OFFSETS: one relocation step from the offsets of three is the fourth
        q1, q4 = abi.probe_place_params(0.5, min_front_distance=0.1, iterations=1), abi.probe_place_params(0.5, min_front_distance=0.1, iterations=4)
        again = pt.place_probes(_PROBES, spp=70, seeds=_SEEDS, start=off, **_args(q1))
        whole = pt.place_probes(_PROBES, spp=70, seeds=_SEEDS, **_args(q4))
        assert (_bits(again[0]) == _bits(whole[0])).all() and (again[1] == whole[1]).all()
        assert [len(x) for x in pt.place_probes(_PROBES[:0], spp=70, **_args(q))] == [0, 0]                # count == 0 -> PT_OK
        # PTStats moves as the iterations + 1 PTTraceRays calls over the same rays move it
        pt.set_stats_level(1)
        counted = []
        for call in (lambda: pt.place_probes(_PROBES, spp=70, seeds=_SEEDS, **_args(q)), lambda: _host_loop(pt, _PROBES, _SEEDS, 70, q, 0)):
            pt.reset_stats()
            call()
            pt.synchronize()
            counted.append(pt.stats().as_dict())
        pt.set_stats_level(0)
        assert counted[0] == counted[1] and counted[0]["closestHitRays"] == 4 * 5 * 70, counted
    finally:
        pt.close()


def test_placement_instanced():
    pt = _tracer(scenes.instanced_scene())
    try:
        q = abi.probe_place_params(1.0, max_distance=3.0, min_front_distance=0.4, iterations=3)
        off, states, st = _composition(pt, _INSTANCED_PROBES, np.arange(5, dtype=U) + 77, 70, q, 0, "instanced")
        assert (st["back"] + st["front"] > 0).any() and (st["back"] + st["front"] < 70).any(), "the test would compare trivia"
    finally:
        pt.close()


def test_errors_with_a_context():
    lib = plugin.load_library()
    rows = plugin.probe_rows(_PROBES)
    out = np.empty((5, 4), F)
    q = abi.probe_place_params(0.5)
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    try:
        assert lib.PTProbePlaceHost(ctx, rows.ctypes.data, 5, 0, 4, C.byref(q), 0, out.ctypes.data, None) == abi.PT_ERR_NO_SCENE
        assert lib.PTProbePlace(ctx, 16, 5, 0, 4, C.byref(q), 0, 32, None) == abi.PT_ERR_NO_SCENE
        assert lib.PTProbePlace(ctx, 16, 5, 0, 4, C.byref(q), 2, 32, None) == abi.PT_ERR_INVALID_ARG             # arguments come first
        # the placed lookup needs no scene
        import torch
        dev = "cuda:0"
        g = plugin.probe_grid_desc((0, 0, 0), (1, 1, 1), (1, 1, 1), wrap=True, visibility=False)
        sh = torch.zeros((1, 28), dtype=torch.float32, device=dev)
        sh[0, :3] = 2.0 * math.sqrt(math.pi)
        recv = torch.from_numpy(plugin.receiver_rows([(0.2, 0.3, 0.4)], [(0.0, 1.0, 0.0)])).to(dev)
        e = torch.full((1, 4), -1.0, dtype=torch.float32, device=dev)
        for state, want in ((0, math.pi), (abi.PT_PROBE_INSIDE, 0.0)):
            pl = torch.from_numpy(plugin.probe_placement_rows([(0.1, 0.0, 0.0)], [state])).to(dev)
            torch.cuda.synchronize()
            plugin.check(lib.PTProbeGridIrradiancePlaced(ctx, C.byref(g), sh.data_ptr(), None, pl.data_ptr(), recv.data_ptr(), 1, e.data_ptr()))
            plugin.check(lib.PTSynchronize(ctx))
            assert np.abs(e.cpu().numpy()[0, :3] - want).max() <= 1e-6 * math.pi
    finally:
        lib.PTDestroy(ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. closed forms: the twin over plane distances
# ---------------------------------------------------------------------------------------------------------------------------
def test_placement_closed_form():
    """256 samples, spacing 0.5, maxOffset 0.45, minFrontDistance 0.1.  The expected values are the host twin's over the plane
    distances of tests/placement_cases.py; the device differs from them by the trace's rounding of t alone: 1e-5 relative on every
    t, element by element (DESIGN.md 5.21's bound for a closed form reached through the traversal), and exactly 0 where there is
    no such sample.  An offset is a sum of at most `iterations` terms w * len with len = t + c or c - t, so a term is off by 1e-5 of
    the t it used, and an origin that is off by d changes the next t by d over the cosine of the incidence; with 2 allowed for
    that, an offset stays within iterations x 2 x 1e-5 x L, where L is the longest a move of this run can be: the largest
    tNearestBack of a buried probe on the grid plus half of minFrontDistance, or minFrontDistance (a probe that is outside after a
    move is not buried again in this scene).  Without a relocation step the offsets are 0 exactly.  What is read is printed."""
    samples = 256
    pt = _tracer(_box())
    try:
        res, longest = {}, 0.0
        for it in (0, 2):
            q = abi.probe_place_params(0.5, min_front_distance=0.1, max_offset=0.45, iterations=it)
            got = pt.place_probes(_PROBES, spp=samples, seeds=_SEEDS, stats=True, **_args(q))
            want = placement_cases.place(_PROBES, _SEEDS, samples, q)
            for name in ("back", "front", "nearestBack", "nearestFront", "farthestFront"):
                assert (got[2][name] == want[2][name]).all(), (it, name, got[2][name], want[2][name])
            t_err = 0.0
            for name in ("tNearestBack", "tNearestFront", "tFarthestFront"):
                g, w = got[2][name].astype(np.float64), want[2][name].astype(np.float64)
                some = w != 0
                assert (g[~some] == 0).all(), (it, name, g, w)
                if some.any():
                    t_err = max(t_err, float((np.abs(g[some] - w[some]) / w[some]).max()))
            if it == 0:
                buried = want[1] == abi.PT_PROBE_INSIDE
                longest = max(float(want[2]["tNearestBack"][buried].max()) + 0.5 * q.minFrontDistance, q.minFrontDistance)
            o_err = float(np.abs(got[0].astype(np.float64) - want[0]).max())
            bound = it * 2e-5 * longest
            print(f"[placement] closed form, {samples} samples, {it} iterations: t off by {t_err:.2e} relative per element at most, offsets by {o_err:.2e} "
                  f"(bound {bound:.2e}, longest move {longest:.3f}); states {got[1]}, |offset| {np.linalg.norm(got[0], axis=1)}")
            assert (got[1] == want[1]).all() and t_err <= 1e-5 and o_err <= bound
            res[it] = got
        off0, states0, st0 = res[0]
        assert states0[0] == abi.PT_PROBE_INSIDE and st0["back"][0] == samples and (off0 == 0).all()
        off, states, st = res[2]
        # the cube's probe: live, outside the cube, and at least the nearest face's 0.08 and half of minFrontDistance away
        final = _PROBES.astype(np.float64) + off
        assert states[0] == 0 and not placement_cases.in_cube(final[0])
        assert np.linalg.norm(off[0].astype(np.float64)) >= (0.08 + 0.05) * (1.0 - 1e-5)
        # the floor's probe: moved up, to minFrontDistance at most
        print(f"[placement] the floor's probe ends {final[1, 1]:.6f} above the floor, the cube's probe {np.linalg.norm(off[0]):.6f} from its grid point")
        assert 0.03 < final[1, 1] <= 0.1 * (1.0 + 1e-5)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. chunks
# ---------------------------------------------------------------------------------------------------------------------------
def test_placement_chunks():
    """17 probes x 65,536 samples = two chunks of 16 and 1 probes through the same scratch, each through both steps, against two calls"""
    n, samples = 17, 65536
    rng = np.random.default_rng(17)
    pos = np.stack([rng.uniform(-0.95, 0.95, n), rng.uniform(0.02, 1.9, n), rng.uniform(-0.95, 0.95, n)], axis=1).astype(F)
    pos[3], pos[16] = (0.12, 0.5, 0.0), (-0.1, 0.45, 0.1)                 # in the cube, one in each chunk
    seeds = np.arange(n, dtype=U) + 1000
    args = _args(abi.probe_place_params(0.5, min_front_distance=0.1, iterations=1))
    pt = _tracer(_box())
    try:
        whole = pt.place_probes(pos, spp=samples, seeds=seeds, stats=True, **args)
        parts = [pt.place_probes(pos[a:b], spp=samples, seeds=seeds[a:b], stats=True, **args) for a, b in ((0, 9), (9, 17))]
        assert (_bits(whole[0]) == _bits(np.concatenate([p[0] for p in parts]))).all()
        assert (whole[1] == np.concatenate([p[1] for p in parts])).all() and _same_stats(whole[2], np.concatenate([p[2] for p in parts]))
        assert (whole[0][[3, 16]] != 0).any(axis=1).all() and (whole[2]["back"] + whole[2]["front"] > 0).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the placed lookup is its host twin's, on a real placement and bake
# ---------------------------------------------------------------------------------------------------------------------------
_LO, _HI = (-0.58, 0.5, -0.7), (0.82, 1.5, 0.7)               # 3 x 3 x 3: probe 10 = (0.12, 0.5, 0) is the one inside the cube
_BURIED = 10


def test_placed_lookup_equals_the_host_twin():
    import torch
    lib = plugin.load_library()
    pt = _tracer(_box(emission=_EMISSION))
    try:
        dev = f"cuda:{pt.device}"
        # no relocation step: the cube's probe stays buried and the lookup has a corner to leave out; a second volume has moved probes
        for relocate in ({"iterations": 0}, True):
            vol = pt.bake_probe_volume(_LO, _HI, (3, 3, 3), spp=64, depth_spp=64, relocate=relocate)
            sh, depth, pl = vol.sh.cpu().numpy(), vol.depth.cpu().numpy(), vol.placement.cpu().numpy()
            states = _bits(pl[:, 3])
            assert (states[_BURIED] == abi.PT_PROBE_INSIDE) == (relocate is not True) and (np.delete(states, _BURIED) == 0).all()
            assert (pl[_BURIED, :3] != 0).any() == (relocate is True)
            rng = np.random.default_rng(18)
            P = rng.uniform((-0.7, 0.3, -0.8), (0.9, 1.6, 0.8), (200, 3)).astype(F)
            P[0] = vol.positions()[4]                           # on a probe's grid point
            P[1] = (math.nan, 1.0, 0.0)
            P[2] = _HI                                          # on the last planes
            N = _unit(rng.normal(0, 1, (200, 3)))
            bias = 0.05
            for flags in range(4):
                g = plugin.probe_grid_desc(vol.grid.origin, vol.grid.spacing, vol.counts, wrap=bool(flags & 1), visibility=bool(flags & 2), normal_bias=bias)
                want = plugin.probe_grid_irradiance(g, sh, depth, P, N, placement=pl)
                for count in (1, 63, 64, 65, 200):
                    got = vol.irradiance(P[:count], N[:count], wrap=bool(flags & 1), visibility=bool(flags & 2), normal_bias=bias)
                    assert got.shape == (count, 4) and (_bits(got) == _bits(want[:count])).all(), (flags, count)
                plain = plugin.probe_grid_irradiance(g, sh, depth, P, N)
                # (with both flags off every live corner weighs 1 wherever it stands: only a buried probe shows then)
                if flags or relocate is not True:
                    assert (_bits(want) != _bits(plain)).any(), "the placement changes nothing: the test would compare trivia"
        # nothing past count is written; dPlacement == NULL is PTProbeGridIrradiance, bit for bit
        g = plugin.probe_grid_desc(vol.grid.origin, vol.grid.spacing, vol.counts, normal_bias=bias)
        want = plugin.probe_grid_irradiance(g, sh, depth, P, N, placement=pl)
        recv = torch.from_numpy(plugin.receiver_rows(P, N)).to(dev)
        out = torch.full((200, 4), -123.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        plugin.check(lib.PTProbeGridIrradiancePlaced(pt.ctx, C.byref(g), vol._rows.data_ptr(), vol._depth.data_ptr(), vol.placement.data_ptr(), recv.data_ptr(),
                                                     130, out.data_ptr()))
        pt.synchronize()
        out = out.cpu().numpy()
        assert (_bits(out[:130]) == _bits(want[:130])).all() and (out[130:] == F(-123.25)).all()
        a, b = (torch.full((200, 4), -1.0, dtype=torch.float32, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        plugin.check(lib.PTProbeGridIrradiancePlaced(pt.ctx, C.byref(g), vol._rows.data_ptr(), vol._depth.data_ptr(), None, recv.data_ptr(), 200, a.data_ptr()))
        plugin.check(lib.PTProbeGridIrradiance(pt.ctx, C.byref(g), vol._rows.data_ptr(), vol._depth.data_ptr(), recv.data_ptr(), 200, b.data_ptr()))
        pt.synchronize()
        assert (_bits(a.cpu().numpy()) == _bits(b.cpu().numpy())).all()
        assert (_bits(a.cpu().numpy()) == _bits(plugin.probe_grid_irradiance(g, sh, depth, P, N))).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_bake_probe_volume_relocated():
    pt = _tracer(_box(emission=_EMISSION))
    try:
        plain = pt.bake_probe_volume(_LO, _HI, (3, 3, 3), spp=64, depth_spp=64)
        pos = plain.positions()
        assert [i for i in range(27) if placement_cases.in_cube(pos[i])] == [_BURIED]
        # unplaced: the cube is closed, the sky is black, and any-hit shadow rays stop at its faces
        sh0 = plain.sh.cpu().numpy()
        assert plain.placement is None and (_bits(sh0[_BURIED]) == 0).all() and (np.delete(sh0, _BURIED, axis=0)[:, 0, :] > 0).all()
        # relocate=None and False are today's bake, bit for bit
        again = pt.bake_probe_volume(_LO, _HI, (3, 3, 3), spp=64, depth_spp=64, relocate=False)
        assert again.placement is None and (_bits(again.sh.cpu().numpy()) == _bits(sh0)).all()
        assert (_bits(again.depth.cpu().numpy()) == _bits(plain.depth.cpu().numpy())).all()
        # relocated: the probe is live and lit, and the bakes are probe_sh and probe_depth at positions + offset
        vol = pt.bake_probe_volume(_LO, _HI, (3, 3, 3), spp=64, depth_spp=64, relocate=True)
        pl = vol.placement.cpu().numpy()
        off, states = pl[:, :3], _bits(pl[:, 3])
        assert (states == 0).all() and (off[_BURIED] != 0).any() and not placement_cases.in_cube(pos[_BURIED] + off[_BURIED])
        want_off, want_states = pt.place_probes(pos, [vol.grid.spacing[a] for a in range(3)])
        assert (_bits(off) == _bits(want_off)).all() and (states == want_states).all()
        sh, m2 = pt.probe_sh((pos + off).astype(F), spp=64)
        depth = pt.probe_depth((pos + off).astype(F), spp=64, max_distance=vol.max_distance)
        assert (_bits(vol.sh.cpu().numpy()) == _bits(sh)).all() and (_bits(vol.m2.cpu().numpy()) == _bits(m2)).all()
        assert (_bits(vol.depth.cpu().numpy()) == _bits(depth)).all()
        assert (sh[_BURIED, 0, :] > 0).all()
        # classified only: the probe is buried and the lookup leaves it out
        marked = pt.bake_probe_volume(_LO, _HI, (3, 3, 3), spp=64, depth_spp=64, relocate={"iterations": 0})
        mp = marked.placement.cpu().numpy()
        assert (mp[:, :3] == 0).all() and _bits(mp[:, 3])[_BURIED] == abi.PT_PROBE_INSIDE and (np.delete(_bits(mp[:, 3]), _BURIED) == 0).all()
        assert (_bits(marked.sh.cpu().numpy()) == _bits(sh0)).all()
        # the queries in the eight cells around the probe: on the floor and on the cube's faces below the grid's first layer the
        # lookup clamps, so take points in the free room around the cube
        rng = np.random.default_rng(3)
        P = rng.uniform((-0.5, 0.55, -0.6), (0.7, 0.95, 0.6), (256, 3)).astype(F)
        P = P[~np.array([((p > placement_cases.CUBE_LO - 0.05) & (p < placement_cases.CUBE_HI + 0.05)).all() for p in P])]
        N = _unit(rng.normal(0, 1, P.shape))
        truth = pt.irradiance(P, N, spp=1024)[:, :3].astype(np.float64)
        scale = truth.mean()
        for name, v in (("unplaced", plain), ("buried probe left out", marked), ("relocated", vol)):
            e = v.irradiance(P, N)
            err = np.abs(e[:, :3] - truth).mean() / scale
            print(f"[placement] {len(P)} queries around the cube's probe, {name}: mean m2 {e[:, 3].mean():.4f}, mean error against a 1,024-sample gather "
                  f"{err:.4f} of the mean irradiance {scale:.4f}")
            assert np.isfinite(e).all()
        # the buried probe left out, flags off: the support is what the other corners hold
        e_plain, e_marked = plain.irradiance(P, N, wrap=False, visibility=False), marked.irradiance(P, N, wrap=False, visibility=False)
        assert (e_marked[:, 3] < e_plain[:, 3] - 1e-3).any() and np.abs(e_plain[:, 3] - 1.0).max() <= 4 * EPS
    finally:
        pt.close()
