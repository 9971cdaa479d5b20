"""SH light probes (PTProbeSH / PTProbeSHHost / PTProbeRays / PTProbeIrradiance, include/ptmi_plugin.h Part 15) on the MI355X.

The rule is bit-exact and most of these tests hold it without tolerances: a probe's samples are the radiance queries of its rays,
projected by tests/probe_ref.py; a list's results depend neither on its order, the schedule nor on how it is cut into chunks.  Two
tests have tolerances, both from outside the code under test: the closed form of a point or spot light (1e-5 relative, the gather
test's own for the same arithmetic) and the band-1 identity against PTGatherIrradiance (five standard errors from the calls' own
m2)."""
import ctypes as C
import math

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import probe_ref

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def _box(emission=(0.0, 0.0, 0.0), lights=(), occluder=None, ceiling=True, sky="basic"):
    """tests/test_gpu_gather.py's box: a CLOSED Cornell shell, every material of roughness 1.  emission: a 1.2 x 1.2 ceiling patch
    with an emissive MATERIAL (no analytic light).  Basic sky of intensity 0.  ceiling=False leaves the ceiling and its patch off:
    the render's shadow rays have no far end, so a light that geometry encloses lights nothing."""
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
    L = np.stack(lights).astype(F) if len(lights) else np.zeros((0, 16), dtype=F)
    s = scenes.Scene("probe_box", verts, attrs, np.stack(mats), L, np.zeros(0, dtype=np.uint32),
                     scenes.Camera(eye=(0.0, 1.0, -0.9), target=(0.0, 1.0, 0.0), vfov_deg=40.0),
                     environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0), environment_intensity=0.0)
    if sky == "black map":
        # mode 0 with an all-black 8 x 4 map at intensity 1: as dark as the basic sky of intensity 0, but every surface hit now draws
        # and traces an environment shadow ray, which adds nothing (envCdfSum == 0: its pdf is 0 / 0, valid == 2)
        texels = np.zeros((4, 8, 4), dtype=F)
        texels[..., 3] = 1.0
        s.environment_mode, s.environment_intensity, s.environment_texture = 0, 1.0, texels
    else:
        assert sky == "basic"
    return s


_EMISSION = (6.0, 5.0, 3.0)
_BOX_PROBES = np.array([(0.0, 1.0, 0.0), (-0.7, 0.3, 0.6), (0.55, 1.6, -0.4), (0.8, 0.15, -0.8), (-0.2, 1.9, 0.3)], F)


def _tracer(scene, schedule=1, bounces=3):
    return PathTracer(scene, width=64, height=48, samplesPerPass=1, maxRayBounces=bounces, schedule=schedule)


def _with_bounces(pt, bounces):
    p = pt.params(seed=0)
    p.MaxRayBounces = bounces
    return p


def _camera_probes(scene, n):
    """n positions spread around the first half of the camera's line of sight"""
    eye, target = np.asarray(scene.camera.eye, np.float64), np.asarray(scene.camera.target, np.float64)
    rng = np.random.default_rng(n)
    t = rng.uniform(0.0, 0.5, (n, 1))
    return (eye + t * (target - eye) + rng.uniform(-0.15, 0.15, (n, 3)) * np.linalg.norm(target - eye)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a probe's samples are the radiance queries of its rays; the projection is the restated rule's, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def _continuation(pt, pos, seeds, samples, p, tag, first=0):
    n = len(pos)
    rays = pt.probe_rays(pos, spp=samples, first_sample=first, seeds=seeds, params=p)
    host = plugin.probe_directions(pos, samples, first_sample=first, seeds=seeds)
    assert rays.shape == (n * samples, 8) and (_bits(rays) == _bits(host)).all()
    rad = pt.radiance(rays, spp=1, params=p)
    want_sh, want_m2 = probe_ref.project(rays[:, 3:6].reshape(n, samples, 3), rad[:, :3].reshape(n, samples, 3))
    sh, m2 = pt.probe_sh(pos, spp=samples, first_sample=first, seeds=seeds, delta_lights=False, params=p)
    bad = int((_bits(sh) != _bits(want_sh)).reshape(n, -1).any(axis=1).sum())
    print(f"[probe] {tag}, {samples} samples: {bad} of {n} probes differ from the projection of their rays' radiance; "
          f"{float((rad[:, :3].max(axis=1) > 0).mean()):.2f} of the samples are lit")
    assert bad == 0
    assert (_bits(m2) == _bits(want_m2)).all()
    return rad, sh


@pytest.mark.parametrize("schedule", [1, 2, 3])
def test_continuation_is_the_radiance_query(schedule):
    seeds = (np.arange(5, dtype=np.uint32) * 7919 + 0x1234).astype(np.uint32)
    pt = _tracer(_box(emission=_EMISSION), schedule, bounces=3)
    try:
        p = _with_bounces(pt, 3)
        assert p.UseRussianRoulette == 1
        # 70: some lanes own two samples, others one, and the count is no multiple of 64; 1 and 64: one lane, every lane once
        rad, sh = _continuation(pt, _BOX_PROBES, seeds, 70, p, f"schedule {schedule}")
        assert (rad[:, :3].max(axis=1) > 0).mean() > 0.1, "the emissive patch lights nothing: the test would compare zeros"
        assert (sh[:, 0, :] > 0).all()
        _continuation(pt, _BOX_PROBES, seeds, 1, p, f"schedule {schedule}", first=3)
        _continuation(pt, _BOX_PROBES, seeds, 64, p, f"schedule {schedule}", first=0xFFFFFFF0)
    finally:
        pt.close()


def test_continuation_instanced():
    scene = scenes.instanced_scene()
    pt = _tracer(scene, 1, bounces=3)
    try:
        pos = _camera_probes(scene, 5)
        rad, _ = _continuation(pt, pos, np.arange(5, dtype=np.uint32) + 77, 70, pt.params(seed=0), "instanced")
        assert (rad[:, :3].max(axis=1) > 0).mean() > 0.1
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. delta lights, closed form
# ---------------------------------------------------------------------------------------------------------------------------
_LIGHT_POS = (0.2, 1.6, 0.1)
_LIGHTS = {
    "point": scenes.pack_point_light(_LIGHT_POS, (1.0, 0.8, 0.6), intensity=5.0, rng=10.0),
    # aimed at the first probe (inside the inner cone); the second sits in the soft edge between 20 and 60 degrees
    "spot": scenes.pack_spot_light(_LIGHT_POS, (-0.5, -1.0, -0.3), 120.0, 40.0, (0.6, 0.8, 1.0), intensity=7.0, rng=12.0),
}


def _direct(light, P, w):
    """gather_ref.direct_irradiance for the receiver whose NEE origin is the probe.  The closed form lights a receiver from
    P + N * PT_EPSILON (Part 13's NEE origin); a probe is lit at P itself (Part 15: scatterPos = P).  With N = w, the direction to
    the light, that step of 1e-4 towards a light 1.2 away changes the distance falloff by 4.3e-5 (measured with the probe's own
    position: a relative error of 4.34e-05 at the first probe), more than the 1e-5 this test allows for the arithmetic.  So the
    receiver is placed one epsilon behind the probe: its NEE origin is the probe's position to a rounding."""
    return probe_ref.direct_irradiance(light, np.asarray(P, F) - np.asarray(w, F) * F(1.0e-4), w)


# the sky: the box's own basic sky of intensity 0, and an all-black environment map -- the walls a probe sees now draw and trace an
# environment shadow ray that adds nothing; the delta term is the difference of two results with the same paths, so it cannot move
_SKIES = [pytest.param("point", "basic", id="point"), pytest.param("spot", "basic", id="spot"),
          pytest.param("point", "black map", id="point-black-map"), pytest.param("spot", "black map", id="spot-black-map")]


@pytest.mark.parametrize("kind,sky", _SKIES)
def test_delta_light_closed_form(kind, sky):
    light = _LIGHTS[kind]
    lp = np.asarray(_LIGHT_POS, dtype=np.float64)
    # probes 0, 1: in the open; 2: behind the occluder; 3: beside the light, behind the spot's cone.  All four lie below the light, so
    # that their lines to it leave through the open top
    pos = np.array([(-0.3, 0.6, -0.2), (0.5, 0.5, -0.3), (0.6, 0.4, 0.5), (0.9, 1.3, 0.6)], dtype=np.float64)
    to_light = (lp - pos) / np.linalg.norm(lp - pos, axis=1, keepdims=True)
    assert (np.abs(to_light[:2]) > 0.1).all(), "the light directions are not axis-aligned: all nine signs and the axis order are pinned"
    mid = 0.5 * (lp + pos[2])
    a = np.cross(to_light[2], (0.0, 1.0, 0.0)); a /= np.linalg.norm(a)
    b = np.cross(to_light[2], a)
    occluder = (tuple(mid - 0.2 * a - 0.2 * b), tuple(0.4 * a), tuple(0.4 * b), tuple(to_light[2]))
    pos32, samples, seeds = pos.astype(F), 70, np.arange(4, dtype=np.uint32) + 11
    # The dark box with its top open.  Without the flag a probe still sees the walls the light shines on (their own NEE), so the
    # difference of the two results carries one rounding of the sum: half an ulp of a coefficient of order 1, a hundredth of 1e-5
    pt = _tracer(_box(lights=[light], occluder=occluder, ceiling=False, sky=sky), 1, bounces=2)
    try:
        p = _with_bounces(pt, 2)
        off, m2_off = pt.probe_sh(pos32, spp=samples, seeds=seeds, delta_lights=False, params=p)
        on, m2_on = pt.probe_sh(pos32, spp=samples, seeds=seeds, delta_lights=True, params=p)
        assert (_bits(m2_on) == _bits(m2_off)).all() and np.abs(off).max() < 8.0
        diff = on.astype(np.float64) - off.astype(np.float64)
        for i in (0, 1):
            w = to_light[i].astype(F)
            E = _direct(light, pos32[i], w).astype(np.float64)
            want = E[None, :] * probe_ref.basis(w).astype(np.float64)[:, None]
            assert (E > 0).all()
            rel = np.abs(diff[i] - want).max() / np.abs(want).max()
            print(f"[probe] {kind} probe {i}: largest coefficient {np.abs(want).max():.4f}, relative error {rel:.2e}")
            assert rel <= 1e-5
            assert (np.sign(diff[i, 1:4]) == np.sign(want[1:4])).all() and (np.abs(want[1:]) > 0).all()
        if kind == "spot":
            ratio = _direct(light, pos32[1], to_light[1].astype(F))[0] / _direct(light, pos32[0], to_light[0].astype(F))[0]
            assert 0.02 < ratio < 0.98, "the second probe must sit in the cone's soft edge"
        assert (_bits(on[2]) == _bits(off[2])).all(), on[2]          # behind the occluder
        if kind == "spot":
            assert (_bits(on[3]) == _bits(off[3])).all(), on[3]      # facing away from the spot: Li = 0, the pair is skipped
        else:
            assert (on[3, 0] > 0).all()                              # a point light shines that way too
        # the irradiance the coefficients give for the normal that faces the light: the delta term's cosine lobe to SH's band limit
        # (bands 0 to 2 of a clamped cosine at its peak: 1/4 + 1/2 + 5/16 = 1.0625 of the true value)
        e = pt.probe_irradiance(on[:1] - off[:1], to_light[:1].astype(F), [0])[0, :3]
        E0 = _direct(light, pos32[0], to_light[0].astype(F))
        assert np.abs(e / E0 - 1.0625).max() < 1e-4, e / E0
    finally:
        pt.close()
    # under the ceiling every shadow ray ends on it behind the light, exactly as in a render of that box: the bits stay
    pt = _tracer(_box(emission=_EMISSION, lights=[light], occluder=occluder, sky=sky), 1, bounces=2)
    try:
        p = _with_bounces(pt, 2)
        off, m2_off = pt.probe_sh(pos32, spp=samples, seeds=seeds, delta_lights=False, params=p)
        on, m2_on = pt.probe_sh(pos32, spp=samples, seeds=seeds, delta_lights=True, params=p)
        assert (off[:, 0, :] > 0).all()
        assert (_bits(on) == _bits(off)).all() and (_bits(m2_on) == _bits(m2_off)).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. band 1 against the gather: E(+a) - E(-a) is the integral of L (w . a), which is sh[band 1, axis a] / 0.48860251 -- exactly
# ---------------------------------------------------------------------------------------------------------------------------
def test_band_one_against_the_gather():
    n = 16384
    P = np.array([(0.25, 0.8, -0.3)], F)
    pt = _tracer(_box(emission=_EMISSION), 1, bounces=3)
    try:
        # the gather counts the receiver as the first bounce: its gather ray carries what the probe's ray carries with one bounce less
        sh, m2 = pt.probe_sh(P, spp=n, seeds=[901], delta_lights=False, params=_with_bounces(pt, 2))
        # Var(sh[k]) = (4 PI)^2 Var(L Y_k) / n <= (4 PI)^2 * 0.48860251^2 * (m2 / n) / n, since |Y_k| <= 0.48860251 in band 1 and
        # m2 / n is the mean of lum(L)^2; dividing the coefficient by 0.48860251 leaves (4 PI)^2 m2 / n^2
        var_probe = (4.0 * math.pi) ** 2 * float(m2[0]) / n ** 2
        for axis, k in ((0, 3), (1, 1), (2, 2)):                 # Y3 = x, Y1 = y, Y2 = z
            a = np.zeros((1, 3), F)
            a[0, axis] = 1.0
            plus = pt.irradiance(P, a, spp=n, seeds=[902 + axis], params=_with_bounces(pt, 3))[0]
            minus = pt.irradiance(P, -a, spp=n, seeds=[912 + axis], params=_with_bounces(pt, 3))[0]
            lum = [float(probe_ref.luminance(e[:3])) for e in (plus, minus)]
            var = [(float(e[3]) - n * l * l) / (n - 1) / n for e, l in zip((plus, minus), lum)]       # of the mean
            got = float(probe_ref.luminance(sh[0, k])) / 0.48860251
            tol = 5.0 * math.sqrt(var[0] + var[1] + var_probe)
            print(f"[probe] axis {axis}: E(+a) - E(-a) = {lum[0] - lum[1]:+.4f}, sh / 0.4886 = {got:+.4f}, tolerance {tol:.4f}")
            assert abs((lum[0] - lum[1]) - got) <= tol
        assert abs(float(probe_ref.luminance(sh[0, 1]))) / 0.48860251 > 0.2, "the ceiling patch must show in the y coefficient"
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. invariants, without tolerance
# ---------------------------------------------------------------------------------------------------------------------------
def test_invariants():
    import torch
    scene = scenes.material_zoo(env_map=(64, 32))
    n, samples = 37, 70
    pt = _tracer(scene, 1, bounces=3)
    try:
        p = pt.params(seed=0)
        pos = _camera_probes(scene, n)
        seeds = (np.arange(n, dtype=np.uint32) * 2654435761 + 99).astype(np.uint32)
        lights = int(scene.lights.shape[0])
        pt.set_stats_level(1)
        counted = {}
        for flag in (False, True):
            pt.reset_stats()
            counted[flag] = pt.probe_sh(pos, spp=samples, seeds=seeds, delta_lights=flag, params=p)
            pt.synchronize()
            st = pt.stats().as_dict()
            assert st["paths"] == n * samples and st["pixelsWritten"] == 0 and st["pixelsRead"] == 0, st
            counted[flag] += (st["shadowRays"],)
        pt.set_stats_level(0)
        print(f"[probe] {lights} lights: shadowRays {counted[False][2]} without the flag, {counted[True][2]} with it")
        assert counted[True][2] - counted[False][2] == n * lights
        full, full_m2 = counted[True][:2]
        assert full.shape == (n, 9, 3) and np.isfinite(full).all() and (full[:, 0, :] > 0).all() and (full_m2 > 0).all()
        # a permuted list gives permuted results
        perm = np.random.default_rng(7).permutation(n)
        sh, m2 = pt.probe_sh(pos[perm], spp=samples, seeds=seeds[perm], params=p)
        assert (_bits(sh) == _bits(full[perm])).all() and (_bits(m2) == _bits(full_m2[perm])).all()
        # the device variant equals the host variant; nothing past count is written
        dev = f"cuda:{pt.device}"
        d_sh, d_m2 = pt.probe_sh(torch.from_numpy(pos).to(dev), spp=samples, seeds=torch.from_numpy(seeds.astype(np.int64)).to(dev), params=p)
        assert d_sh.is_cuda and (_bits(d_sh.cpu().numpy()) == _bits(full)).all() and (_bits(d_m2.cpu().numpy()) == _bits(full_m2)).all()
        rows = torch.from_numpy(plugin.probe_rows(pos, seeds)).to(dev)
        out = torch.full((n, 28), -123.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        plugin.check(pt.lib.PTProbeSH(pt.ctx, C.byref(p), rows.data_ptr(), 30, 0, samples, abi.PT_PROBE_DELTA_LIGHTS, out.data_ptr()))
        pt.synchronize()
        out = out.cpu().numpy()
        assert (_bits(out[:30, :27]) == _bits(full[:30].reshape(30, 27))).all() and (_bits(out[:30, 27]) == _bits(full_m2[:30])).all()
        assert (out[30:] == F(-123.25)).all()
        # schedules
        for s in (2, 3):
            pt.set_schedule(s)
            sh, m2 = pt.probe_sh(pos, spp=samples, seeds=seeds, params=p)
            assert (_bits(sh) == _bits(full)).all() and (_bits(m2) == _bits(full_m2)).all(), s
        pt.set_schedule(1)
        # evaluation: the device equals the host twin bit for bit; an index out of range gives zeros
        rng = np.random.default_rng(3)
        q = 1000
        nrm = rng.normal(0, 1, (q, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
        idx = rng.integers(0, n, q).astype(np.uint32)
        idx[5], idx[6], idx[999] = n, 0xFFFFFFFF, 0x80000000
        E = pt.probe_irradiance(full, nrm, idx)
        assert E.shape == (q, 4) and (_bits(E) == _bits(plugin.probe_irradiance(full, nrm, idx))).all()
        assert (E[[5, 6, 999]] == 0).all() and (E[:, 3] == 0).all() and (np.abs(E[:, :3]).max(axis=1) > 0).sum() == q - 3
        d_E = pt.probe_irradiance(d_sh, torch.from_numpy(nrm).to(dev), torch.from_numpy(idx.astype(np.int64)).to(dev))
        assert d_E.is_cuda and (_bits(d_E.cpu().numpy()) == _bits(E)).all()
    finally:
        pt.close()


def test_chunks():
    """130 probes x 16,384 samples = two launch sequences of 128 and 2 probes, against two lists of 65"""
    scene = scenes.material_zoo(env_map=(64, 32))
    n, samples = 130, 16384
    pt = _tracer(scene, 1, bounces=2)
    try:
        p = _with_bounces(pt, 2)
        pos = _camera_probes(scene, n)
        seeds = np.arange(n, dtype=np.uint32) + 1000
        whole, whole_m2 = pt.probe_sh(pos, spp=samples, seeds=seeds, params=p)
        parts = [pt.probe_sh(pos[k:k + 65], spp=samples, seeds=seeds[k:k + 65], params=p) for k in (0, 65)]
        assert (_bits(whole) == _bits(np.concatenate([s for s, _ in parts]))).all()
        assert (_bits(whole_m2) == _bits(np.concatenate([m for _, m in parts]))).all()
        assert np.isfinite(whole).all() and (whole[:, 0, :] > 0).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    lib = plugin.load_library()
    pos = _BOX_PROBES
    pt = _tracer(_box(), 1)
    try:
        p = pt.params(seed=0)

        def code(fn):
            with pytest.raises(plugin.PluginError) as e:
                fn()
            return e.value.code, str(e.value)

        for schedule in (0, 4):
            pt.set_schedule(schedule)
            c, msg = code(lambda: pt.probe_sh(pos, spp=2, params=p))
            assert c == abi.PT_ERR_UNSUPPORTED and f"schedule {schedule}" in msg, msg
            assert pt.probe_rays(pos, spp=2, params=p).shape == (10, 8)                     # needs no scene and no schedule
        pt.set_schedule(1)
        for bad in (0, 65537):
            assert code(lambda: pt.probe_sh(pos, spp=bad, params=p))[0] == abi.PT_ERR_UNSUPPORTED
            assert code(lambda: pt.probe_rays(pos, spp=bad, params=p))[0] == abi.PT_ERR_UNSUPPORTED
        assert pt.probe_sh(pos, spp=65536, params=p)[0].shape == (5, 9, 3)
        q = _with_bounces(pt, 8192)
        assert code(lambda: pt.probe_sh(pos, spp=2, params=q))[0] == abi.PT_ERR_UNSUPPORTED
        sh, m2 = pt.probe_sh(pos[:0], spp=2, params=p)                                      # count == 0 -> PT_OK
        assert sh.shape == (0, 9, 3) and m2.shape == (0,)
        rows = plugin.probe_rows(pos)
        out = np.empty((5, 28), F)
        assert lib.PTProbeSHHost(pt.ctx, C.byref(p), rows.ctypes.data, 5, 0, 2, 2, out.ctypes.data) == abi.PT_ERR_INVALID_ARG
        assert b"flag" in lib.PTGetLastError()
        assert lib.PTProbeSH(pt.ctx, C.byref(p), 16, 5, 0, 2, 0x80000001, 32) == abi.PT_ERR_INVALID_ARG and b"flag" in lib.PTGetLastError()
        assert lib.PTProbeSH(pt.ctx, C.byref(p), None, 5, 0, 2, 0, None) == abi.PT_ERR_INVALID_ARG
        assert lib.PTProbeSH(pt.ctx, None, 16, 5, 0, 2, 0, 32) == abi.PT_ERR_INVALID_ARG
        assert lib.PTProbeSH(pt.ctx, C.byref(p), 8, 5, 0, 2, 0, 16) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
        assert lib.PTProbeRays(pt.ctx, C.byref(p), 16, 5, 0, 2, 8) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
        assert lib.PTProbeIrradiance(pt.ctx, 16, 1, 8, 4, 32) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
        assert lib.PTProbeIrradiance(pt.ctx, 16, 1, None, 4, 32) == abi.PT_ERR_INVALID_ARG
        assert lib.PTProbeIrradiance(pt.ctx, 16, 1, 32, 0, 48) == abi.PT_OK                 # count == 0 launches nothing
    finally:
        pt.close()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    try:
        rows = plugin.probe_rows(pos)
        out = np.empty((5, 28), F)
        assert lib.PTProbeSHHost(ctx, C.byref(p), rows.ctypes.data, 5, 0, 2, 0, out.ctypes.data) == abi.PT_ERR_NO_SCENE
    finally:
        lib.PTDestroy(ctx)
