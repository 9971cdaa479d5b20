"""Irradiance gathers (PTGatherIrradiance / PTGatherIrradianceHost / PTGatherRays, include/ptmi_plugin.h Part 13) on the MI355X.

The rule is bit-exact and most of these tests hold it without tolerances: a gather's continuation is the radiance query of its
gather ray, a list's results depend neither on its order, its length, the split of its sample range, the schedule nor on how it is
cut into chunks.  Only the closed form of the direct light has a tolerance (1e-5 relative: fewer than twenty fp32 roundings)."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import gather_ref

pytestmark = pytest.mark.gpu

F = np.float32
PI = gather_ref.PI
SEED0 = 0x1234


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def _box(emission=(0.0, 0.0, 0.0), lights=(), occluder=None, ceiling=True, sky="basic"):
    """A CLOSED Cornell shell (scenes._cornell_shell plus ceiling and front wall), every material of roughness 1.  emission: a
    1.2 x 1.2 ceiling patch with an emissive MATERIAL (no analytic light).  Basic sky of intensity 0: no environment NEE, and
    nothing to see anyway (an escaping ray adds exactly 0).  ceiling=False leaves the ceiling and its patch off: the render's
    shadow rays have no far end (util/light.hlsl:99), so a light that geometry encloses lights nothing -- the reason the
    project's own Cornell box has no ceiling."""
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
    s = scenes.Scene("gather_box", verts, attrs, np.stack(mats), L, np.zeros(0, dtype=np.uint32),
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


def _box_receivers(n, seed=3):
    """n receivers on the floor and the four walls of the box, normals pointing inwards"""
    rng = np.random.default_rng(seed)
    faces = [((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0)), ((-1, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, -1)),
             ((-1, 0, -1), (0, 0, 2), (0, 2, 0), (1, 0, 0)), ((1, 0, -1), (0, 0, 2), (0, 2, 0), (-1, 0, 0)),
             ((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1))]
    which = rng.integers(0, len(faces), n)
    uv = rng.uniform(0.02, 0.98, (n, 2))
    pos = np.array([np.asarray(faces[w][0], float) + u * np.asarray(faces[w][1], float) + v * np.asarray(faces[w][2], float)
                    for w, (u, v) in zip(which, uv)], dtype=F)
    nrm = np.array([faces[w][3] for w in which], dtype=F)
    return pos, nrm


def _tracer(scene, schedule=1, bounces=3):
    return PathTracer(scene, width=64, height=48, samplesPerPass=1, maxRayBounces=bounces, schedule=schedule)


def _with_bounces(pt, bounces):
    p = pt.params(seed=0)
    p.MaxRayBounces = bounces
    return p


def _all_hit(pt, rays):
    q = rays.copy()
    q[:, 6], q[:, 7] = F(1.0e5), F(0.0)
    hits = pt.trace_rays(q)
    return (_bits(hits[:, 3]) != 0xFFFFFFFF) & (hits[:, 0] < F(1.0e5))


def _fold(parts):
    """rgb and m2 of one call from its samples' one-sample results, in the rule's order"""
    n = len(parts)
    rgb, m2 = parts[0][:, :3].copy(), parts[0][:, 3].copy()
    for e in parts[1:]:
        rgb, m2 = rgb + e[:, :3], m2 + e[:, 3]
    return np.concatenate([rgb / F(n), m2[:, None]], axis=1).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the continuation is the radiance query, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [1, 2, 3])
def test_continuation_is_the_radiance_query(schedule):
    n, samples = 300, 5
    pos, nrm = _box_receivers(n)
    seeds = (np.arange(n, dtype=np.uint32) * 7919 + SEED0).astype(np.uint32)
    pt = _tracer(_box(emission=(6.0, 5.0, 3.0)), schedule, bounces=3)
    try:
        p3, p2 = _with_bounces(pt, 3), _with_bounces(pt, 2)
        assert p3.UseRussianRoulette == 1
        rays = pt.gather_rays(pos, nrm, spp=samples, seeds=seeds, params=p3)
        assert rays.shape == (n * samples, 8) and not np.isnan(rays[:, :6]).any()          # (column 6 is RNG bits)
        hit = _all_hit(pt, rays)
        assert hit.all(), f"{int((~hit).sum())} gather rays leave the closed box"
        rad = pt.radiance(rays, spp=1, params=p2)
        parts = []
        for j in range(samples):
            e = pt.irradiance(pos, nrm, spp=1, first_sample=j, seeds=seeds, params=p3)
            want = rad[j::samples, :3] * PI
            bad = int((_bits(e[:, :3]) != _bits(want)).any(axis=1).sum())
            print(f"[gather] schedule {schedule} sample {j}: {bad} of {n} entries differ from PI x the radiance of their gather ray")
            assert bad == 0
            lum = gather_ref.luminance(want)
            assert (_bits(e[:, 3]) == _bits(lum * lum)).all()
            parts.append(e)
        lit = np.concatenate([q[:, :3] for q in parts]).max(axis=1)
        assert (lit > 0).mean() > 0.1, "the emissive patch lights nothing: the test would compare zeros"
        five = pt.irradiance(pos, nrm, spp=samples, seeds=seeds, params=p3)
        assert (_bits(five) == _bits(_fold(parts))).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. direct light at the receiver, closed form
# ---------------------------------------------------------------------------------------------------------------------------
_LIGHT_POS = (0.2, 1.6, 0.1)
_LIGHTS = {
    "point": scenes.pack_point_light(_LIGHT_POS, (1.0, 0.8, 0.6), intensity=5.0, rng=10.0),
    # aimed at the first receiver (inside the inner cone); the other three sit in the soft edge between 20 and 60 degrees
    "spot": scenes.pack_spot_light(_LIGHT_POS, (-0.5, -1.0, -0.3), 120.0, 40.0, (0.6, 0.8, 1.0), intensity=7.0, rng=12.0),
}


# the sky: the box's own basic sky of intensity 0, and an all-black environment map -- an extra draw and an extra traced ray per
# receiver that add nothing; every sample of a point or spot light has the same value, so the shifted draws cannot move the result
_SKIES = [pytest.param("point", "basic", id="point"), pytest.param("spot", "basic", id="spot"),
          pytest.param("point", "black map", id="point-black-map"), pytest.param("spot", "black map", id="spot-black-map")]


@pytest.mark.parametrize("kind,sky", _SKIES)
def test_direct_light_closed_form(kind, sky):
    light = _LIGHTS[kind]
    lp = np.asarray(_LIGHT_POS, dtype=np.float64)
    pos = np.array([(-0.3, 0.6, -0.2), (0.5, 0.5, -0.3), (0.4, 0.7, 0.3), (0.6, 0.4, 0.5)], dtype=np.float64)
    to_light = (lp - pos) / np.linalg.norm(lp - pos, axis=1, keepdims=True)
    tilt = to_light[1] + np.array([0.9, 0.1, -0.4])
    nrm = np.stack([to_light[0], tilt / np.linalg.norm(tilt), -to_light[2], to_light[3]])
    # an occluder quad halfway between the light and the last receiver, facing both
    mid = 0.5 * (lp + pos[3])
    a = np.cross(to_light[3], (0.0, 1.0, 0.0)); a /= np.linalg.norm(a)
    b = np.cross(to_light[3], a)
    occluder = (tuple(mid - 0.2 * a - 0.2 * b), tuple(0.4 * a), tuple(0.4 * b), tuple(to_light[3]))
    pos, nrm = pos.astype(F), nrm.astype(F)
    samples, seeds = 8, np.arange(4, dtype=np.uint32) + 11
    # Under the ceiling every shadow ray ends on it behind the light, exactly as in a render of that box: E is 0 everywhere.
    pt = _tracer(_box(lights=[light], occluder=occluder, sky=sky), 1, bounces=1)
    try:
        assert (pt.irradiance(pos, nrm, spp=samples, seeds=seeds, params=_with_bounces(pt, 1)) == 0).all()
    finally:
        pt.close()
    # The dark box with its top open (all four lines to the light leave through it): the closed form.
    pt = _tracer(_box(lights=[light], occluder=occluder, ceiling=False, sky=sky), 1, bounces=1)
    try:
        out = pt.irradiance(pos, nrm, spp=samples, seeds=seeds, params=_with_bounces(pt, 1))
        want = np.stack([gather_ref.direct_irradiance(light, pos[i], nrm[i]) for i in range(4)])
        print(f"[gather] {kind}: E = {out[:, :3].tolist()}  closed form (unoccluded) = {want.tolist()}")
        assert (want[0] > 0).all() and (want[1] > 0).all() and (want[3] > 0).all() and (want[2] == 0).all()
        assert 0.05 < want[1].max() / want[0].max() < 0.95, "the tilted receiver must differ visibly from the facing one"
        for i in (0, 1):
            rel = np.abs(out[i, :3].astype(np.float64) - want[i]) / want[i]
            print(f"[gather] {kind} receiver {i}: relative error {rel.max():.2e}")
            assert rel.max() <= 1e-5
            # every sample has the same value: the sample variance from m2 is 0 up to rounding
            lum = float(gather_ref.luminance(out[i, :3]))
            var = (float(out[i, 3]) - samples * lum * lum) / (samples - 1)
            assert abs(var) <= 1e-5 * lum * lum, (var, lum)
        assert (out[2] == 0).all(), out[2]           # facing away
        assert (out[3] == 0).all(), out[3]           # behind the occluder
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. invariants, without tolerance
# ---------------------------------------------------------------------------------------------------------------------------
def _surface_receivers(pt, n):
    """the first n first hits of the tracer's camera rays: position, and the normal turned towards the camera"""
    rays = pt.camera_rays(seed=5)
    q = rays.copy()
    q[:, 6], q[:, 7] = F(1.0e5), F(0.0)
    hits, surf = pt.trace_rays(q, surface=True)
    ok = np.nonzero(_bits(hits[:, 3]) != 0xFFFFFFFF)[0]
    assert len(ok) >= n, len(ok)
    ok = ok[np.linspace(0, len(ok) - 1, n).astype(np.int64)]
    pos, nrm = surf[ok, 0:3].copy(), surf[ok, 4:7].copy()
    back = (nrm * rays[ok, 3:6]).sum(axis=1) > 0
    nrm[back] = -nrm[back]
    return pos, nrm


def _invariants(scene, schedules):
    import torch
    n, samples = 257, 5
    pt = _tracer(scene, schedules[0], bounces=3)
    try:
        p = pt.params(seed=0)
        pos, nrm = _surface_receivers(pt, n)
        seeds = (np.arange(n, dtype=np.uint32) * 2654435761 + 99).astype(np.uint32)
        pt.reset_stats()
        full = pt.irradiance(pos, nrm, spp=samples, seeds=seeds, params=p)
        pt.synchronize()
        st = pt.stats().as_dict()
        assert st["paths"] == n * samples and st["pixelsWritten"] == 0 and st["pixelsRead"] == 0, st
        assert full.shape == (n, 4) and np.isfinite(full).all() and (full >= 0).all()
        assert (full[:, :3].max(axis=1) > 0).mean() > 0.5
        # a permuted list gives permuted results
        perm = np.random.default_rng(7).permutation(n)
        assert (_bits(pt.irradiance(pos[perm], nrm[perm], spp=samples, seeds=seeds[perm], params=p)) == _bits(full[perm])).all()
        # lengths
        for k in (1, 255, 256, 257):
            assert (_bits(pt.irradiance(pos[:k], nrm[:k], spp=samples, seeds=seeds[:k], params=p)) == _bits(full[:k])).all(), k
        # one call of 5 samples = five calls of one sample
        parts = [pt.irradiance(pos, nrm, spp=1, first_sample=j, seeds=seeds, params=p) for j in range(samples)]
        assert (_bits(_fold(parts)) == _bits(full)).all()
        # ... and a call that starts in the middle of the range
        tail = pt.irradiance(pos, nrm, spp=2, first_sample=3, seeds=seeds, params=p)
        assert (_bits(_fold(parts[3:])) == _bits(tail)).all()
        # the device variant equals the host variant; nothing past count is written
        dev = f"cuda:{pt.device}"
        d_pos, d_nrm = torch.from_numpy(pos).to(dev), torch.from_numpy(nrm).to(dev)
        got = pt.irradiance(d_pos, d_nrm, spp=samples, seeds=torch.from_numpy(seeds.astype(np.int64)).to(dev), params=p)
        assert got.is_cuda and (_bits(got.cpu().numpy()) == _bits(full)).all()
        recv = torch.from_numpy(pt._receivers(pos, nrm, seeds)).to(dev)
        out = torch.full((n, 4), -123.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        plugin.check(pt.lib.PTGatherIrradiance(pt.ctx, C.byref(p), recv.data_ptr(), 200, 0, samples, out.data_ptr()))
        pt.synchronize()
        out = out.cpu().numpy()
        assert (_bits(out[:200]) == _bits(full[:200])).all() and (out[200:] == F(-123.25)).all()
        # schedules
        for s in schedules[1:]:
            pt.set_schedule(s)
            assert (_bits(pt.irradiance(pos, nrm, spp=samples, seeds=seeds, params=p)) == _bits(full)).all(), s
    finally:
        pt.close()


def test_invariants():
    _invariants(scenes.material_zoo(env_map=(64, 32)), [1, 2, 3])


def test_invariants_instanced():
    _invariants(scenes.instanced_scene(), [1])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. chunking: 600 x 4,096 samples = two launch sequences of 512 and 88 entries
# ---------------------------------------------------------------------------------------------------------------------------
def test_chunks():
    n, samples = 600, 4096
    pos, nrm = _box_receivers(n, seed=4)
    pt = _tracer(_box(emission=(6.0, 5.0, 3.0)), 1, bounces=3)
    try:
        p = _with_bounces(pt, 3)
        seeds = np.arange(n, dtype=np.uint32) + 1000
        whole = pt.irradiance(pos, nrm, spp=samples, seeds=seeds, params=p)
        lists = [pt.irradiance(pos[k:k + 100], nrm[k:k + 100], spp=samples, seeds=seeds[k:k + 100], params=p) for k in range(0, n, 100)]
        assert (_bits(whole) == _bits(np.concatenate(lists))).all()
        assert np.isfinite(whole).all() and (whole[:, :3].max(axis=1) > 0).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. PTGatherRays
# ---------------------------------------------------------------------------------------------------------------------------
_RAY_SCENES = {
    "no_lights": (lambda: _box(), 2),             # the basic sky: no environment draws
    "point_light": (lambda: _box(lights=[_LIGHTS["point"]]), 3),
    "rect_light": (lambda: _box(lights=[scenes._cornell_light()]), 5),
}


@pytest.mark.parametrize("name", list(_RAY_SCENES))
def test_gather_rays(oracle, name):
    lib = oracle.load_oracle()
    make, draws = _RAY_SCENES[name]
    n, samples, first = 70, 3, 9
    pos, nrm = _box_receivers(n, seed=6)
    seeds = (np.arange(n, dtype=np.uint32) * 40503 + 0xFFFFFFF0).astype(np.uint32)
    pt = _tracer(make(), 1)
    try:
        rays = pt.gather_rays(pos, nrm, spp=samples, first_sample=first, seeds=seeds)
        assert rays.shape == (n * samples, 8) and (_bits(rays[:, 7]) == 0).all()
        rng = _bits(rays[:, 6])
        for i in range(n):
            for j in range(samples):
                s = C.c_uint32(gather_ref.sample_seed(int(seeds[i]), first, j))
                for _ in range(draws):
                    lib.oracle_random_float(C.byref(s))
                assert int(rng[i * samples + j]) == s.value, (i, j)
        d = rays[:, 3:6].astype(np.float64)
        assert not np.isnan(d).any()
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-6
        N, P = np.repeat(nrm, samples, axis=0).astype(np.float64), np.repeat(pos, samples, axis=0).astype(np.float64)
        assert ((N * d).sum(axis=1) > 0).all()
        assert np.abs(rays[:, 0:3] - (P + d * 1e-4)).max() <= 1e-6
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    lib = plugin.load_library()
    pos, nrm = _box_receivers(16)
    pt = _tracer(_box(), 1)
    try:
        p = pt.params(seed=0)

        def code(fn):
            with pytest.raises(plugin.PluginError) as e:
                fn()
            return e.value.code, str(e.value)

        for schedule in (0, 4):
            pt.set_schedule(schedule)
            c, msg = code(lambda: pt.irradiance(pos, nrm, spp=2, params=p))
            assert c == abi.PT_ERR_UNSUPPORTED and f"schedule {schedule}" in msg, msg
            assert code(lambda: pt.gather_rays(pos, nrm, spp=2, params=p))[0] == abi.PT_ERR_UNSUPPORTED
        pt.set_schedule(1)
        for bad in (0, 65537):
            assert code(lambda: pt.irradiance(pos, nrm, spp=bad, params=p))[0] == abi.PT_ERR_UNSUPPORTED
        assert pt.irradiance(pos, nrm, spp=65536, params=p).shape == (16, 4)
        q = _with_bounces(pt, 8192)
        assert code(lambda: pt.irradiance(pos, nrm, spp=2, params=q))[0] == abi.PT_ERR_UNSUPPORTED
        assert pt.irradiance(pos[:0], nrm[:0], spp=2, params=p).shape == (0, 4)             # count == 0 -> PT_OK
        recv = pt._receivers(pos, nrm, None)
        recv[5, 7:8].view(np.uint32)[0] = 1
        out = np.empty((16, 4), F)
        assert lib.PTGatherIrradianceHost(pt.ctx, C.byref(p), recv.ctypes.data, 16, 0, 2, out.ctypes.data) == abi.PT_ERR_INVALID_ARG
        assert b"receivers[5].reserved" in lib.PTGetLastError()
        assert lib.PTGatherIrradiance(pt.ctx, C.byref(p), None, 16, 0, 2, None) == abi.PT_ERR_INVALID_ARG
        assert lib.PTGatherIrradiance(pt.ctx, C.byref(p), 8, 16, 0, 2, 16) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
        assert lib.PTGatherRays(pt.ctx, C.byref(p), 16, 16, 0, 2, 8) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    finally:
        pt.close()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    try:
        recv = pt._receivers(pos, nrm, None)
        out = np.empty((16, 4), F)
        assert lib.PTGatherIrradianceHost(ctx, C.byref(p), recv.ctypes.data, 16, 0, 2, out.ctypes.data) == abi.PT_ERR_NO_SCENE
    finally:
        lib.PTDestroy(ctx)
