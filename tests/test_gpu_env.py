"""HAS_ENVIRONMENT_TEXTURE at its edges, on the MI355X: pt_device.h's environment functions inside a kernel, and whole frames, against
the oracle over the maps and inputs of tests/env_cases.py (black, one-hot, 1 x 1, one row, one column, odd sizes, inf / NaN / negative /
subnormal texels; rotations outside [0, 1); draws that land on a CDF entry or on the sum).

libpt-env-probe.so (csrc/env_probe.hip, `make env-probe`; test-only) holds one kernel, one element per lane, compiled twice: unit 0 with
the flags of the product's kernels, unit 1 with those of the default schedule's unit.  It calls env_sample_level, env_binary_search,
eval_env_map and sample_env_map themselves and uploads the CDF PTSetScene uploads (csrc/pt_env_cdf.h).

The contract is math_cases': where the oracle's result is not a NaN the device's bits equal it, the sign of a zero included; where it
is a NaN the device's is a NaN.  The device has no tolerance of its own: what the oracle is held to on the CPU (tests/test_env.py)
carries over through bit equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import env_cases as ec
import math_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
LIB = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib")
PROBE = os.path.join(LIB, "libpt-env-probe.so")
STRESS = {"stress": os.path.join(LIB, "libpt-stress-small-stacks.so"), "stress-repack": os.path.join(LIB, "libpt-stress-repack.so")}

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
PER_OUT = {0: 1, 1: 2, 2: 4, 3: 8, 4: 3}
PER_IN = {0: 1, 1: 1, 2: 3, 3: 1, 4: 2}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. function level: both units of the probe against the oracle, every map, every input
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device():
    """device(unit, what, name, rotation) -> (n, PER_OUT[what]) float32 over env_cases.inputs(what, name), through PTEnvProbe"""
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-C", CSRC, "env-probe"], stdout=subprocess.DEVNULL)
    import torch  # noqa: F401  -- the frame tests below hand torch buffers over: its copy of the HIP runtime has to load first (plugin.load_library)
    lib = C.CDLL(PROBE)
    lib.PTEnvProbe.restype = C.c_int
    lib.PTEnvProbe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_uint64, C.c_void_p]

    def run(unit, what, name, rotation=0.0):
        texels = np.ascontiguousarray(ec.maps()[name], dtype=F32)
        h, w = texels.shape[:2]
        vin = np.arange(w * h, dtype=F32) if what == 0 else np.ascontiguousarray(ec.inputs(what, name))
        assert vin.dtype == (U32 if what == 3 else F32) and vin.size % PER_IN[what] == 0
        n = vin.size // PER_IN[what]
        assert n <= ec.N_MAX
        out = np.full((n, PER_OUT[what]), -123.25, dtype=F32)
        err = lib.PTEnvProbe(unit, what, texels.ctypes.data, w, h, rotation, vin.ctypes.data, n, out.ctypes.data)
        assert err == 0, f"PTEnvProbe(unit {unit}, what {what}, {name}, n {n}) returned hipError {err}"
        return out
    return run


def _assert_equals_the_oracle(label, what, name, got, want):
    """bit for bit, a NaN matched by any NaN; the report names the element's first input word and its output word"""
    vin = np.arange(len(want), dtype=F32) if what == 0 else ec.inputs(what, name)
    first = np.ascontiguousarray(vin).view(U32).reshape(len(want), -1)[:, 0]
    x = np.repeat(first, PER_OUT[what])
    y = np.tile(np.arange(PER_OUT[what], dtype=U32), len(want))
    mc.assert_same_bits(label, x, y, _bits(got).ravel(), _bits(want).ravel(), "device", "oracle")


@pytest.mark.parametrize("name", ec.MAP_NAMES)
def test_device_functions_equal_the_oracle(name, device, oracle):
    """what 0 to 4 on both units.  eval_env_map runs at each of the six rotations, sample_env_map at three (its rotation only turns
    the direction); env_sample_level and the search take no rotation.  In a report x is the element's first input word, y the
    index of the output word."""
    runs = [(0, 0.0), (1, 0.0), (4, 0.0)] + [(2, r) for r in ec.ROTATIONS] + [(3, r) for r in (0.0, -0.35, 1.75)]
    for what, rotation in runs:
        want, _ = ec.oracle_probe(name, what, rotation)
        for unit in (0, 1):
            got = device(unit, what, name, rotation)
            assert got.shape == want.shape
            _assert_equals_the_oracle(f"{name} what {what} rotation {rotation} unit {unit}", what, name, got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. frames: fuzzed scenes under every map and every sky setting, every schedule
# ---------------------------------------------------------------------------------------------------------------------------
N_SEEDS = 32
W, H, SPP = 48, 32, 3
SKY_KINDS = ("map", "no map", "mode 1 with a map", "mode 2")


def _fuzz_env_scene(seed):
    """test_gpu_parity._fuzz_scene(1000 + seed) with the sky redrawn.  Seeds below len(MAP_NAMES) get mode 0 with the map of their
    number, so every map of env_cases is rendered; the others take turns with mode 0 without a map, mode 1 with a map set (which
    must be ignored) and mode 2 (no sky at all: both branches of sample_sky_radiance fall through).  Rotation and intensity are
    drawn.  Returns (scene, sky kind, map name or None)."""
    from test_gpu_parity import _fuzz_scene
    s = _fuzz_scene(1000 + seed)
    rng = np.random.RandomState(5000 + seed)
    if seed < len(ec.MAP_NAMES):
        kind, name = "map", ec.MAP_NAMES[seed]
    else:
        kind = SKY_KINDS[1 + (seed - len(ec.MAP_NAMES)) % 3]
        name = ec.MAP_NAMES[int(rng.randint(0, len(ec.MAP_NAMES)))] if kind == "mode 1 with a map" else None
    s.environment_mode = {"map": 0, "no map": 0, "mode 1 with a map": 1, "mode 2": 2}[kind]
    s.environment_texture = None if name is None else np.array(ec.maps()[name])
    s.environment_map_rotation = float(rng.choice(ec.FRAME_ROTATIONS))
    s.environment_intensity = float(rng.choice([0.0, 1.0, rng.uniform(0.2, 2.0)]))
    return s, kind, name


def _seed_of(name):
    return ec.MAP_NAMES.index(name)


def _fuzz_params(s, seed, spp=SPP):
    from unity_webgpu_pathtracer_amd import scenes
    return scenes.frame_params(s, W, H, spp=spp, seed=0xE57 + seed, max_bounces=1 + seed % 5, russian_roulette=seed % 2 == 0,
                               firefly=seed % 2 == 1, max_firefly_luminance=4.0)


_oracle_frames = {}


def _oracle_fuzz_frame(oracle, seed, spp=SPP):
    """the oracle's frame and counters of a seed: computed once, shared by the tests that need it (the CPU-built BVH is the same)"""
    from unity_webgpu_pathtracer_amd.pathtracer import BVHScene
    if (seed, spp) not in _oracle_frames:
        s, _, _ = _fuzz_env_scene(seed)
        ref, st = oracle.render(oracle.buffers_from_bvhscene(BVHScene(s)), _fuzz_params(s, seed, spp), shadow_any_hit=True)
        ref.setflags(write=False)
        _oracle_frames[(seed, spp)] = (ref, st)
    return _oracle_frames[(seed, spp)]


def _assert_frame(what, gpu, ref):
    """the NaN pattern, then the bits (of a NaN pixel the pattern is the contract)"""
    assert gpu.shape == ref.shape
    nan_g, nan_r = np.isnan(gpu), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), f"{what}: NaN pattern differs in {int((nan_g != nan_r).any(axis=-1).sum())} pixels"
    bad = ((_bits(gpu) != _bits(ref)) & ~nan_r).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first {tuple(int(v) for v in np.argwhere(bad)[0])}"


def _render(pt, p):
    import torch
    out = torch.zeros((p.OutputHeight, p.OutputWidth, 4), dtype=torch.float32, device=f"cuda:{pt.device}")
    torch.cuda.synchronize()
    pt.render_pass_to(p, out.data_ptr(), 0)
    pt.synchronize()
    return out.cpu().numpy()


def test_generator_covers_every_map_and_every_sky_kind():
    got = [_fuzz_env_scene(seed) for seed in range(N_SEEDS)]
    assert {name for _, kind, name in got if kind == "map"} == set(ec.MAP_NAMES)
    assert {kind for _, kind, _ in got} == set(SKY_KINDS)
    for s, kind, name in got:
        assert (s.environment_texture is not None) == (kind in ("map", "mode 1 with a map")) and (s.features & 8 != 0) == (name is not None)
    assert {s.environment_map_rotation for s, _, _ in got} == set(ec.FRAME_ROTATIONS)
    assert {0.0, 1.0} < {s.environment_intensity for s, _, _ in got}


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_fuzzed_env_scenes_bit_exact(oracle, seed):
    """48 x 32 at 3 spp, bounces 1 + seed % 5, Russian roulette and the firefly filter on alternate seeds, schedules 0 to 4 on one
    context: every frame and all 16 counters equal the oracle's."""
    from test_gpu_parity import ALL_COUNTERS, _stats_equal
    from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
    s, kind, name = _fuzz_env_scene(seed)
    ref, st = _oracle_fuzz_frame(oracle, seed)
    p = _fuzz_params(s, seed)
    pt = PathTracer(s, width=W, height=H, samplesPerPass=SPP, maxRayBounces=1 + seed % 5)
    try:
        pt.set_stats_level(1)
        for schedule in range(5):
            pt.set_schedule(schedule)
            pt.reset_stats()
            gpu = _render(pt, p)
            _assert_frame(f"seed {seed} ({kind}, {name}), schedule {schedule}", gpu, ref)
            _stats_equal(pt.stats(), st, ALL_COUNTERS)
    finally:
        pt.close()


@pytest.mark.parametrize("name", ["black_w8h4", "w1h1", "hot_interior", "w5h3"])
def test_instanced_scene_under_edge_maps(oracle, name):
    """HAS_TLAS + HAS_ENVIRONMENT_TEXTURE: the environment shadow ray through the two-level walk, schedules 0 and 1."""
    from test_gpu_parity import ALL_COUNTERS, _stats_equal
    from unity_webgpu_pathtracer_amd import scenes
    from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
    s = scenes.instanced_scene(count=9, detail=6)
    s.environment_texture = np.array(ec.maps()[name])
    s.environment_map_rotation, s.environment_intensity = -0.35, 1.0
    assert s.environment_mode == 0 and s.features & 0xC == 0xC
    pt = PathTracer(s, width=64, height=40, samplesPerPass=2)
    try:
        pt.set_stats_level(1)
        p = pt.params(seed=0x7E4A)
        ref, st = oracle.render(oracle.buffers_from_bvhscene(pt._bvhScene), p, shadow_any_hit=True)
        for schedule in (0, 1):
            pt.set_schedule(schedule)
            pt.reset_stats()
            _assert_frame(f"instanced under {name}, schedule {schedule}", _render(pt, p), ref)
            _stats_equal(pt.stats(), st, ALL_COUNTERS)
    finally:
        pt.close()


# ---- the stress builds: small traversal stacks (every ray through the slab), a slot repack after every iteration --------------------
STRESS_SEEDS = (_seed_of("black_w8h4"), _seed_of("hot_col_last"))      # the one-hot seed whose drawn intensity is not 0

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
from test_gpu_env import STRESS_SEEDS, W, H, SPP, _fuzz_env_scene, _fuzz_params, _render
out = {}
for seed in STRESS_SEEDS:
    s, kind, name = _fuzz_env_scene(seed)
    pt = PathTracer(s, width=W, height=H, samplesPerPass=SPP, maxRayBounces=1 + seed % 5, schedule=1)
    pt.set_stats_level(1)
    out[f"frame{seed}"] = _render(pt, _fuzz_params(s, seed))
    st = pt.stats().as_dict()
    out[f"stats{seed}"] = np.array([st[k] for k in sorted(st)], dtype=np.uint64)
    pt.close()
np.savez(sys.argv[2], **out)
'''


@pytest.mark.parametrize("build", sorted(STRESS))
def test_stress_builds_carry_the_environment_ray(oracle, build, tmp_path):
    """Under the black map every environment shadow ray is traced and adds nothing (valid == 2); under the one-hot map nearly all of
    them carry a contribution.  A slab, or a slot repack, that lost that state would change the frame or the shadow-ray counters.
    Both seeds rendered by the variant library in one fresh child process, the default schedule."""
    from test_gpu_parity import ALL_COUNTERS
    if not os.path.exists(STRESS[build]):
        subprocess.check_call(["make", "-C", CSRC, build], stdout=subprocess.DEVNULL)
    out = str(tmp_path / "frames.npz")
    subprocess.check_call([sys.executable, "-c", CHILD, ROOT, out], env=dict(os.environ, PT_PLUGIN=STRESS[build]), timeout=300)
    got = np.load(out)
    for seed in STRESS_SEEDS:
        ref, st = _oracle_fuzz_frame(oracle, seed)
        _assert_frame(f"{build}, seed {seed}", got[f"frame{seed}"], ref)
        want = st.as_dict()
        stats = dict(zip(sorted(want), (int(v) for v in got[f"stats{seed}"])))
        bad = {k: (stats[k], want[k]) for k in ALL_COUNTERS if stats[k] != want[k]}
        assert not bad, f"{build}, seed {seed}: counter mismatch (gpu, oracle): {bad}"
        assert want["shadowRays"] > 0


# ---- radiance queries under edge maps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["black_w8h4", "hot_row0", "w1h1", "one_inf_texel"])
def test_camera_rays_then_radiance_is_the_frame(oracle, name):
    """tests/test_gpu_radiance.py's invariant under edge maps: the camera's rays traced as a list give the 1-spp frame of
    PTRenderPassTo, which is the oracle's."""
    from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
    seed = _seed_of(name)
    s, _, _ = _fuzz_env_scene(seed)
    ref, _ = _oracle_fuzz_frame(oracle, seed, spp=1)
    p = _fuzz_params(s, seed, spp=1)
    pt = PathTracer(s, width=W, height=H, samplesPerPass=1, maxRayBounces=1 + seed % 5, schedule=1)
    try:
        rays = pt.camera_rays(params=p)
        got = pt.radiance(rays, spp=1, params=p)
        frame = _render(pt, p)
        _assert_frame(f"frame under {name}", frame, ref)
        _assert_frame(f"radiance under {name}", got[:, :3].reshape(H, W, 3), frame[..., :3])
    finally:
        pt.close()


# ---- sky pixels under a constant map ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["constant_grey", "constant_colour"])
def test_escaping_camera_rays_see_the_texel(name):
    """Under a constant map a pixel whose camera ray escapes is the texel, exactly: a + t (a - a) at whatever direction and rotation, and
    depth 0 takes intensity 1 whatever EnvironmentIntensity says.  The escaping pixels are the misses of trace_rays over the
    camera's own rays; the scene's analytic lights are taken out (a rectangle light in the way is a hit trace_rays does not see)."""
    from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
    seed = _seed_of(name)
    s, _, _ = _fuzz_env_scene(seed)
    s.lights = np.zeros((0, 16), dtype=F32)
    s.camera.vfov_deg = 70.0                                     # wide enough to look past the back wall
    s.environment_intensity = 0.37
    texel = ec.maps()[name][0, 0, :3]
    for rotation in ec.FRAME_ROTATIONS:
        s.environment_map_rotation = rotation
        p = _fuzz_params(s, seed, spp=1)
        p.UseFireflyFilter = 0
        pt = PathTracer(s, width=W, height=H, samplesPerPass=1, maxRayBounces=1 + seed % 5, schedule=1)
        try:
            rays = pt.camera_rays(params=p)
            q = rays.copy()
            q[:, 6], q[:, 7] = F32(1.0e5), F32(0.0)
            hits = pt.trace_rays(q)
            miss = (_bits(hits[:, 3]) == 0xFFFFFFFF).reshape(H, W)
            assert 50 < miss.sum() < W * H - 50, int(miss.sum())
            frame = _render(pt, p)
            assert (_bits(frame[miss][:, :3]) == _bits(texel)[None, :]).all(), (name, rotation)
            assert (_bits(frame[~miss][:, :3]) != _bits(texel)[None, :]).any()
        finally:
            pt.close()
