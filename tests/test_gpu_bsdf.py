"""The material fetch and the Disney BSDF at their edges, on the MI355X: pt_device.h's functions inside a kernel, and whole frames,
against the oracle over the materials, textures and inputs of tests/bsdf_cases.py (clamped parameters, black and over-bright base
colours, NaN / inf scalars, 1 x 1 / one-row / one-column textures, uv on texel centres and past 2^24, grazing and zero directions,
degenerate normals, draws on the lobe boundaries).

libpt-bsdf-probe.so (csrc/bsdf_probe.hip, `make bsdf-probe`; test-only) holds one kernel, one element per lane, compiled twice: unit 0
with the flags of the product's kernels, unit 1 with those of the default schedule's unit.  It calls get_material, sample_texture,
sample_textures4, the sampling helpers, tint_colors, lobe_weights, onb_of_normal, eval_brdf_onb and sample_brdf themselves, in the setting
path_shade_hit gives them.

The contract is math_cases': where the oracle's result is not a NaN the device's bits equal it, the sign of a zero included; where it
is a NaN the device's is a NaN.  The device has no tolerance of its own: what the oracle is held to on the CPU (tests/test_bsdf.py)
carries over through bit equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bsdf_cases as bc
import math_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
LIB = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib")
PROBE = os.path.join(LIB, "libpt-bsdf-probe.so")
STRESS = {"stress": os.path.join(LIB, "libpt-stress-small-stacks.so"), "stress-repack": os.path.join(LIB, "libpt-stress-repack.so")}

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. function level: both units of the probe against the oracle, every material, every input
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device():
    """device(unit, what, mi) -> (n, PER_OUT[what]) float32 over bsdf_cases.inputs(what, mi), through PTBsdfProbe"""
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-C", CSRC, "bsdf-probe"], stdout=subprocess.DEVNULL)
    import torch  # noqa: F401  -- the frame tests below hand torch buffers over: its copy of the HIP runtime has to load first (plugin.load_library)
    lib = C.CDLL(PROBE)
    lib.PTBsdfProbe.restype = C.c_int
    lib.PTBsdfProbe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    mats = np.ascontiguousarray(bc.materials(), dtype=F32)
    tex = np.ascontiguousarray(bc.texture_data(), dtype=U32)

    def run(unit, what, mi):
        vin = np.ascontiguousarray(bc.inputs(what, mi))
        assert vin.dtype == F32 and vin.shape[1] == bc.PER_IN[what] and len(vin) <= bc.N_MAX
        out = np.full((len(vin), bc.PER_OUT[what]), -123.25, dtype=F32)
        err = lib.PTBsdfProbe(unit, what, mats.ctypes.data, len(mats), tex.ctypes.data, tex.size, vin.ctypes.data, len(vin), out.ctypes.data)
        if err not in (0, 1):           # not a refused argument: the device reported an error, nothing more is started on it
            pytest.exit(f"PTBsdfProbe(unit {unit}, what {what}, {bc.block_name(what, mi)}) returned hipError {err}", returncode=3)
        assert err == 0, f"PTBsdfProbe(unit {unit}, what {what}, {bc.block_name(what, mi)}, n {len(vin)}) returned hipError {err}"
        return out
    return run


def _assert_equals_the_oracle(label, what, mi, got, want):
    """bit for bit, a NaN matched by any NaN.  A report names the block, the what, the element (x: its number; its inputs follow)
    and the output word (y)."""
    assert got.shape == want.shape
    per = bc.PER_OUT[what]
    x = np.repeat(np.arange(len(want), dtype=U32), per)
    y = np.tile(np.arange(per, dtype=U32), len(want))
    try:
        mc.assert_same_bits(label, x, y, _bits(got).ravel(), _bits(want).ravel(), "device", "oracle")
    except AssertionError as e:
        first, word = divmod(int(mc.mismatches(_bits(got).ravel(), _bits(want).ravel())[0]), per)
        vin = bc.inputs(what, mi)[first]
        field = f" (Material.{bc.MATERIAL_FIELDS[word % 24]})" if what == 0 and word < 48 else ""
        raise AssertionError(f"{e}\n  element {first} of {label}, output word {word}{field}: inputs {[float(v) for v in vin]} "
                             f"(bits {[hex(int(b)) for b in _bits(vin)]})") from None


def _check_block(device, what, mi):
    want = bc.oracle_probe(what, mi)
    for unit in (0, 1):
        got = device(unit, what, mi)
        _assert_equals_the_oracle(f"{bc.block_name(what, mi)} what {what} unit {unit}", what, mi, got, want)
        if what == 0:           # the counted and the uncounted form are one function
            bad = mc.mismatches(_bits(got[:, :24]).ravel(), _bits(got[:, 24:48]).ravel())
            assert not bad.size, f"{bc.block_name(what, mi)} unit {unit}: get_material<true> and <false> differ in {bad.size} words, first {int(bad[0])}"


@pytest.mark.parametrize("name", bc.MATERIAL_NAMES)
def test_material_and_bsdf_equal_the_oracle(name, device, oracle):
    """what 0 (get_material, both forms, and the counters of one fetch), 3 (tint_colors, lobe_weights), 4 (eval_brdf_onb in the basis of
    ffnormal and, through onb_of_normal, of normal) and 5 (sample_brdf and the RNG state it leaves) of one material, on both units."""
    for what in (0, 3, 4, 5):
        _check_block(device, what, bc.MI[name])


@pytest.mark.parametrize("name", bc.TEXTURE_NAMES)
def test_texture_lookups_equal_the_oracle(name, device, oracle):
    """what 1: sample_texture<false> and sample_textures4<false> with the texture in each of its four slots, over every uv pair."""
    _check_block(device, 1, bc.TEX[name])


@pytest.mark.parametrize("name", bc.HELPERS)
def test_helpers_equal_the_oracle(name, device, oracle):
    """what 2: one helper over math_cases' special values, its branch boundaries and its domain."""
    _check_block(device, 2, bc.HELPERS.index(name))


def test_the_probe_checks_its_arguments(device):
    """a bad unit, a bad what, an index outside the scene: hipErrorInvalidValue (1), nothing launched"""
    lib = C.CDLL(PROBE)
    mats = np.ascontiguousarray(bc.materials(), dtype=F32)
    tex = np.ascontiguousarray(bc.texture_data(), dtype=U32)
    out = np.zeros(64, dtype=F32)

    def call(unit, what, vin, mats=mats, tex_size=tex.size):
        vin = np.ascontiguousarray(vin, dtype=F32)
        return lib.PTBsdfProbe(C.c_int(unit), C.c_int(what), C.c_void_p(mats.ctypes.data), C.c_uint32(len(mats)), C.c_void_p(tex.ctypes.data),
                               C.c_uint64(tex_size), C.c_void_p(vin.ctypes.data), C.c_uint64(1), C.c_void_p(out.ctypes.data))
    ok = np.zeros(14, F32)
    assert call(0, 0, ok) == 0
    assert call(2, 0, ok) == 1 and call(0, 6, ok) == 1 and call(0, -1, ok) == 1
    for bad in (len(mats), -1.0, 0.5, np.nan):
        vin = ok.copy(); vin[0] = bad
        assert call(0, 0, vin) == 1 and call(1, 4, vin) == 1
    vin = ok.copy(); vin[0] = len(bc.TEXTURE_NAMES)
    assert call(0, 1, vin) == 1 and call(0, 1, ok) == 0
    wrong = mats.copy(); wrong[0, 22] = len(bc.TEXTURE_NAMES)             # a material that names a texture the scene does not have
    assert call(0, 0, ok, mats=wrong) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# 2. frames: constructed scenes that send paths through the edges on purpose
# ---------------------------------------------------------------------------------------------------------------------------
W, H, SPP, BOUNCES = 48, 32, 3, 5
SCENES = ("grazing_anisotropic_floor", "back_faces_under_three_lights", "nested_glass", "nested_glass_instanced", "edge_textures",
          "rough_then_mirror")


def _three_lights(scenes):
    return np.stack([scenes.pack_rect_light((0.0, 3.0, 0.0), (1, 0, 0), (0, 0, 1), (1.5, 1.5), (9, 8, 7), rng=40.0),
                     scenes.pack_point_light((-1.5, 1.2, -1.0), (5, 5, 6), rng=12.0),
                     scenes.pack_spot_light((1.5, 2.0, -1.5), (-0.4, -1.0, 0.5), 80.0, 50.0, (8, 7, 6), rng=15.0)])


def _scene(name):
    from unity_webgpu_pathtracer_amd import scenes
    from unity_webgpu_pathtracer_amd.scenes import Camera, Scene, SoupBuilder, pack_material
    M = lambda n: np.array(bc.materials()[bc.MI[n]])
    no_tex = np.zeros(0, dtype=U32)
    sky = dict(environment_mode=0, environment_color=(0.5, 0.6, 0.8, 1.0), environment_intensity=0.9)
    sb = SoupBuilder()
    if name == "grazing_anisotropic_floor":      # the camera 1e-3 above a rough anisotropic metal floor, looking along it
        sb.quad((-6, 0, -6), (12, 0, 0), (0, 0, 12), (0, 1, 0), 2, 2, 0)
        sb.uv_sphere((0.0, 0.6, 3.0), 0.6, 10, 6, 1)
        verts, attrs = sb.finish()
        mats = np.stack([M("aniso1"), M("pointwise3"), ])
        return Scene(name, verts, attrs, mats, _three_lights(scenes)[:1], no_tex, Camera(eye=(0, 1e-3, -5.0), target=(0, 1e-3, 5.0), vfov_deg=50.0), **sky)
    if name == "back_faces_under_three_lights":  # single-sided quads seen from behind: normal != ffnormal at every first hit
        mats = np.stack([M("pointwise4"), M("pointwise9"), M("coat_gloss1"), M("pointwise7")])
        sb.quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, -1, 0), 2, 2, 0)           # a floor whose normal points down
        for k, x in enumerate((-1.6, 0.0, 1.6)):
            sb.quad((x - 0.6, 0.2, 1.0 + 0.3 * k), (1.2, 0, 0.2 * k), (0, 1.4, 0.3), (0, 0.2, 1), 2, 2, 1 + k)      # facing away from the camera
        verts, attrs = sb.finish()
        return Scene(name, verts, attrs, mats, _three_lights(scenes), no_tex, Camera(eye=(0, 1.5, -4.0), target=(0, 0.6, 1.0), vfov_deg=50.0), **sky)
    if name in ("nested_glass", "nested_glass_instanced"):      # ior at both clamps: eta flips at every shell, total internal reflection inside
        mats = np.stack([M("pointwise0"), M("opacity0"), M("pointwise8"), M("opacity-0.5")])
        mats[1, 11], mats[2, 11], mats[3, 11] = 2.5, 0.5, 2.0
        cam = Camera(eye=(0, 1.2, -3.5), target=(0, 1.0, 0.0), vfov_deg=40.0)
        if name == "nested_glass":
            sb.quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0), 2, 2, 0)
            for k, r in enumerate((1.0, 0.7, 0.4)):
                sb.uv_sphere((0.0, 1.0, 0.0), r, 12, 8, 1 + k)
            verts, attrs = sb.finish()
            return Scene(name, verts, attrs, mats, _three_lights(scenes)[:2], no_tex, cam, **sky)
        sb.uv_sphere((0, 0, 0), 0.5, 12, 8, 0)
        sphere = sb.finish()
        sb = SoupBuilder()
        sb.quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0), 2, 2, 0)
        floor = sb.finish()
        verts, attrs = np.concatenate([sphere[0], floor[0]]), np.concatenate([sphere[1], floor[1]])
        n0 = sphere[0].shape[0] // 3
        inst = [(1, scenes._trs(), 0)] + [(0, scenes._trs((0.0, 1.0, 0.0), 20.0 * k, 10.0 * k, (2 * r, 2 * r * (1.0 + 0.1 * k), 2 * r)), 1 + k)
                                          for k, r in enumerate((1.0, 0.7, 0.4))]
        return Scene(name, verts, attrs, mats, _three_lights(scenes)[:2], no_tex, cam, mesh_ranges=[(0, n0), (n0, floor[0].shape[0] // 3)], instances=inst, **sky)
    if name == "edge_textures":                  # the 1 x 1, 1 x 7 and 7 x 1 textures in every slot, under the extreme uv transforms
        t = bc.TEX
        base = dict(color=(0.9, 0.8, 0.7, 1), roughness=0.5, metallic=0.3, ior=1.4)
        mats = np.stack([
            pack_material(tex_base=t["w1h1"], tex_mr=t["w1h7"], tex_emission=t["w7h1"], tex_occlusion=t["w1h1"], **base),
            pack_material(tex_base=t["w1h7"], tex_mr=t["w7h1"], tex_emission=t["w1h1"], tex_occlusion=t["w7h1"], uv_scale=(0.0, 0.0), uv_offset=(1.0, 1.0), **base),
            pack_material(tex_base=t["w7h1"], tex_mr=t["w1h1"], tex_emission=t["w1h7"], tex_occlusion=t["w1h7"], uv_scale=(1.0, 1.0), uv_offset=(-1.5, 2.25), **base),
            pack_material(tex_base=t["w1h7"], tex_mr=t["w1h7"], tex_emission=t["w7h1"], tex_occlusion=t["w7h1"], uv_scale=(4.0 * bc.TWO24, 1.0), uv_offset=(0.0, 2.0 * bc.TWO24), **base),
            M("tex_all_four")])
        sb.quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0), 3, 3, 0, uv_scale=(2.0, 2.0))
        for k in range(4):
            sb.uv_sphere((-2.1 + 1.4 * k, 0.6, 0.5 * (k % 2)), 0.55, 10, 6, 1 + k, uv_scale=(1.0, 1.0) if k % 2 else (3.0, -2.0))
        verts, attrs = sb.finish()
        return Scene(name, verts, attrs, mats, _three_lights(scenes), np.array(bc.texture_data()), Camera(eye=(0, 2.0, -4.5), target=(0, 0.5, 0.0), vfov_deg=45.0), **sky)
    if name == "rough_then_mirror":              # a roughness-1 first hit, then a roughness-0 mirror: the running maximum overrides the clamped 0.001
        mats = np.stack([M("rough1"), M("rough0"), pack_material(color=(0.9, 0.9, 0.9, 1), roughness=0.0, metallic=1.0)])
        sb.quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0), 2, 2, 0)
        sb.quad((-4, 0, 2.0), (8, 0, 0), (0, 4, 0), (0, 0, -1), 2, 2, 2)
        sb.uv_sphere((0.0, 0.7, 0.0), 0.7, 12, 8, 1)
        verts, attrs = sb.finish()
        return Scene(name, verts, attrs, mats, _three_lights(scenes)[:1], no_tex, Camera(eye=(0, 2.5, -4.0), target=(0, 0.2, 0.5), vfov_deg=50.0), **sky)
    raise ValueError(name)


def _params(s, seed=0xB5DF):
    from unity_webgpu_pathtracer_amd import scenes
    return scenes.frame_params(s, W, H, spp=SPP, seed=seed, max_bounces=BOUNCES, russian_roulette=False)


_oracle_frames = {}


def _oracle_frame(oracle, name):
    """the oracle's frame and counters of a scene: computed once, shared by the tests that need it (the CPU-built BVH is the same)"""
    from unity_webgpu_pathtracer_amd.pathtracer import BVHScene
    if name not in _oracle_frames:
        s = _scene(name)
        ref, st = oracle.render(oracle.buffers_from_bvhscene(BVHScene(s)), _params(s), shadow_any_hit=True)
        ref.setflags(write=False)
        _oracle_frames[name] = (ref, st)
    return _oracle_frames[name]


@pytest.mark.parametrize("name", SCENES)
def test_constructed_scenes_bit_exact(oracle, name):
    """48 x 32 at 3 spp, 5 bounces, schedules 0, 1 and 4 on one context: every frame and all 16 counters equal the oracle's (on the
    instanced scene, HAS_TLAS, schedule 4 runs schedule 1's two-level kernels)."""
    from test_gpu_env import _assert_frame, _render
    from test_gpu_parity import ALL_COUNTERS, _stats_equal
    from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
    s = _scene(name)
    ref, st = _oracle_frame(oracle, name)
    assert st.materialFetches > W * H and not np.isnan(ref[..., :3]).all()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=SPP, maxRayBounces=BOUNCES)
    try:
        pt.set_stats_level(1)
        for schedule in (0, 1, 4):
            pt.set_schedule(schedule)
            pt.reset_stats()
            _assert_frame(f"{name}, schedule {schedule}", _render(pt, _params(s)), ref)
            _stats_equal(pt.stats(), st, ALL_COUNTERS)
    finally:
        pt.close()


STRESS_SCENE = "nested_glass"

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
from test_gpu_env import _render
from test_gpu_bsdf import STRESS_SCENE, W, H, SPP, BOUNCES, _scene, _params
s = _scene(STRESS_SCENE)
pt = PathTracer(s, width=W, height=H, samplesPerPass=SPP, maxRayBounces=BOUNCES, schedule=1)
pt.set_stats_level(1)
frame = _render(pt, _params(s))
st = pt.stats().as_dict()
pt.close()
np.savez(sys.argv[2], frame=frame, stats=np.array([st[k] for k in sorted(st)], dtype=np.uint64))
'''


@pytest.mark.parametrize("build", sorted(STRESS))
def test_stress_builds_render_the_nested_glass(oracle, build, tmp_path):
    """The nested glass spheres on both stress builds (traversal stacks of one LDS entry; a slot repack after every iteration), the
    default schedule, in one fresh child process: the frame and all counters equal the oracle's."""
    from test_gpu_env import _assert_frame
    from test_gpu_parity import ALL_COUNTERS
    if not os.path.exists(STRESS[build]):
        subprocess.check_call(["make", "-C", CSRC, build], stdout=subprocess.DEVNULL)
    out = str(tmp_path / "frame.npz")
    subprocess.check_call([sys.executable, "-c", CHILD, ROOT, out], env=dict(os.environ, PT_PLUGIN=STRESS[build]), timeout=300)
    got = np.load(out)
    ref, st = _oracle_frame(oracle, STRESS_SCENE)
    _assert_frame(f"{build}, {STRESS_SCENE}", got["frame"], ref)
    want = st.as_dict()
    stats = dict(zip(sorted(want), (int(v) for v in got["stats"])))
    bad = {k: (stats[k], want[k]) for k in ALL_COUNTERS if stats[k] != want[k]}
    assert not bad, f"{build}: counter mismatch (gpu, oracle): {bad}"
