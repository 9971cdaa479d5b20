"""The packed path state of a repacked sequence on the GPU (csrc/pt_wf_state.h, shade_slot's PACKED, csrc/pt_repack.hip).

In a repacked sequence the RNG state lives in rad.w and the pending throughput in envC.w, lightC.w and thr.w; B.rng and B.pthr are
not touched, color is stored only by a step that changed it, and a slot that ends a step DONE stores its flags and its pixel's sum
only.  None of that may change a result: the variant library of tests/test_gpu_repack.py (make stress-repack: sets of 256 slots,
a candidate after every iteration, no fill threshold) renders every case in ONE child process, every frame is compared bitwise
with the oracle's, and at stats level 1 all 16 counters with the oracle's.  The cases are chosen for the words that moved."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRESS = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib", "libpt-stress-repack.so")
SEEDS = [0x9ACCED01, 0x9ACCED02, 0x9ACCED03]
QUERY_RAYS = 1024

# name -> (scene, its arguments, width, height, spp, bounces, frame_params keywords)
CASES = {
    # RNG continuity through rad.w across many moves; pending NEE carried across a repack in envC.w, lightC.w and thr.w
    "zoo": ("material_zoo", {}, 64, 32, 3, 4, {}),
    # the fold paths that decide the color store: the clamp of the firefly filter (a luminance the zoo's lights exceed), no
    # roulette so that paths end at the bounce limit; then the roulette's kills
    "firefly": ("material_zoo", {}, 64, 32, 3, 4, {"firefly": True, "max_firefly_luminance": 1.0, "russian_roulette": False}),
    "roulette": ("material_zoo", {}, 64, 32, 3, 4, {"firefly": False, "russian_roulette": True, "seed": SEEDS[1]}),        # other paths than "zoo"
    # every sample is its pixel's last: DONE-only stores right after a pending-only step
    "last": ("material_zoo", {}, 64, 32, 1, 1, {}),
    # HAS_TLAS shade and cleanup
    "tlas": ("instanced_scene", {"count": 20}, 64, 48, 2, 4, {}),
}
# the two cases that share one context across layouts and schedules
MIX = ("material_zoo", {}, 64, 32, 2, 4)

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from unity_webgpu_pathtracer_amd import scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
from test_gpu_packed_state import CASES, MIX, SEEDS, QUERY_RAYS, case_params
out = {}

def to_frame(pt, p, w, h):
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    pt.render_pass_to(p, frame.data_ptr(), 0)
    pt.synchronize()
    return frame.cpu().numpy()

def repacks(pt):
    rp = pt.repack_stats().as_dict()
    return np.array([rp[k] for k in ("sequences", "candidates", "repacks", "slotsMoved")], dtype=np.uint64)

for name, (scene, kw, w, h, spp, bounces, fp) in CASES.items():
    s = getattr(scenes, scene)(**kw)
    for level in (0, 1):
        pt = PathTracer(s, width=w, height=h, samplesPerPass=spp, maxRayBounces=bounces, schedule=1)
        pt.set_stats_level(level)
        out[f"{name}_frame{level}"] = to_frame(pt, case_params(s, w, h, spp, bounces, fp), w, h)
        st = pt.stats().as_dict()
        out[f"{name}_stats{level}"] = np.array([st[k] for k in sorted(st)], dtype=np.uint64)
        out[f"{name}_repack{level}"] = repacks(pt)
        print(f"[packed] {name} level {level}: {pt.repack_stats().as_dict()}", flush=True)
        pt.close()

scene, kw, w, h, spp, bounces = MIX
s = getattr(scenes, scene)(**kw)
# two layouts on one state set: a repacked pass, a radiance query (ray map: reads and returns B.rng), a pass over a block list
# (B.rng, B.pthr), a second repacked pass
pt = PathTracer(s, width=w, height=h, samplesPerPass=spp, maxRayBounces=bounces, schedule=1)
p0 = pt.params(SEEDS[0])
pt.OnRenderImage(SEEDS[0])
out["mix_pass1"] = pt.readback()
out["mix_repack1"] = repacks(pt)
rays = pt.camera_rays(params=p0)[:QUERY_RAYS]
out["mix_query"] = pt.radiance(rays, spp=2, params=p0)
pt.adaptive_begin()
assert pt.set_active_blocks(None) == (w // 16) * (h // 16)
pt.render_active([SEEDS[1]])
out["mix_active"] = pt.readback(last_output=False)
out["mix_pass2"] = to_frame(pt, case_params(s, w, h, spp, bounces, {}, SEEDS[2]), w, h)
out["mix_repack2"] = repacks(pt)
pt.close()
fresh = PathTracer(s, width=w, height=h, samplesPerPass=spp, maxRayBounces=bounces, schedule=1)
out["mix_query_fresh"] = fresh.radiance(rays, spp=2, params=p0)
fresh.close()

# schedule 1 -> 4 -> 1 on one context
pt = PathTracer(s, width=w, height=h, samplesPerPass=spp, maxRayBounces=bounces, schedule=1)
p = case_params(s, w, h, spp, bounces, {}, SEEDS[1])
for k, schedule in enumerate((1, 4, 1)):
    pt.set_schedule(schedule)
    out[f"sched_frame{k}"] = to_frame(pt, p, w, h)
    out[f"sched_repack{k}"] = repacks(pt)
pt.close()
np.savez(sys.argv[2], **out)
'''


def case_params(s, w, h, spp, bounces, fp, seed=SEEDS[0], current_sample=0):
    from unity_webgpu_pathtracer_amd import scenes
    fp = dict(fp)
    return scenes.frame_params(s, w, h, spp=spp, current_sample=current_sample, seed=fp.pop("seed", seed), max_bounces=bounces, **fp)


@pytest.fixture(scope="module")
def packed_run(tmp_path_factory):
    """every case rendered by the variant library, in ONE fresh child process"""
    if not os.path.exists(STRESS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc"), "stress-repack"], stdout=subprocess.DEVNULL)
    out = str(tmp_path_factory.mktemp("packed") / "packed.npz")
    subprocess.check_call([sys.executable, "-c", CHILD, ROOT, out], env=dict(os.environ, PT_PLUGIN=STRESS), timeout=600)
    return np.load(out)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle_buffers(oracle, scene, kw):
    from unity_webgpu_pathtracer_amd import scenes
    from unity_webgpu_pathtracer_amd.pathtracer import BVHScene
    s = getattr(scenes, scene)(**kw)
    return s, oracle.buffers_from_bvhscene(BVHScene(s))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_frames_and_counters_equal_the_oracle(packed_run, oracle, name):
    scene, kw, w, h, spp, bounces, fp = CASES[name]
    s, b = _oracle_buffers(oracle, scene, kw)
    ref, st = oracle.render(b, case_params(s, w, h, spp, bounces, fp), shadow_any_hit=True)
    total = st.as_dict()
    for level in (0, 1):
        got = packed_run[f"{name}_frame{level}"]
        bad = int((_bits(got) != _bits(ref)).any(axis=-1).sum())
        sequences, candidates, repacks, moved = (int(x) for x in packed_run[f"{name}_repack{level}"])
        print(f"[packed] {name} level {level}: {bad} pixels differ; candidates {candidates} repacks {repacks} slots moved {moved}")
        assert bad == 0, (name, level, bad)
        assert sequences == 1 and repacks >= 1 and moved >= repacks, (name, candidates, repacks, moved)      # the words really moved
    assert np.array_equal(packed_run[f"{name}_stats1"], np.array([total[k] for k in sorted(total)], dtype=np.uint64)), name
    for k in ("paths", "closestHitRays", "shadowRays"):                                                     # level 0 counts paths and rays only
        assert int(packed_run[f"{name}_stats0"][sorted(total).index(k)]) == total[k], (name, k)


@pytest.mark.gpu
def test_two_layouts_share_one_state_set(packed_run, oracle):
    """A repacked pass leaves RNG states in rad.w and nothing in B.rng; the query and the block-list pass that follow on the same
    context use B.rng and B.pthr, and the repacked pass after them starts from pt_wf_init again."""
    scene, kw, w, h, spp, bounces = MIX
    s, b = _oracle_buffers(oracle, scene, kw)
    ref1, _ = oracle.render(b, case_params(s, w, h, spp, bounces, {}, SEEDS[0]), shadow_any_hit=True)
    assert (_bits(packed_run["mix_pass1"]) == _bits(ref1)).all()
    ref_active, _ = oracle.render(b, case_params(s, w, h, spp, bounces, {}, SEEDS[1], current_sample=spp), accumulated=ref1, shadow_any_hit=True)
    assert (_bits(packed_run["mix_active"]) == _bits(ref_active)).all()
    ref2, _ = oracle.render(b, case_params(s, w, h, spp, bounces, {}, SEEDS[2]), shadow_any_hit=True)
    assert (_bits(packed_run["mix_pass2"]) == _bits(ref2)).all()
    assert packed_run["mix_query"].shape == (QUERY_RAYS, 4)
    assert (_bits(packed_run["mix_query"]) == _bits(packed_run["mix_query_fresh"])).all()
    first, second = packed_run["mix_repack1"], packed_run["mix_repack2"]
    assert int(first[2]) >= 1 and int(second[0]) == 2 and int(second[2]) > int(first[2]), (first, second)     # both frame passes repacked, nothing else did


@pytest.mark.gpu
def test_schedules_alternate_on_one_context(packed_run, oracle):
    scene, kw, w, h, spp, bounces = MIX
    s, b = _oracle_buffers(oracle, scene, kw)
    ref, _ = oracle.render(b, case_params(s, w, h, spp, bounces, {}, SEEDS[1]), shadow_any_hit=True)
    for k in range(3):
        assert (_bits(packed_run[f"sched_frame{k}"]) == _bits(ref)).all(), k
    seq = [int(packed_run[f"sched_repack{k}"][0]) for k in range(3)]
    assert seq == [1, 1, 2], seq                                       # schedule 4 has no slots to repack
