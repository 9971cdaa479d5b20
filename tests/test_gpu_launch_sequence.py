"""The launch sequence of every schedule, counted: PTTimings.kernelLaunches of one call is what the launcher's structure implies.

A 32x32 frame, 1 sample per pass and MaxRayBounces = 2 give spp * (bounces + 2) + 4 = 8 iterations.  A wavefront sequence is the
init kernel, per iteration the trace launches and the shade kernel, then cleanup, resolve and the counter fold:
  schedule 1, flat scene      1 + 8 * 3 + 3 = 28   (refill trace + its tail launch + shade)
  schedule 1, HAS_TLAS        1 + 8 * 2 + 3 = 20   (the two-level refill kernel has no tail launch)
  schedules 2 and 3           1 + 8 * 2 + 3 = 20   (one trace launch per iteration)
  schedule 4, flat scene      3                    (fused persistent kernel, resolve, fold)
  schedule 4, HAS_TLAS        20                   (runs schedule 1's HAS_TLAS sequence)
  schedule 0                  1                    (the megakernel)
A pass over a block list and a radiance query, an irradiance gather or an SH probe call of one chunk run the same sequence
(a gather and a probe call run one sample per slot: 16 entries x 4 samples = 64 slots, rounded up to 256, the same 8 iterations);
schedules 0 and 4 have none of them.  A list call cut into k chunks runs k sequences: a chunk holds 2^21 slots."""
import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer

pytestmark = pytest.mark.gpu

W = H = 32
ITERATIONS = 8
SCENES = {"flat": scenes.material_zoo, "tlas": scenes.instanced_scene}


def _wavefront(launches_per_iteration):
    return 1 + ITERATIONS * launches_per_iteration + 3


EXPECTED = {(1, "flat"): _wavefront(3), (1, "tlas"): _wavefront(2),
            (2, "flat"): _wavefront(2), (2, "tlas"): _wavefront(2),
            (3, "flat"): _wavefront(2), (3, "tlas"): _wavefront(2),
            (4, "flat"): 3, (4, "tlas"): _wavefront(2),
            (0, "flat"): 1, (0, "tlas"): 1}


def _tracer(kind, schedule, width=W, height=H):
    pt = PathTracer(SCENES[kind](), width=width, height=height, samplesPerPass=1, maxRayBounces=2, schedule=schedule)
    pt.set_profiling(True)
    return pt


def _launches(pt, call):
    """kernelLaunches of what `call` enqueues: timings reset before, read after a drain"""
    pt.reset_timings()
    call()
    pt.synchronize()
    return pt.timings().kernelLaunches


def _points(rays, n):
    """n fixed points in front of the camera, one unit along the first n camera rays, facing back at it"""
    return rays[:n, 0:3] + rays[:n, 3:6], -rays[:n, 3:6]


@pytest.mark.parametrize("kind", ["flat", "tlas"])
@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4])
def test_launches_per_call(schedule, kind):
    want = EXPECTED[(schedule, kind)]
    pt = _tracer(kind, schedule)
    try:
        p = pt.params(seed=0x1A2B)
        got = {"render_pass": _launches(pt, lambda: pt.render_pass(p))}
        if schedule in (1, 2, 3):
            pt.adaptive_begin(current_sample=0)
            assert pt.set_active_blocks(None) == 4               # all four 16x16 blocks
            got["render_active"] = _launches(pt, lambda: pt.render_active([0x1A2B]))
            pt.adaptive_end()
            rays = pt.camera_rays(params=p)
            assert rays.shape == (W * H, 8)                      # 1,024 rays: one chunk
            got["radiance"] = _launches(pt, lambda: pt.radiance(rays, spp=1, params=p))
            pos, nrm = _points(rays, 16)
            got["irradiance"] = _launches(pt, lambda: pt.irradiance(pos, nrm, spp=4, params=p))
            got["probe_sh"] = _launches(pt, lambda: pt.probe_sh(pos, spp=4, delta_lights=False, params=p))
        print(f"[launch sequence] schedule {schedule} {kind}: {got}, expected {want} each")
        assert all(n == want for n in got.values()), (got, want)
    finally:
        pt.close()


def test_two_sub_frames_are_two_sequences():
    """64x32: both sub-frames own 16x16 blocks, each runs the whole sequence of schedule 1 on a flat scene"""
    pt = _tracer("flat", 1, width=64, height=32)
    try:
        assert pt.passes_in_flight() >= 2
        pt.set_sub_frames(2)
        p = pt.params(seed=0x1A2B)
        got = _launches(pt, lambda: pt.render_pass(p))
        print(f"[launch sequence] two sub-frames: {got}, expected {2 * EXPECTED[(1, 'flat')]}")
        assert got == 2 * EXPECTED[(1, "flat")]
    finally:
        pt.close()


def test_chunks_are_sequences():
    """The smallest lists that reach a second chunk of 2^21 slots, schedule 1 on a flat scene: two sequences each"""
    want = 2 * EXPECTED[(1, "flat")]
    pt = _tracer("flat", 1)
    try:
        p = pt.params(seed=0x1A2B)
        rays = pt.camera_rays(params=p)
        many = np.tile(rays, ((1 << 21) // len(rays) + 1, 1))[:(1 << 21) + 1]                 # chunks of 2^21 and 1
        pos, nrm = _points(rays, 33)                                                        # 65,536 samples each: chunks of 32 and 1
        got = {"radiance": _launches(pt, lambda: pt.radiance(many, spp=1, params=p)),
               "irradiance": _launches(pt, lambda: pt.irradiance(pos, nrm, spp=65536, params=p)),
               "probe_sh": _launches(pt, lambda: pt.probe_sh(pos, spp=65536, delta_lights=False, params=p))}
        print(f"[launch sequence] two chunks: {got}, expected {want} each")
        assert all(n == want for n in got.values()), (got, want)
    finally:
        pt.close()
