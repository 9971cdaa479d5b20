"""The launch sequence of every schedule, counted: PTTimings.kernelLaunches of one call is what the launcher's structure implies.

A 32x32 frame, 1 sample per pass and MaxRayBounces = 2 give spp * (bounces + 2) + 4 = 8 iterations.  A wavefront sequence is the
init kernel, per iteration the trace launches and the shade kernel, then cleanup, resolve and the counter fold:
  schedule 1, flat scene      1 + 8 * 3 + 3 = 28   (refill trace + its tail launch + shade)
  schedule 1, HAS_TLAS        1 + 8 * 2 + 3 = 20   (the two-level refill kernel has no tail launch)
  schedules 2 and 3           1 + 8 * 2 + 3 = 20   (one trace launch per iteration)
  schedule 4, flat scene      3                    (fused persistent kernel, resolve, fold)
  schedule 4, HAS_TLAS        20                   (runs schedule 1's HAS_TLAS sequence)
  schedule 0                  1                    (the megakernel)
A pass over a block list and a radiance query of one chunk run the same sequence; schedules 0 and 4 have neither."""
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
