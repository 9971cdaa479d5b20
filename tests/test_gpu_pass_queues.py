"""Every pass in flight runs on its state set's own stream, and with fewer than 16 hardware queues the set streams are created
at stream priority levels of their own (create_set_stream, csrc/pt_api_context.hip).  None of that may show in a result:
whatever the queue limit and however many sets take turns, a sequence of accumulating passes gives the bytes and the 16
counters it gives with the passes back to back, and the default number of passes in flight is the documented one.

What these tests do not see is which hardware queue a stream landed on: that is a kernel trace's to show
(profiles/own_queues_ab.md).  The default of 12 at a limit of 4 is reached only when set 0's stream could be created at a
private level, so that much of the mechanism is covered.

The Cornell box is rendered with schedule 1: its automatic schedule is the megakernel, which uses no state sets."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0, SEED_STEP = 0x0C0FFEE1, 0x9E3779B9
SIZES = ((64, 48), (40, 24))        # 40x24: a partial 16x16 block per row of blocks, and fewer slots than one 128-slot trace range


def _sequence(pt, passes, between=None):
    """`passes` accumulating passes from a fresh frame; between(k), if given, runs before pass k.  -> (frame, counters)"""
    pt.synchronize()
    pt.Reset()
    pt.reset_stats()
    for k in range(passes):
        if between:
            between(k)
        pt.OnRenderImage((SEED0 + k * SEED_STEP) & 0xFFFFFFFF)
    frame = pt.readback()
    st = pt.stats().as_dict()
    assert len(st) == 16
    return frame, np.array([st[k] for k in sorted(st)], dtype=np.uint64)


def _tracer(w, h):
    from unity_webgpu_pathtracer_amd import scenes
    from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
    pt = PathTracer(scenes.cornell_box(), width=w, height=h, samplesPerPass=2, maxRayBounces=3, schedule=1)
    pt.set_stats_level(1)
    return pt


# run as `python -c CHILD <root> <out.npz>` under the environment a case asks for
CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_pass_queues as t
out = {}
for w, h in t.SIZES:
    pt = t._tracer(w, h)
    sets = pt.passes_in_flight()
    out[f"default_{w}"] = np.array([sets])
    out[f"frame_{w}"], out[f"stats_{w}"] = t._sequence(pt, 2 * sets + 2)          # more passes than sets: the rotation wraps
    pt.set_passes_in_flight(1)
    out[f"frame1_{w}"], out[f"stats1_{w}"] = t._sequence(pt, 2 * sets + 2)
    pt.set_passes_in_flight(0)
    out[f"default_again_{w}"] = np.array([pt.passes_in_flight()])
    pt.close()
np.savez(sys.argv[2], **out)
'''


@pytest.mark.gpu
@pytest.mark.parametrize("queues", ["4", "16", None])
def test_queue_settings(tmp_path, queues):
    """GPU_MAX_HW_QUEUES = 4 (the runtime's own default), 16, and not set at all: two private priority levels of that many queues
    hold 8 or more set streams, which is what the documented default of 12 passes in flight asks for (include/ptmi_plugin.h)."""
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = queues
    out = str(tmp_path / "queues.npz")
    subprocess.check_call([sys.executable, "-c", CHILD, ROOT, out], env=env, timeout=300)
    got = np.load(out)
    for w, _ in SIZES:
        print(f"[pass queues] GPU_MAX_HW_QUEUES={queues}, width {w}: default passes in flight {int(got[f'default_{w}'][0])}, "
              f"counters {json.dumps(got[f'stats_{w}'].tolist())}")
        assert int(got[f"default_{w}"][0]) == 12 and int(got[f"default_again_{w}"][0]) == 12
        assert got[f"frame_{w}"].any()
        assert np.array_equal(got[f"frame_{w}"].view(np.uint32), got[f"frame1_{w}"].view(np.uint32))
        assert np.array_equal(got[f"stats_{w}"], got[f"stats1_{w}"])


@pytest.mark.gpu
def test_set_count_and_sub_frames():
    """PTSetPassesInFlight(1, 2, 5, 12, 0) and PTSetSubFrames(3) between the passes of one context: k + 1 passes at every k, so
    that each count's rotation wraps; the frames are those of the same passes back to back."""
    w, h = SIZES[0]
    pt = _tracer(w, h)
    plan = []                                   # per pass: what to set before it
    for k in (1, 2, 5, 12, 0):
        plan += [("sets", k)] + [None] * (k if k else pt.passes_in_flight())
    plan += [("sub", 3), None, None, ("sub", 1), None]

    def between(i):
        if plan[i]:
            (pt.set_passes_in_flight if plan[i][0] == "sets" else pt.set_sub_frames)(plan[i][1])

    frame, stats = _sequence(pt, len(plan), between)
    assert pt.passes_in_flight() in (3, 6, 12)              # the default again, whatever this process's queue limit is
    pt.set_passes_in_flight(1)
    frame1, stats1 = _sequence(pt, len(plan))
    pt.close()
    assert frame.any()
    assert np.array_equal(frame.view(np.uint32), frame1.view(np.uint32))
    assert np.array_equal(stats, stats1)


@pytest.mark.gpu
def test_context_lifetime():
    """Three contexts, one after the other in one process, each rendering with all of its sets: a destroyed context gives its
    streams back, so the third behaves like the first."""
    w, h = SIZES[0]
    results = []
    for _ in range(3):
        pt = _tracer(w, h)
        sets = pt.passes_in_flight()
        results.append((sets,) + _sequence(pt, sets + 2))
        pt.close()
    for sets, frame, stats in results[1:]:
        assert sets == results[0][0]
        assert np.array_equal(frame.view(np.uint32), results[0][1].view(np.uint32))
        assert np.array_equal(stats, results[0][2])
