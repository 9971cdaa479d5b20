"""The streams of the state sets below a limit of 16 hardware queues (create_set_stream, csrc/pt_api_context.hip).

The current mechanism, which supersedes the one the docstring of tests/test_gpu_pass_queues.py describes (private stream priority
levels): with GPU_MAX_HW_QUEUES below 16 every set stream is made with hipExtStreamCreateWithCUMask and every CU enabled.  The
runtime cannot pool a queue that carries a CU mask, so each of the twelve sets has a hardware queue of its own at normal
priority (DESIGN.md 5.1 "Queues of the sets' own", profiles/normal_queues_ab.md).  That call takes no flags, so these streams
synchronise with the null stream, which the earlier hipStreamNonBlocking ones did not.  What these tests hold on to:

* a host that works on the null stream between passes (and synchronises the device now and then) orders more, never less: the
  frame and the 16 counters are those of the passes back to back;
* a destroyed context gives its streams and their queues back: eight contexts in a row behave like the first;
* set counts and sub-frames wrap their rotations under a limit of 4 as they do under the test process's own.

No test looks at queue ids: a kernel trace shows those (profiles/normal_queues_ab.md).  Shapes and passes are those of
tests/test_gpu_pass_queues.py: Cornell box, schedule 1 (its automatic schedule, the megakernel, uses no state sets), 2 spp, depth 3."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0, SEED_STEP = 0x0C0FFEE1, 0x9E3779B9
SIZES = ((64, 48), (40, 24))        # 40x24: a partial 16x16 block per row of blocks, and fewer slots than one 128-slot trace range
SETS = 12                           # the documented default of passes in flight (include/ptmi_plugin.h)


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


def _null_stream_traffic(out):
    """per size: the reference (one pass in flight, nothing in between) once, then all sets with a small operation on torch's
    default stream -- the null stream -- before every pass, without and with a device synchronisation every fifth pass"""
    import torch
    x = torch.zeros(256, dtype=torch.float32, device="cuda")
    assert torch.cuda.current_stream().cuda_stream == 0           # the null stream: what a blocking stream synchronises with

    def touch(k):
        x.add_(1.0)

    def touch_and_sync(k):
        x.add_(1.0)
        if k % 5 == 4:
            torch.cuda.synchronize()

    for w, h in SIZES:
        pt = _tracer(w, h)
        sets = pt.passes_in_flight()
        out[f"default_{w}"] = np.array([sets])
        passes = 2 * SETS + 2                                     # more passes than sets: the rotation wraps
        pt.set_passes_in_flight(1)
        out[f"frame1_{w}"], out[f"stats1_{w}"] = _sequence(pt, passes)
        pt.set_passes_in_flight(0)
        out[f"frame_touch_{w}"], out[f"stats_touch_{w}"] = _sequence(pt, passes, touch)
        out[f"frame_sync_{w}"], out[f"stats_sync_{w}"] = _sequence(pt, passes, touch_and_sync)
        pt.close()
    torch.cuda.synchronize()
    out["touched"] = x[:1].cpu().numpy()


def _set_count_and_sub_frames(out):
    w, h = SIZES[0]
    pt = _tracer(w, h)
    out["default"] = np.array([pt.passes_in_flight()])
    plan = []                                   # per pass: what to set before it
    for k in (1, 5, 12, 0):
        plan += [("sets", k)] + [None] * (k if k else pt.passes_in_flight())
    plan += [("sub", 3), None, None, ("sub", 1), None]

    def between(i):
        if plan[i]:
            (pt.set_passes_in_flight if plan[i][0] == "sets" else pt.set_sub_frames)(plan[i][1])

    out["frame"], out["stats"] = _sequence(pt, len(plan), between)
    out["default_again"] = np.array([pt.passes_in_flight()])
    pt.set_passes_in_flight(1)
    out["frame1"], out["stats1"] = _sequence(pt, len(plan))
    pt.close()


# run as `python -c CHILD <root> <out.npz> <case>` under the environment a case asks for
CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_set_streams as t
out = {}
getattr(t, "_" + sys.argv[3])(out)
np.savez(sys.argv[2], **out)
'''


def _child(tmp_path, case, queues):
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = queues
    out = str(tmp_path / f"{case}.npz")
    subprocess.check_call([sys.executable, "-c", CHILD, ROOT, out, case], env=env, timeout=300)
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("queues", ["4", None])
def test_null_stream_traffic_between_passes(tmp_path, queues):
    """2 * 12 + 2 accumulating passes with a small torch operation on the null stream before every pass, and the same with a
    torch.cuda.synchronize() every fifth pass: bit-equal to the passes with one pass in flight, the 16 counters equal."""
    got = _child(tmp_path, "null_stream_traffic", queues)
    assert float(got["touched"][0]) == 2.0 * len(SIZES) * (2 * SETS + 2)         # every operation on the null stream ran
    for w, _ in SIZES:
        print(f"[set streams] GPU_MAX_HW_QUEUES={queues}, width {w}: default passes in flight {int(got[f'default_{w}'][0])}, "
              f"counters {json.dumps(got[f'stats1_{w}'].tolist())}")
        assert int(got[f"default_{w}"][0]) == SETS
        assert got[f"frame1_{w}"].any()
        for variant in ("touch", "sync"):
            assert np.array_equal(got[f"frame_{variant}_{w}"].view(np.uint32), got[f"frame1_{w}"].view(np.uint32)), variant
            assert np.array_equal(got[f"stats_{variant}_{w}"], got[f"stats1_{w}"]), variant


@pytest.mark.gpu
def test_eight_contexts_in_a_row():
    """Eight contexts, one after the other in one process, each rendering 12 + 2 passes with all of its sets (every wrapper call
    raises on an error code): each reports 12 passes in flight and gives the first one's bytes and counters -- a destroyed
    context has given its twelve set streams, and whatever queues they held, back."""
    w, h = SIZES[0]
    results = []
    for _ in range(8):
        pt = _tracer(w, h)
        sets = pt.passes_in_flight()
        results.append((sets,) + _sequence(pt, SETS + 2))
        pt.close()
    assert results[0][1].any()
    for sets, frame, stats in results:
        assert sets == SETS
        assert np.array_equal(frame.view(np.uint32), results[0][1].view(np.uint32))
        assert np.array_equal(stats, results[0][2])


@pytest.mark.gpu
def test_set_count_and_sub_frames_under_four_queues(tmp_path):
    """PTSetPassesInFlight(1, 5, 12, 0) and PTSetSubFrames(3) between the passes of one context created under
    GPU_MAX_HW_QUEUES=4: k + 1 passes at every k, so that each count's rotation wraps; the frame is that of the same passes back
    to back.  Mirrors tests/test_gpu_pass_queues.py::test_set_count_and_sub_frames, which runs under the test process's own limit."""
    got = _child(tmp_path, "set_count_and_sub_frames", "4")
    assert int(got["default"][0]) == SETS and int(got["default_again"][0]) == SETS
    assert got["frame"].any()
    assert np.array_equal(got["frame"].view(np.uint32), got["frame1"].view(np.uint32))
    assert np.array_equal(got["stats"], got["stats1"])
