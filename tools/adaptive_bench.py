"""Adaptive passes on the Sponza-class scene at 1920x1080, 8 spp: one JSON line.

Alternating legs of one process, each `--steps` pipelined calls after `--warmup` into two caller-owned frames (wall clock, as
bench.py's headline; Mrays/s = rays traced / elapsed):
  batch<c> / active_all<c>   PTRenderPassBatchTo against PTRenderPassActiveTo with every block active, c passes per call: the
                             difference is the price of the table indirection and of the copy of the frame;
  checker<c> / eighth<c>     PTRenderPassActiveTo over every second block (checkerboard) and every eighth block: the rate per
                             rendered path at 1/2 and 1/8 of the frame, with c = 1 and c = 8 passes per call.
Then PTAccumulateMomentsActiveTo over the same lists against its byte roof (96 B per listed pixel at the project's achievable
HBM rate, 6.3 TB/s), timed with device events on the context's stream."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H, SPP = 1920, 1080, 8
HBM_BYTES_PER_S = 6.3e12


def block_lists(pt):
    rows, cols = pt.block_grid()
    ids = np.arange(rows * cols)
    return {"all": None, "checker": ids[(ids % cols + ids // cols) % 2 == 0], "eighth": ids[ids % 8 == 0]}


def leg(pt, scene, frames, state, kind, ids, count, steps, warmup):
    """Mrays/s and ms per call of `steps` pipelined calls of `count` passes."""
    if kind != "batch":
        pt.set_active_blocks(ids)

    def run(calls):
        for _ in range(calls):
            cur = state["cur"]
            out, acc = frames[cur].data_ptr(), frames[1 - cur].data_ptr()
            seeds = [0x12345678 + state["k"] + j for j in range(count)]
            if kind == "batch":
                ps = [scenes.frame_params(scene, W, H, spp=SPP, current_sample=state["n"] + j * SPP, seed=s) for j, s in enumerate(seeds)]
                pt.render_batch_to(ps, out, acc)
                state["n"] += count * SPP
            else:
                pt.render_active(seeds, d_output=out, d_accumulated=acc)
            state["k"] += count
            state["cur"] = 1 - cur
    run(warmup)
    pt.synchronize()
    pt.reset_stats()
    t0 = time.perf_counter()
    run(steps)
    pt.synchronize()
    elapsed = time.perf_counter() - t0
    st = pt.stats()
    return round(st.rays / elapsed / 1e6, 1), round(elapsed / steps * 1e3, 3), int(st.paths // steps)


def time_calls(pt, fn, launches, reps):
    import torch
    s = torch.cuda.ExternalStream(pt.stream(), device="cuda:0")
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(launches):
            fn()
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b) / launches)
    return float(np.median(ms))


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=SPP)
    frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    lists = block_lists(pt)
    out = {"image": f"{W}x{H}", "spp": SPP, "steps": args.steps, "warmup": args.warmup, "schedule": pt.schedule(),
           "blocks": {k: (int(pt.block_grid()[0] * pt.block_grid()[1]) if v is None else int(v.size)) for k, v in lists.items()}}

    # priming as bench.py: every state set allocated and touched, clocks up; one tracked pass so that the moments exist
    p0 = scenes.frame_params(s, W, H, spp=SPP, current_sample=0, seed=1)
    for _ in range(max(12, pt.passes_in_flight())):
        pt.render_pass_to(p0, frames[0].data_ptr(), 0)
    pt.accumulate_moments(p0, d_output=frames[0].data_ptr())
    pt.synchronize()
    pt.adaptive_begin(current_sample=SPP)
    state = {"cur": 1, "k": 1, "n": SPP}
    out["passes_in_flight"] = pt.passes_in_flight()

    kinds = [("batch", None, c) for c in (8, 1)] + [("active_all", None, c) for c in (8, 1)]
    kinds += [(name, lists[name], c) for name in ("checker", "eighth") for c in (8, 1)]
    res = {f"{name}{c}": {"mrays": [], "ms_per_call": [], "paths_per_call": 0} for name, _, c in kinds}
    for _ in range(args.legs):
        for name, ids, c in kinds:
            mrays, ms, paths = leg(pt, s, frames, state, "batch" if name == "batch" else "active", ids, c, args.steps, args.warmup)
            r = res[f"{name}{c}"]
            r["mrays"].append(mrays)
            r["ms_per_call"].append(ms)
            r["paths_per_call"] = paths
    out["legs"] = res
    med = {k: float(np.median(v["mrays"])) for k, v in res.items()}
    out["active_all_vs_batch_percent"] = {c: round(100.0 * (med[f"active_all{c}"] - med[f"batch{c}"]) / med[f"batch{c}"], 2) for c in (8, 1)}
    out["rate_vs_full_frame"] = {k: round(med[k] / med["batch8"], 3) for k in med}

    # ---- PTAccumulateMomentsActiveTo against its byte roof
    acc = {}
    for name in ("all", "checker", "eighth"):
        pt.set_active_blocks(lists[name])
        listed = int(pt.active_blocks().size) * 256

        def call():
            cur = state["cur"]
            pt.render_active([state["k"]], d_output=frames[cur].data_ptr(), d_accumulated=frames[1 - cur].data_ptr())
            pt.accumulate_moments_active(1, d_output=frames[cur].data_ptr(), d_accumulated=frames[1 - cur].data_ptr())
            state["k"] += 1
            state["cur"] = 1 - cur

        def render_only():
            cur = state["cur"]
            pt.render_active([state["k"]], d_output=frames[cur].data_ptr(), d_accumulated=frames[1 - cur].data_ptr())
            state["k"] += 1
            state["cur"] = 1 - cur
        for _ in range(3):
            call()
        pt.synchronize()
        # the accumulate needs an adaptive call before it: time the pair and the render alone, on the context stream (which waits
        # for each call's resolve), and report the difference
        both = time_calls(pt, call, args.launches, args.reps)
        alone = time_calls(pt, render_only, args.launches, args.reps)
        roof_us = 96.0 * listed / HBM_BYTES_PER_S * 1e6
        acc[name] = {"listed_pixels": listed, "accumulate_us": round((both - alone) * 1e3, 2), "roof_us": round(roof_us, 2)}
    out["accumulate_active"] = acc
    st = pt.noise()
    out["noise"] = {"observations": st.observations, "samples": st.samples, "mean": round(st.meanError, 5)}
    pt.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
