"""Variance tracking on the Sponza-class scene at 1920x1080: one JSON line.

Times (device events on the context's stream around `--launches` calls after a warm-up, median of `--reps`):
  PTAccumulateMomentsTo, PTMeasureNoise (synchronous: its readback and host wait are inside), PTDenoiseMoments at 5 levels.
Bytes: accumulate reads Out and Acc and reads and rewrites both planes (96 B per pixel); the measure kernel reads the frame and
plane 0 (32 B per pixel); both as fractions of the byte roof at the project's achievable HBM rate (6.3 TB/s).
Throughput: bench.py's workload (8 spp passes into two caller-owned frames, pipelined, --steps after --warmup) with an accumulate
after every pass and without, alternating in one process; the cost of tracking is the difference between those legs."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import abi, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H, SPP = 1920, 1080, 8
HBM_BYTES_PER_S = 6.3e12


def time_calls(pt, fn, launches, reps):
    import torch
    s = torch.cuda.ExternalStream(pt.stream(), device="cuda:0")
    for _ in range(3):
        fn()
    pt.synchronize()
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


def throughput_leg(pt, scene, frames, steps, warmup, track):
    """bench.py's timed region: Mrays/s over `steps` pipelined passes (wall clock, as its headline)."""
    def run(k0, k1, cur):
        for k in range(k0, k1):
            p = scenes.frame_params(scene, W, H, spp=SPP, current_sample=k * SPP, seed=0x12345678 + k)
            acc = frames[1 - cur].data_ptr() if k > 0 else 0
            pt.render_pass_to(p, frames[cur].data_ptr(), acc)
            if track:
                pt.accumulate_moments(p, d_output=frames[cur].data_ptr(), d_accumulated=acc)
            cur = 1 - cur
        return cur
    cur = run(0, warmup, 0)
    pt.synchronize()
    pt.reset_stats()
    t0 = time.perf_counter()
    run(warmup, warmup + steps, cur)
    pt.synchronize()
    elapsed = time.perf_counter() - t0
    return pt.stats().rays / elapsed / 1e6


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", type=int, default=3, help="throughput legs of each kind, alternating untracked / tracked")
    args = ap.parse_args()
    out = {"image": f"{W}x{H}", "launches": args.launches, "reps": args.reps, "iterations": args.iterations}

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=SPP)
    frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()

    # ---- throughput with and without tracking (priming as bench.py: every state set allocated and touched, clocks up)
    p0 = scenes.frame_params(s, W, H, spp=SPP, current_sample=0, seed=1)
    for _ in range(max(12, pt.passes_in_flight())):
        pt.render_pass_to(p0, frames[0].data_ptr(), 0)
    pt.accumulate_moments(p0, d_output=frames[0].data_ptr())            # allocates the planes outside the timed legs
    pt.synchronize()
    legs = {"untracked": [], "tracked": []}
    for _ in range(args.legs):
        for kind in ("untracked", "tracked"):
            legs[kind].append(round(throughput_leg(pt, s, frames, args.steps, args.warmup, kind == "tracked"), 1))
    out["passes_in_flight"] = pt.passes_in_flight()
    out["mrays_untracked"] = legs["untracked"]
    out["mrays_tracked"] = legs["tracked"]
    mu, mt = float(np.median(legs["untracked"])), float(np.median(legs["tracked"]))
    out["tracking_cost_percent"] = round(100.0 * (mu - mt) / mu, 2)

    # ---- the calls themselves; the last tracked leg left >= 2 observations and frames[...] as the frame last accumulated
    k, samples, _, _ = pt.moments_info()
    state = {"n": samples, "cur": 0}

    def accumulate():
        p = scenes.frame_params(s, W, H, spp=SPP, current_sample=state["n"], seed=0)
        pt.accumulate_moments(p, d_output=frames[state["cur"]].data_ptr(), d_accumulated=frames[1 - state["cur"]].data_ptr())
        state["n"] += SPP
        state["cur"] = 1 - state["cur"]
    us = time_calls(pt, accumulate, args.launches, args.reps) * 1e3
    roof = 96.0 * W * H / HBM_BYTES_PER_S * 1e6
    out["accumulate_us"] = round(us, 2)
    out["accumulate_roof_us"] = round(roof, 2)
    out["accumulate_roof_fraction"] = round(roof / us, 3)

    us = time_calls(pt, lambda: pt.noise(), args.launches, args.reps) * 1e3
    roof = 32.0 * W * H / HBM_BYTES_PER_S * 1e6
    out["measure_us"] = round(us, 2)
    out["measure_roof_us"] = round(roof, 2)
    out["measure_roof_fraction"] = round(roof / us, 3)
    st = pt.noise()
    out["noise"] = {"observations": st.observations, "samples": st.samples, "mean": round(st.meanError, 5),
                    "p95_upper_edge": round(st.percentileError, 5), "below_2_percent": round(st.pixelsBelow / st.pixels, 4)}

    pt.render_guides(1, p0)
    dst = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    dp = abi.denoise_params(iterations=args.iterations)
    out["denoise_moments_ms"] = round(time_calls(pt, lambda: pt.denoise(dp, d_dst=dst.data_ptr(), variance="moments"), args.launches, args.reps), 4)
    out["denoise_spatial_ms"] = round(time_calls(pt, lambda: pt.denoise(dp, d_src=frames[0].data_ptr(), d_dst=dst.data_ptr()), args.launches, args.reps), 4)
    pt.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
