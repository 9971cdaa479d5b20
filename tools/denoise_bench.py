"""Guides and denoising on the Sponza-class scene at 1920x1080: one JSON line.

Times (device events on the context's stream around `--launches` calls after a warm-up, median of `--reps`):
  guides at S = 1 and S = 4 (PTRenderGuides), denoising at 5 levels (PTDenoise, one 4 spp pass as input).
Bytes: what the filter algorithm moves through HBM per launch at least (each pixel's state, guides and input read once and
its results written once; the taps themselves are served from LDS / L2 / the Infinity Cache), over the measured time."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import abi, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H = 1920, 1080


def filter_bytes(pixels, iterations):
    """Minimum HBM bytes per PTDenoise: prepass reads colour, albedo, normal+depth (48 B) and writes state + depth gradient
    (24 B); a level reads state, normal+depth, gradient (40 B) and writes state (16 B); remodulation reads colour, albedo,
    state (48 B) and writes the output (16 B)."""
    return pixels * (72 + iterations * 56 + 64)


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


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=5)
    args = ap.parse_args()
    out = {"image": f"{W}x{H}", "launches": args.launches, "reps": args.reps, "iterations": args.iterations}

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=4)
    p = pt.params(seed=1)
    pt.render_pass(p)
    for n in (1, 4):
        out[f"guides_s{n}_ms"] = round(time_calls(pt, lambda: pt.render_guides(n, p), args.launches, args.reps), 4)
    pt.render_guides(1, p)
    dst = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    dp = abi.denoise_params(iterations=args.iterations)
    ms = time_calls(pt, lambda: pt.denoise(dp, d_dst=dst.data_ptr()), args.launches, args.reps)
    nbytes = filter_bytes(W * H, args.iterations)
    out["denoise_ms"] = round(ms, 4)
    out["denoise_launches"] = args.iterations + 2
    out["denoise_bytes"] = nbytes
    out["denoise_gb_s"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
    out["coverage"] = round(float(pt.guides()[0][..., 3].mean()), 4)
    pt.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
