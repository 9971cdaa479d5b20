"""Adaptive gathers on the Sponza-class chart of tools/lightmap_denoise_bench.py at 1024^2: one JSON line.

Legs, alternating in one process, `--legs` times each; every leg is `--steps` calls after `--warmup`, wall clock around a final
synchronise:
  adaptive        PTGatherIrradianceAdaptive at --min / --add / --max (16 / 16 / 256) and `--threshold` (default: the square root of
                  the median of the criterion v / d^2 of a --min-sample gather, so that about half the texels stop after round 0);
  rounds_synced   the same rounds as plain PTGatherIrradiance calls over the same compacted receiver lists with a synchronise after
                  every round, as the loop has: adaptive minus this is the time spent outside the gather rounds (select, fold and
                  the count read-back);
  rounds_alone    those calls enqueued back to back with one synchronise at the end: rounds_synced minus this is what the
                  per-round synchronisation costs;
  uniform_equal   PTGatherIrradiance with the adaptive call's total number of paths divided by the receivers, rounded up;
  uniform_max     PTGatherIrradiance at --max samples.
Then the error of each of the three results against a `--reference`-sample gather of the same receivers over a disjoint sample
range: mean and 95th percentile of |lum - lum_ref| / max(lum_ref, darkFloor).  Nothing is asserted."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402
from lightmap_bench import grid_atlas, timed  # noqa: E402

SIZE = 1024


def luminance(e):
    return e[:, 0].double() * 0.299 + e[:, 1].double() * 0.587 + e[:, 2].double() * 0.114


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--min", type=int, default=16, dest="min_samples")
    ap.add_argument("--add", type=int, default=16, dest="add_samples")
    ap.add_argument("--max", type=int, default=256, dest="max_samples")
    ap.add_argument("--threshold", type=float, default=None, help="default: the median of the criterion after round 0")
    ap.add_argument("--reference", type=int, default=4096, help="samples of the reference gather (0: no error figures)")
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=256, height=256, samplesPerPass=1)
    lib = pt.lib
    dev = torch.device(f"cuda:{pt.device}")
    uvs, _ = grid_atlas(len(s.tri_attrs))
    p = pt.params(seed=0x12345678)
    texels, recv = pt.chart_receivers(SIZE, SIZE, uvs=torch.from_numpy(uvs).to(dev))
    n = recv.shape[0]
    print(f"[adaptive_gather_bench] {SIZE}: {n} receivers", file=sys.stderr, flush=True)

    # the criterion after round 0
    r0 = pt.irradiance(receivers=recv, spp=args.min_samples, params=p)
    l0 = luminance(r0)
    finite = torch.isfinite(r0).all(dim=1)
    dark = 0.01 * float(l0[finite].mean().item())
    S = float(args.min_samples)
    v0 = torch.clamp((r0[:, 3].double() - S * l0 * l0) / (S - 1.0), min=0.0) / S
    criterion = v0 / torch.clamp(l0, min=dark) ** 2
    threshold = args.threshold if args.threshold is not None else float(torch.sqrt(criterion[finite].median()).item())

    a = abi.adaptive_gather(threshold, args.min_samples, args.add_samples, args.max_samples, dark)
    out, counts = torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    plain = torch.empty((n, 4), dtype=torch.float32, device=dev)
    st = abi.PTAdaptiveGatherStats()
    torch.cuda.synchronize(dev)

    def adaptive():
        plugin.check(lib.PTGatherIrradianceAdaptive(pt.ctx, C.byref(p), C.byref(a), recv.data_ptr(), n, out.data_ptr(), counts.data_ptr(), C.byref(st)))

    adaptive()
    stats = st.as_dict()
    uniform_spp = -(-stats["samples"] // n)
    # the rounds' own lists: round r >= 1 gathers the entries whose final count is beyond min + (r - 1) * add
    lists = [recv] + [recv[counts > args.min_samples + r * args.add_samples].contiguous() for r in range(stats["rounds"] - 1)]
    assert sum(x.shape[0] * (args.min_samples if r == 0 else args.add_samples) for r, x in enumerate(lists)) == stats["samples"]
    torch.cuda.synchronize(dev)

    def gather(rows, first, spp):
        plugin.check(lib.PTGatherIrradiance(pt.ctx, C.byref(p), rows.data_ptr(), rows.shape[0], first, spp, plain.data_ptr()))

    def rounds(synced):
        first = 0
        for r, rows in enumerate(lists):
            spp = args.min_samples if r == 0 else args.add_samples
            gather(rows, first, spp)
            if synced:
                pt.synchronize()
            first += spp

    legs = {"adaptive": adaptive, "rounds_synced": lambda: rounds(True), "rounds_alone": lambda: rounds(False), "uniform_equal": lambda: gather(recv, 0, uniform_spp),
            "uniform_max": lambda: gather(recv, 0, args.max_samples)}
    res = {k: [] for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            ms = timed((pt,), fn, args.steps, args.warmup)
            print(f"[adaptive_gather_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
    med = {k: float(np.median(v)) for k, v in res.items()}

    errors = {}
    if args.reference:
        lum_ref = luminance(pt.irradiance(receivers=recv, spp=args.reference, first_sample=1 << 20, params=p))
        results = {"adaptive": out, "uniform_equal": pt.irradiance(receivers=recv, spp=uniform_spp, params=p),
                   "uniform_max": pt.irradiance(receivers=recv, spp=args.max_samples, params=p)}
        for name, e in results.items():
            rel = (luminance(e) - lum_ref).abs() / torch.clamp(lum_ref, min=dark)
            rel = rel[torch.isfinite(rel)]
            errors[name] = {"mean": float(rel.mean().item()), "p95": float(torch.quantile(rel, 0.95).item())}
    cnt = counts.cpu().numpy()
    values, freq = np.unique(cnt, return_counts=True)
    outside = med["adaptive"] - med["rounds_synced"]
    result = {"receivers": n, "min": args.min_samples, "add": args.add_samples, "max": args.max_samples, "threshold": threshold, "dark_floor": dark,
              "steps": args.steps, "warmup": args.warmup, "stats": stats, "stopped_after_round0": round(float((cnt == args.min_samples).mean()), 4),
              "count_histogram": {int(k): int(c) for k, c in zip(values, freq)}, "legs_ms_per_call": res, "median_ms_per_call": med,
              "paths": {"adaptive": stats["samples"], "uniform_equal": n * uniform_spp, "uniform_max": n * args.max_samples},
              "uniform_equal_spp": uniform_spp, "outside_gather_rounds_ms": round(outside, 3),
              "outside_gather_rounds_share": round(outside / med["adaptive"], 4), "outside_ms_per_round": round(outside / stats["rounds"], 4),
              "per_round_synchronisation_ms": round(med["rounds_synced"] - med["rounds_alone"], 3),
              "relative_luminance_error": errors, "reference_samples": args.reference,
              "finite": bool(torch.isfinite(out).all().item()), "device": torch.cuda.get_device_name(0)}
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
