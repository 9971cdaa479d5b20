"""Probe placement on the Sponza-class scene: one JSON line.

The grid: 16 x 8 x 16 probes over the box the first hits of the 1920x1080 camera rays span (tools/probe_volume_bench.py's).  Legs,
alternating in one process, `--legs` times each; every leg is `--steps` calls enqueued back to back after `--warmup` (wall clock):
  place          PTProbePlace, 2,048 probes x 64 samples, 4 iterations (5 traces);
  trace_closest  the rays of the final step (from the placed positions) through PTTraceRays, closest hits only, 5 times;
  trace_surface  the same with PT_QUERY_SURFACE, 5 times: the gap to trace_closest is what learning the face side costs, the gap
                 to place what the ray and step kernels cost;
  lookup         PTProbeGridIrradiance over all first hits, both flags on, on the volume baked at the placed positions;
  lookup_placed  PTProbeGridIrradiancePlaced over the same with the placement: one more 16-byte load per corner with weight.
No ratio is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call; the value in force is reported

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H = 1920, 1080
COUNTS = (16, 8, 16)
SAMPLES, ITERATIONS = 64, 4


def timed(pt, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    pt.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    pt.synchronize()
    return round((time.perf_counter() - t0) / steps * 1e3, 4)


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=8)
    lib = pt.lib
    dev = f"cuda:{pt.device}"
    p = pt.params(seed=0x12345678)

    rays = pt.camera_rays(pixels=torch.arange(W * H, dtype=torch.int32, device=dev), params=p)
    q = rays.clone()
    q[:, 6], q[:, 7] = 1.0e5, 0.0
    hits, surf = pt.trace_rays(q, surface=True)
    ok = hits[:, 3].contiguous().view(torch.int32) != -1
    pos, nrm = surf[ok, 0:3].contiguous(), surf[ok, 4:7].contiguous()
    back = (nrm * rays[ok, 3:6]).sum(dim=1) > 0
    nrm[back] = -nrm[back]
    n = pos.shape[0]
    lo, hi = pos.min(dim=0).values.cpu().numpy(), pos.max(dim=0).values.cpu().numpy()

    t0 = time.perf_counter()
    vol = pt.bake_probe_volume(lo, hi, COUNTS, spp=64, depth_spp=256, relocate=dict(spp=SAMPLES, iterations=ITERATIONS))
    pt.synchronize()
    bake_ms = round((time.perf_counter() - t0) * 1e3, 1)
    probes = vol.sh.shape[0]
    spacing = [vol.grid.spacing[a] for a in range(3)]
    params = abi.probe_place_params(spacing, iterations=ITERATIONS)
    placement = vol.placement.cpu().numpy()
    states = placement[:, 3].copy().view(np.uint32)
    moved = (placement[:, :3] != 0).any(axis=1)

    grid_pos = torch.from_numpy(plugin.probe_grid_positions(vol.grid)).to(dev)
    d_probes = pt._probes(grid_pos, None)
    d_place = torch.zeros((probes, 4), dtype=torch.float32, device=dev)
    # the final step's rays, as PTRay rows
    final = (grid_pos + vol.placement[:, :3]).contiguous()
    d_rays = pt.probe_rays(final, spp=SAMPLES).clone()
    d_rays[:, 6], d_rays[:, 7] = params.maxDistance, 0.0
    nr = d_rays.shape[0]
    d_hits = torch.empty((nr, 4), dtype=torch.float32, device=dev)
    d_surf = torch.empty((nr, 12), dtype=torch.float32, device=dev)

    recv = pt._receivers(pos, nrm, None)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    g = abi.PTProbeGrid.from_buffer_copy(vol.grid)
    g.flags = abi.PT_GRID_WRAP | abi.PT_GRID_VISIBILITY
    g.normalBias = vol.default_normal_bias()
    torch.cuda.synchronize()

    def place():
        plugin.check(lib.PTProbePlace(pt.ctx, d_probes.data_ptr(), probes, 0, SAMPLES, C.byref(params), 0, d_place.data_ptr(), None))

    def trace(flags):
        def fn():
            for _ in range(ITERATIONS + 1):
                plugin.check(lib.PTTraceRays(pt.ctx, d_rays.data_ptr(), nr, flags, d_hits.data_ptr(), d_surf.data_ptr() if flags else None))
        return fn

    def lookup():
        plugin.check(lib.PTProbeGridIrradiance(pt.ctx, C.byref(g), vol._rows.data_ptr(), vol._depth.data_ptr(), recv.data_ptr(), n, out.data_ptr()))

    def lookup_placed():
        plugin.check(lib.PTProbeGridIrradiancePlaced(pt.ctx, C.byref(g), vol._rows.data_ptr(), vol._depth.data_ptr(), vol.placement.data_ptr(), recv.data_ptr(), n,
                                                     out.data_ptr()))

    legs = {"place": place, "trace_closest": trace(abi.PT_QUERY_CLOSEST), "trace_surface": trace(abi.PT_QUERY_SURFACE), "lookup": lookup,
            "lookup_placed": lookup_placed}
    res = {k: [] for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            ms = timed(pt, fn, args.steps, args.warmup)
            print(f"[probe_place_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
    same = bool((d_place.cpu().numpy().view(np.uint32) == placement.view(np.uint32)).all())
    lookup_placed()
    pt.synchronize()
    placed = out.cpu().numpy().copy()
    med = {k: float(np.median(v)) for k, v in res.items()}
    result = {"image": f"{W}x{H}", "queries": n, "grid": list(COUNTS), "probes": probes, "samples": SAMPLES, "iterations": ITERATIONS,
              "max_distance": params.maxDistance, "min_front_distance": params.minFrontDistance, "bake_ms_once": bake_ms,
              "probes_inside": int((states & abi.PT_PROBE_INSIDE != 0).sum()), "probes_moved": int(moved.sum()),
              "steps": args.steps, "warmup": args.warmup, "legs": res, "median_ms_per_call": med,
              "surface_over_closest": round(med["trace_surface"] / med["trace_closest"], 3),
              "place_over_surface": round(med["place"] / med["trace_surface"], 3),
              "lookup_placed_over_lookup": round(med["lookup_placed"] / med["lookup"], 3),
              "place_equals_the_bakes_placement": same, "mean_support_placed": float(placed[:, 3].mean()),
              "finite": bool(np.isfinite(placed).all()), "gpu_max_hw_queues": os.environ["GPU_MAX_HW_QUEUES"],
              "device": torch.cuda.get_device_name(0)}
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
