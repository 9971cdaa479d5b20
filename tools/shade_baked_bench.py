"""Shading from the bakes on the Sponza-class scene: one JSON line.

The 1920x1080 first hits (PTShadeBakedFrame's own rays, traced once) are shaded from a 16 x 8 x 16 probe volume with a placement and
from 64 reflection probes at R = 64 with 5 levels and boxes.  Legs, alternating in one process, `--legs` times each; every leg is
`--steps` calls enqueued back to back after `--warmup` (wall clock, as bench.py's headline):
  fused          PTShadeBaked over the first hits;
  composition    PTShadeSurfaces, PTProbeGridIrradiancePlaced, PTReflectionLookup, PTShadeCompose over the same, through 128 bytes
                 per entry of terms, receivers and queries written and read again and 32 of irradiance and radiance;
  frame          PTShadeBakedFrame whole: rays, the closest-hit walk with surface records, the fused kernel;
  query          PTTraceRays with surface records over the frame's rays: what of `frame` is the walk;
  dfg_32         PTBakeDFG at 32.
Once, outside the legs: PTBakeDFGHost at 32 on one thread.  The fused result is compared with the composition's bit for bit.  No
ratio is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H = 1920, 1080
GRID = (16, 8, 16)
PROBES, RES, LEVELS = 64, 64, 5


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
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--short", action="store_true", help="profiling runs: one leg of each kind, two calls")
    args = ap.parse_args()
    if args.short:
        args.legs, args.steps = 1, 2

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=8)
    lib = pt.lib
    dev = torch.device(f"cuda:{pt.device}")
    p = pt.params(seed=0x12345678)
    v = s.vertices[:, :3]
    lo, hi = v.min(0), v.max(0)
    pad = (hi - lo) * 0.04
    volume = pt.bake_probe_volume(lo + pad, hi - pad, GRID, spp=64, depth_spp=64, relocate=dict(spp=32, iterations=2))
    rng = np.random.default_rng(3)
    pos = (lo + pad + rng.random((PROBES, 3)) * (hi - lo - 2 * pad)).astype(np.float32)
    half = (hi - lo) * 0.2
    refl = pt.capture_reflection_probes(pos, res=RES, spp=4, levels=LEVELS, boxes=(pos - half, pos + half))
    dfg = pt.bake_dfg(32)
    inputs, keep = pt._shade_inputs(volume, refl, dfg)

    n = W * H
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    plugin.check(lib.PTShadeBakedFrame(pt.ctx, C.byref(p), C.byref(inputs), out.data_ptr(), rays.data_ptr()))
    pt.synchronize()
    hits, surf = pt.trace_rays(rays, surface=True)
    mat, terms, recv, qr = (torch.empty((n, c), dtype=torch.float32, device=dev) for c in (12, 12, 8, 8))
    irr, spec, out4 = (torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(3))
    dfg_out = torch.empty((32, 32, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def fused():
        plugin.check(lib.PTShadeBaked(pt.ctx, C.byref(inputs), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr()))

    def composition():
        plugin.check(lib.PTShadeSurfaces(pt.ctx, rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, refl.probe_rows.data_ptr(), refl.box_rows.data_ptr(), PROBES,
                                         None, terms.data_ptr(), recv.data_ptr(), qr.data_ptr()))
        plugin.check(lib.PTProbeGridIrradiancePlaced(pt.ctx, C.byref(inputs.grid), volume._rows.data_ptr(), volume._depth.data_ptr(), volume.placement.data_ptr(),
                                                     recv.data_ptr(), n, irr.data_ptr()))
        plugin.check(lib.PTReflectionLookup(pt.ctx, refl.maps.data_ptr(), PROBES, RES, LEVELS, refl.probe_rows.data_ptr(), refl.box_rows.data_ptr(), qr.data_ptr(), n,
                                            spec.data_ptr()))
        plugin.check(lib.PTShadeCompose(pt.ctx, terms.data_ptr(), irr.data_ptr(), spec.data_ptr(), n, dfg.data_ptr(), 32, out4.data_ptr()))

    def frame():
        plugin.check(lib.PTShadeBakedFrame(pt.ctx, C.byref(p), C.byref(inputs), out.data_ptr(), None))

    def query():
        plugin.check(lib.PTTraceRays(pt.ctx, rays.data_ptr(), n, abi.PT_QUERY_CLOSEST | abi.PT_QUERY_SURFACE, hits.data_ptr(), surf.data_ptr()))

    def dfg_32():
        plugin.check(lib.PTBakeDFG(pt.ctx, 32, dfg_out.data_ptr()))

    legs = {"fused": fused, "composition": composition, "frame": frame, "query": query, "dfg_32": dfg_32}
    res = {k: [] for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            ms = timed(pt, fn, args.steps, args.warmup)
            print(f"[shade_baked_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
    med = {k: float(np.median(x)) for k, x in res.items()}
    fused()
    composition()
    pt.synchronize()
    torch.cuda.synchronize()
    same = bool((out.cpu().numpy().view(np.uint32) == out4.cpu().numpy().view(np.uint32)).all())
    t0 = time.perf_counter()
    twin = plugin.bake_dfg(32)
    host_ms = round((time.perf_counter() - t0) * 1e3, 2)
    prim = hits.cpu().numpy().view(np.uint32)[:, 3]
    result = {"image": f"{W}x{H}", "entries": n, "first_hits": int((prim != 0xFFFFFFFF).sum()), "grid": list(GRID), "probes": PROBES, "res": RES, "levels": LEVELS,
              "dfg_res": 32, "steps": args.steps, "warmup": args.warmup, "legs_ms_per_call": res, "median_ms_per_call": med,
              "fused_over_composition": round(med["fused"] / med["composition"], 3), "fused_spread_ms": round(max(res["fused"]) - min(res["fused"]), 4),
              "composition_spread_ms": round(max(res["composition"]) - min(res["composition"]), 4),
              "frame_minus_query_ms": round(med["frame"] - med["query"], 4), "dfg_host_ms_once": host_ms,
              "fused_equals_composition": same, "dfg_kernel_equals_host_twin": bool((dfg_out.cpu().numpy().view(np.uint32) == twin.view(np.uint32)).all()),
              "mean_rgb": [float(x) for x in out.cpu().numpy()[:, :3].mean(axis=0)], "finite": bool(np.isfinite(out.cpu().numpy()).all()),
              "device": torch.cuda.get_device_name(0)}
    del keep
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
