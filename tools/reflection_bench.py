"""Reflection probes on the Sponza-class scene: one JSON line.

Probes: first hits of the 1920x1080 camera rays (trace_rays(surface=True)), lifted 0.25 off the surface along the normal turned
towards the camera.  Legs, alternating in one process, `--legs` times each; every leg is `--steps` calls enqueued back to back after
`--warmup` (wall clock, as bench.py's headline):
  capture        PTReflectionCapture, 64 probes x 64 x 64 texels x 16 samples (4.2 M paths);
  radiance       PTTraceRadiance over the same 4.2 M rays, made beforehand by PTReflectionRays: the difference is what the rays
                 kernel, the fold and the scratch cost;
  prefilter_64, prefilter_1024      PTReflectionPrefilter at R = 64 with 5 levels;
  prefilter_64_l3                   the same with 3 levels: levels 0 to 2 have 256 outputs or more, so what 5 levels cost beyond it is
                                    the time spent in the levels with fewer than 256 (a level's cost does not depend on its roughness);
  lookup_r0, lookup_r05, lookup_r0_box, lookup_r05_box      PTReflectionLookup of the reflection direction at every first hit;
  sh_irradiance  PTProbeIrradiance over the same count.
Once, outside the legs: PTReflectionPrefilterHost of the 64 probes' maps on `--host-threads` threads.  No ratio is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H = 1920, 1080
PROBES, RES, SAMPLES, LEVELS = 64, 64, 16, 5
MANY = 1024


def timed(pt, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    pt.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    pt.synchronize()
    return round((time.perf_counter() - t0) / steps * 1e3, 3)


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--short", action="store_true", help="profiling runs: one leg of each kind, no host twin")
    args = ap.parse_args()
    if args.short:
        args.legs, args.steps = 1, 2

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=8)
    lib = pt.lib
    dev = f"cuda:{pt.device}"
    p = pt.params(seed=0x12345678)
    p1 = pt._radiance_params(p, spp=1)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)

    rays = pt.camera_rays(pixels=torch.arange(W * H, dtype=torch.int32, device=dev), params=p)
    q = rays.clone()
    q[:, 6], q[:, 7] = 1.0e5, 0.0
    hits, surf = pt.trace_rays(q, surface=True)
    ok = hits[:, 3].contiguous().view(torch.int32) != -1
    pos, nrm, view = surf[ok, 0:3].contiguous(), surf[ok, 4:7].contiguous(), rays[ok, 3:6].contiguous()
    back = (nrm * view).sum(dim=1) > 0
    nrm[back] = -nrm[back]
    n = pos.shape[0]
    refl = (view - 2.0 * (view * nrm).sum(dim=1, keepdim=True) * nrm).contiguous()

    idx = torch.linspace(0, n - 1, PROBES, device=dev).long()
    probe_pos = (pos[idx] + 0.25 * nrm[idx]).contiguous()
    probes = pt._probes(probe_pos, None)
    slots = PROBES * RES * RES * SAMPLES
    base = torch.empty((PROBES, RES * RES, 4), dtype=torch.float32, device=dev)
    d_rays = pt.reflection_rays(probe_pos, res=RES, spp=SAMPLES, params=p)
    d_rad = torch.empty((slots, 4), dtype=torch.float32, device=dev)
    texels = plugin.reflection_texel_count(RES, LEVELS)
    maps = torch.empty((PROBES, texels, 4), dtype=torch.float32, device=dev)
    maps3 = torch.empty((PROBES, plugin.reflection_texel_count(RES, 3), 4), dtype=torch.float32, device=dev)
    many_base = torch.rand((MANY, RES * RES, 4), dtype=torch.float32, device=dev)
    many_maps = torch.empty((MANY, texels, 4), dtype=torch.float32, device=dev)
    # every first hit reads the nearest of the 64 probes along the scanline order it was picked from
    queries = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    queries[:, 0:3], queries[:, 4:7] = pos, refl
    queries.view(torch.int32)[:, 7] = (torch.arange(n, device=dev) * PROBES // n).to(torch.int32)
    q05 = queries.clone()
    q05[:, 3] = 0.5
    lo, hi = pos.min(dim=0).values.cpu().numpy(), pos.max(dim=0).values.cpu().numpy()
    boxes = torch.from_numpy(plugin.reflection_box_rows(np.tile(lo, (PROBES, 1)), np.tile(hi, (PROBES, 1)))).to(dev)
    look_out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    sh = torch.rand((PROBES, 28), dtype=torch.float32, device=dev)
    shq = torch.empty((n, 4), dtype=torch.float32, device=dev)
    shq[:, 0:3] = nrm
    shq.view(torch.int32)[:, 3] = queries.view(torch.int32)[:, 7]
    torch.cuda.synchronize()

    def capture():
        plugin.check(lib.PTReflectionCapture(pt.ctx, C.byref(p), probes.data_ptr(), PROBES, RES, 0, SAMPLES, base.data_ptr()))

    def radiance():
        plugin.check(lib.PTTraceRadiance(pt.ctx, C.byref(p1), d_rays.data_ptr(), slots, d_rad.data_ptr()))

    def prefilter(src, count, levels, dst):
        return lambda: plugin.check(lib.PTReflectionPrefilter(pt.ctx, src.data_ptr(), count, RES, levels, dst.data_ptr()))

    def lookup(rows, bx):
        return lambda: plugin.check(lib.PTReflectionLookup(pt.ctx, maps.data_ptr(), PROBES, RES, LEVELS, probes.data_ptr(), bx.data_ptr() if bx is not None else None,
                                                           rows.data_ptr(), n, look_out.data_ptr()))

    def sh_irradiance():
        plugin.check(lib.PTProbeIrradiance(pt.ctx, sh.data_ptr(), PROBES, shq.data_ptr(), n, look_out.data_ptr()))

    # priming as bench.py: every state set in use allocated and touched
    for _ in range(max(12, pt.passes_in_flight())):
        pt.render_pass_to(p, frame.data_ptr(), 0)
    pt.synchronize()

    legs = {"capture": capture, "radiance": radiance, "prefilter_64": prefilter(base, PROBES, LEVELS, maps), "prefilter_64_l3": prefilter(base, PROBES, 3, maps3),
            "prefilter_1024": prefilter(many_base, MANY, LEVELS, many_maps), "lookup_r0": lookup(queries, None), "lookup_r05": lookup(q05, None),
            "lookup_r0_box": lookup(queries, boxes), "lookup_r05_box": lookup(q05, boxes), "sh_irradiance": sh_irradiance}
    res = {k: [] for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            ms = timed(pt, fn, args.steps, args.warmup)
            print(f"[reflection_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
    med = {k: float(np.median(v)) for k, v in res.items()}
    torch.cuda.synchronize()
    h_base, h_maps = base.cpu().numpy(), maps.cpu().numpy()
    host_ms = None
    if not args.short:
        parts = np.array_split(np.arange(PROBES), args.host_threads)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(args.host_threads) as ex:          # ctypes releases the GIL for the call
            twin = list(ex.map(lambda ix: plugin.reflection_prefilter(h_base[ix], RES, LEVELS), [ix for ix in parts if len(ix)]))
        host_ms = round((time.perf_counter() - t0) * 1e3, 1)
        same = bool((np.concatenate(twin).view(np.uint32) == h_maps.view(np.uint32)).all())
    result = {"image": f"{W}x{H}", "first_hits": int(n), "probes": PROBES, "res": RES, "samples": SAMPLES, "levels": LEVELS, "paths_per_capture": slots,
              "max_bounces": pt.maxRayBounces, "steps": args.steps, "warmup": args.warmup, "schedule": pt.schedule(), "passes_in_flight": pt.passes_in_flight(),
              "legs_ms_per_call": res, "median_ms_per_call": med,
              "capture_minus_radiance_ms": round(med["capture"] - med["radiance"], 3), "radiance_spread_ms": round(max(res["radiance"]) - min(res["radiance"]), 3),
              "prefilter_share_in_levels_below_256_outputs": round((med["prefilter_64"] - med["prefilter_64_l3"]) / med["prefilter_64"], 3),
              "prefilter_host_ms_once": host_ms, "host_threads": args.host_threads,
              "mean_base_rgb": [float(v) for v in h_base[..., :3].mean(axis=(0, 1))], "finite": bool(np.isfinite(h_maps).all() and np.isfinite(look_out.cpu().numpy()).all()),
              "device": torch.cuda.get_device_name(0)}
    if host_ms is not None:
        result["prefilter_kernel_equals_host_twin"] = same
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
