"""Direct light at the first hits of the 1920x1080 frame on the Sponza-class scene (or, with --scene instanced, on the HAS_TLAS
scene), the scene's own lights: one JSON line.

For S = 1 and S = 4, legs alternating in one process, `--legs` times each; every leg is `--steps` calls enqueued back to back
after `--warmup` (wall clock, as bench.py's headline):
  direct_light       PTDirectLight, the fused call: material fetch, terms, the pairs and their walks in one kernel;
  shade_surfaces     PTShadeSurfaces over the same hits (terms and receivers out);
  direct_rays        PTDirectRays: 48 bytes stored per pair;
  trace_anyhit       PTTraceRays(PT_QUERY_ANY_HIT) over the pair rays;
  accumulate         PTDirectAccumulate;
  frame_mixed        PTShadeMixedFrame;
  frame_lightmapped  PTShadeLightmappedFrame (nothing bound: the volume lights every hit).
The yardstick is made of kernels that Part 24 does not touch: trace_anyhit + shade_surfaces.  PTDirectLight does the work of both
minus the per-pair traffic, plus the BRDF.  The margin is the spread of the yardstick's own legs.  The fused result is compared
with the four-call composition bit for bit.  No ratio is asserted."""
import argparse
import ctypes as C
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402
from shade_baked_bench import H, W, timed  # noqa: E402

GRID, PROBES, RES, LEVELS = (8, 4, 8), 8, 16, 3


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--short", action="store_true", help="profiling runs: one leg of each kind, two calls")
    ap.add_argument("--scene", default="sponza", choices=["sponza", "instanced"], help="instanced: the HAS_TLAS scene (200 instances, one rectangle light): pt_direct_light_tlas")
    args = ap.parse_args()
    if args.short:
        args.legs, args.steps = 1, 2

    s = scenes.sponza_atrium() if args.scene == "sponza" else scenes.instanced_scene(count=200, detail=24)
    pt = PathTracer(s, width=W, height=H, samplesPerPass=8)
    lib = pt.lib
    dev = torch.device(f"cuda:{pt.device}")
    p = pt.params(seed=0x12345678)
    if args.scene == "sponza":
        v = s.vertices[:, :3]
        lo, hi = v.min(0), v.max(0)
    else:                                                        # the meshes are in local space: a box around what the camera looks at
        eye, target = np.asarray(s.camera.eye, np.float32), np.asarray(s.camera.target, np.float32)
        r = np.float32(0.6) * np.linalg.norm(target - eye).astype(np.float32)
        lo, hi = target - r, target + r
    pad = (hi - lo) * 0.04
    with pt.muted_lights():                                      # the bakes hold sky, emissive surfaces and bounces only
        volume = pt.bake_probe_volume(lo + pad, hi - pad, GRID, spp=16, depth_spp=16)
        rng = np.random.default_rng(3)
        pos = (lo + pad + rng.random((PROBES, 3)) * (hi - lo - 2 * pad)).astype(np.float32)
        refl = pt.capture_reflection_probes(pos, res=RES, spp=4, levels=LEVELS)
    dfg = pt.bake_dfg(32)
    inputs, keep = pt._shade_inputs(volume, refl, dfg)

    n = W * H
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    plugin.check(lib.PTShadeLightmappedFrame(pt.ctx, C.byref(p), C.byref(inputs), out.data_ptr(), rays.data_ptr()))
    pt.synchronize()
    hits, surf = pt.trace_rays(rays, surface=True)
    terms = torch.empty((n, 12), dtype=torch.float32, device=dev)
    recv = torch.empty((n, 8), dtype=torch.float32, device=dev)
    a = (rays.data_ptr(), hits.data_ptr(), surf.data_ptr())
    kinds = pt.light_records()[:, 3].copy().view(np.uint32)
    result = {"scene": s.name, "has_tlas": bool(s.use_tlas), "image": f"{W}x{H}", "entries": n, "first_hits": int((hits.cpu().numpy().view(np.uint32)[:, 3] != 0xFFFFFFFF).sum()),
              "triangles": s.vertices.shape[0] // 3, "instances": len(s.instances) if s.use_tlas else 0, "lights": {"rectangle": int((kinds == 3).sum()), "point": int((kinds == 2).sum()), "spot": int((kinds == 0).sum())},
              "steps": args.steps, "warmup": args.warmup, "strata": {}}

    for strata in (1, 4):
        d = abi.direct_params(strata=strata, seed=7)
        pairs = pt.direct_pair_count(strata)
        pair_rays = torch.empty((n * pairs, 8), dtype=torch.float32, device=dev)
        contrib = torch.empty((n * pairs, 4), dtype=torch.float32, device=dev)
        pair_hits = torch.empty((n * pairs, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def direct_light():
            plugin.check(lib.PTDirectLight(pt.ctx, C.byref(d), *a, n, out.data_ptr()))

        def shade_surfaces():
            plugin.check(lib.PTShadeSurfaces(pt.ctx, *a, n, None, None, 0, None, terms.data_ptr(), recv.data_ptr(), None))

        def direct_rays():
            plugin.check(lib.PTDirectRays(pt.ctx, C.byref(d), rays.data_ptr(), terms.data_ptr(), recv.data_ptr(), n, pair_rays.data_ptr(), contrib.data_ptr()))

        def trace_anyhit():
            plugin.check(lib.PTTraceRays(pt.ctx, pair_rays.data_ptr(), n * pairs, abi.PT_QUERY_ANY_HIT, pair_hits.data_ptr(), None))

        def accumulate():
            plugin.check(lib.PTDirectAccumulate(pt.ctx, terms.data_ptr(), contrib.data_ptr(), pair_hits.data_ptr(), n, pairs, out.data_ptr()))

        def frame_mixed():
            plugin.check(lib.PTShadeMixedFrame(pt.ctx, C.byref(p), C.byref(inputs), C.byref(d), out.data_ptr(), None))

        def frame_lightmapped():
            plugin.check(lib.PTShadeLightmappedFrame(pt.ctx, C.byref(p), C.byref(inputs), out.data_ptr(), None))

        legs = {"direct_light": direct_light, "shade_surfaces": shade_surfaces, "direct_rays": direct_rays, "trace_anyhit": trace_anyhit,
                "accumulate": accumulate, "frame_mixed": frame_mixed, "frame_lightmapped": frame_lightmapped}
        res = {k: [] for k in legs}
        for _ in range(args.legs):
            for name, fn in legs.items():                        # in this order: every step reads what the one before wrote
                ms = timed(pt, fn, args.steps, args.warmup)
                print(f"[direct_light_bench] S = {strata} {name}: {ms} ms per call", file=sys.stderr, flush=True)
                res[name].append(ms)
        med = {k: float(np.median(x)) for k, x in res.items()}
        spread = {k: round(max(x) - min(x), 4) for k, x in res.items()}
        yard = [t + q for t, q in zip(res["trace_anyhit"], res["shade_surfaces"])]
        yard_med, yard_spread = float(np.median(yard)), round(max(yard) - min(yard), 4)
        steps_sum = sum(med[k] for k in ("shade_surfaces", "direct_rays", "trace_anyhit", "accumulate"))
        # the equality on this data
        direct_light()
        pt.synchronize()                                         # the calls run on the context's stream, torch's copies on its own
        got = out.clone()
        torch.cuda.synchronize()
        shade_surfaces(); direct_rays(); trace_anyhit(); accumulate()
        pt.synchronize()
        same = bool((got.cpu().numpy().view(np.uint32) == out.cpu().numpy().view(np.uint32)).all())
        counting = float((pair_rays[:, 6] > 0).float().mean())
        occluded = float(((pair_hits.view(torch.int32)[:, 3] != -1) & (pair_rays[:, 6] > 0)).float().mean())
        g = got.cpu().numpy()
        result["strata"][str(strata)] = {
            "pairs_per_entry": pairs, "pair_bytes": n * pairs * 64, "pairs_that_count": round(counting, 4), "pairs_occluded": round(occluded, 4),
            "legs_ms_per_call": res, "median_ms_per_call": med, "spread_ms": spread, "yardstick_ms": round(yard_med, 4), "yardstick_spread_ms": yard_spread,
            "direct_light_minus_yardstick_ms": round(med["direct_light"] - yard_med, 4),
            "direct_light_within_yardstick_plus_its_spread": bool(med["direct_light"] <= yard_med + yard_spread),
            "composition_steps_sum_ms": round(steps_sum, 4), "direct_light_over_steps_sum": round(med["direct_light"] / steps_sum, 3),
            "frame_mixed_minus_lightmapped_ms": round(med["frame_mixed"] - med["frame_lightmapped"], 4),
            "direct_light_equals_composition": same, "mean_rgb": [float(x) for x in g[:, :3].mean(axis=0)], "finite": bool(np.isfinite(g).all())}
        del pair_rays, contrib, pair_hits
    result["device"] = torch.cuda.get_device_name(0)
    del keep
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
