"""Direct light over many lights at the first hits of the 1920x1080 frame on the Sponza-class scene (or, with --scene instanced, on
the HAS_TLAS scene of direct_light_bench.py: pt_direct_light_tlas against pt_direct_light_grid_tlas): PTDirectLight against
PTDirectLightCulled (include/ptmi_plugin.h Part 25).  One JSON line.

The scene's two lights are replaced, through scene construction, by lattices of 64, 256 and 1,024 local lights -- a third point,
a third spot pointing down, a third rectangle facing down -- with a range of 0.8 lattice spacings; the light grid's cells are one
range wide.  Legs, alternating in one process, `--legs` times each; every leg is `--steps` calls enqueued back to back after
`--warmup` (wall clock, as bench.py's headline):
  S = 1 jittered and centred at every light count, S = 4 jittered at 256 lights: `unculled` (PTDirectLight) and `culled`;
  `build`: PTBuildLightGrid on its own (it holds one stream synchronisation);
  the scene's own two lights through both calls: what the union merge costs when there is nothing to cull.
The yardstick is PTDirectLight on the same lights: `pt_direct_light`, which this change leaves as it was.  The two outputs are
compared bit for bit at full size on every leg; a difference ends the run with an error.  No ratio is asserted."""
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

F = np.float32


def lattice(lo, hi, dims):
    """(lights (n, 16), spacing): dims[0] x dims[1] x dims[2] lights inside the box, the types in turn"""
    ext = (hi - lo).astype(np.float64)
    spacing = float((ext.prod() / np.prod(dims)) ** (1.0 / 3.0))
    rng_ = 0.8 * spacing
    out, k = [], 0
    for iy in range(dims[1]):
        for iz in range(dims[2]):
            for ix in range(dims[0]):
                p = lo + ext * ((ix + 0.5) / dims[0], (iy + 0.5) / dims[1], (iz + 0.5) / dims[2])
                colour = (6.0 + (k % 5), 5.0 + (k % 3), 4.0 + (k % 7))
                if k % 3 == 0:
                    out.append(scenes.pack_point_light(p, colour, rng=rng_))
                elif k % 3 == 1:
                    out.append(scenes.pack_spot_light(p, (0.0, -1.0, 0.0), 120.0, 90.0, colour, intensity=2.0, rng=rng_))
                else:
                    side = 0.1 * spacing
                    out.append(scenes.pack_rect_light(center=p, right=(1, 0, 0), up=(0, 0, 1), size=(side, side), color=colour, intensity=8.0 / side ** 2,
                                                      rng=rng_))
                k += 1
    return np.stack(out).astype(F), rng_


def cells_of(origin, size, dims, X):
    t = (X - np.asarray(origin, F)[None]) / F(size)
    inside = ((t >= 0) & (t < np.asarray(dims, F)[None])).all(axis=1)
    i = np.where(inside[:, None], t, 0).astype(np.uint32)
    return np.where(inside, (i[:, 2] * dims[1] + i[:, 1]) * dims[0] + i[:, 0], int(np.prod(dims)))


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--short", action="store_true", help="profiling runs: one leg of each kind, two calls")
    ap.add_argument("--detail", type=float, default=1.0, help="the scene's tessellation (1: the benchmark's 250,752 triangles)")
    ap.add_argument("--scene", default="sponza", choices=["sponza", "instanced"], help="instanced: the HAS_TLAS scene (200 instances): the _tlas kernels")
    args = ap.parse_args()
    if args.short:
        args.legs, args.steps = 1, 2

    def make_scene():
        return scenes.sponza_atrium(detail=args.detail) if args.scene == "sponza" else scenes.instanced_scene(count=200, detail=24)

    base = make_scene()
    if args.scene == "sponza":
        v = base.vertices[:, :3]
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    else:                                                        # the instances' world boxes: the context knows them
        probe = PathTracer(base, width=W, height=H, samplesPerPass=8)
        lo, hi = (np.asarray(b, np.float64) for b in probe._scene_bounds())
        probe.close()
    result = {"scene": base.name, "image": f"{W}x{H}", "entries": W * H, "triangles": base.vertices.shape[0] // 3, "steps": args.steps, "warmup": args.warmup,
              "configs": {}}
    configs = [("own", None, ((1, False),)), ("64", (4, 4, 4), ((1, False), (1, True))), ("256", (8, 4, 8), ((1, False), (1, True), (4, False))),
               ("1024", (16, 4, 16), ((1, False), (1, True)))]
    rays = hits = surf = None
    for name, dims, modes in configs:
        s = make_scene()
        if dims is None:
            cell = float((hi - lo).max() / 16)
        else:
            s.lights, cell = lattice(lo + (hi - lo) * 0.02, hi - (hi - lo) * 0.02, dims)
        pt = PathTracer(s, width=W, height=H, samplesPerPass=8)
        lib = pt.lib
        dev = torch.device(f"cuda:{pt.device}")
        n = W * H
        if rays is None:                                         # the first hits are the geometry's: made once
            rays = pt.camera_rays(torch.arange(n, dtype=torch.int32, device=dev), seed=0x12345678).contiguous()
            rays[:, 6], rays[:, 7] = 1e30, 0.0                  # a PTRay: tmax and the reserved word in place of the RNG state
        hits, surf = pt.trace_rays(rays, surface=True)
        out_a = torch.empty((n, 4), dtype=torch.float32, device=dev)
        out_b = torch.empty((n, 4), dtype=torch.float32, device=dev)
        a = (rays.data_ptr(), hits.data_ptr(), surf.data_ptr())
        glo = lo.astype(F)                                       # the grid: cubes of one range over the scene's box
        gdims = tuple(int(d) for d in np.maximum(np.ceil((hi - lo) / cell * (1 + 1e-6)), 1))
        info = pt.build_light_grid(glo, cell, gdims)
        offsets, _, _ = pt.light_grid()
        _, terms, recv, _ = pt.shade_surfaces(rays, hits, surf)
        terms, recv = terms.cpu().numpy(), recv.cpu().numpy()
        hit = terms[:, 7] > 0
        O = recv[hit, 0:3] + recv[hit, 4:7] * F(0.0001)
        cell_of_entry = cells_of(glo, cell, gdims, O)
        lengths = np.diff(offsets.astype(np.int64))
        per_entry = lengths[cell_of_entry]
        L = int(info["lightCount"])
        g = abi.light_grid_params(glo, cell, gdims)
        torch.cuda.synchronize()                                 # the calls below go to the context's stream directly

        def build():
            plugin.check(lib.PTBuildLightGrid(pt.ctx, C.byref(g)))

        build_ms = [timed(pt, build, args.steps, args.warmup) for _ in range(args.legs)]
        cfg = {"lights": L, "range": round(cell, 4), "grid": {"dims": [int(d) for d in gdims], "cell": round(cell, 4), "cells": info["cells"], "entries": info["entries"],
                                                               "longest_list": info["longest"], "mean_list_over_cells": round((info["entries"] - L) / info["cells"], 3),
                                                               "mean_list_over_entries": round(float(per_entry.mean()), 3), "max_list_over_entries": int(per_entry.max()),
                                                               "entries_in_overflow_cell": int((cell_of_entry == info["cells"]).sum())},
               "first_hits": int(hit.sum()), "build_ms": build_ms, "build_median_ms": float(np.median(build_ms)), "modes": {}}
        for strata, centred in modes:
            d = abi.direct_params(strata=strata, seed=7, centered=centred)

            def unculled():
                plugin.check(lib.PTDirectLight(pt.ctx, C.byref(d), *a, n, out_a.data_ptr()))

            def culled():
                plugin.check(lib.PTDirectLightCulled(pt.ctx, C.byref(d), *a, n, out_b.data_ptr()))

            res = {"unculled": [], "culled": []}
            for _ in range(args.legs):
                for leg, fn in (("unculled", unculled), ("culled", culled)):
                    ms = timed(pt, fn, args.steps, args.warmup)
                    print(f"[many_lights_bench] {name} lights, S = {strata}{' centred' if centred else ''}, {leg}: {ms} ms per call", file=sys.stderr, flush=True)
                    res[leg].append(ms)
            pt.synchronize()
            same = bool((out_a.cpu().numpy().view(np.uint32) == out_b.cpu().numpy().view(np.uint32)).all())
            if not same:
                raise SystemExit(f"{name} lights, S = {strata}, centred = {centred}: PTDirectLightCulled differs from PTDirectLight")
            med = {k: float(np.median(x)) for k, x in res.items()}
            spread = {k: round(max(x) - min(x), 4) for k, x in res.items()}
            gout = out_a.cpu().numpy()
            cfg["modes"][f"S{strata}{'c' if centred else 'j'}"] = {
                "strata": strata, "centred": centred, "pairs_per_entry": pt.direct_pair_count(strata), "legs_ms_per_call": res, "median_ms_per_call": med,
                "spread_ms": spread, "culled_minus_unculled_ms": round(med["culled"] - med["unculled"], 4), "unculled_over_culled": round(med["unculled"] / med["culled"], 3),
                "beyond_the_spreads": bool(abs(med["culled"] - med["unculled"]) > spread["culled"] + spread["unculled"]), "bit_equal": same,
                "lit": round(float((gout[hit, 0:3] > 0).any(axis=1).mean()), 4), "finite": bool(np.isfinite(gout).all())}
        result["configs"][name] = cfg
        pt.close()
    j, c = result["configs"]["1024"]["modes"]["S1j"]["median_ms_per_call"], result["configs"]["1024"]["modes"]["S1c"]["median_ms_per_call"]
    result["jittered_minus_centred_at_1024_ms"] = {k: round(j[k] - c[k], 4) for k in j}
    result["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
