"""First hits shaded from a baked lightmap on the Sponza-class scene: one JSON line.

The 1920x1080 first hits, the 16 x 8 x 16 probe volume with a placement, the 64 reflection probes and the DFG table are
tools/shade_baked_bench.py's; the lightmap is 2048 x 2048 over the grid atlas tools/lightmap_bench.py builds, baked here.  Legs,
alternating in one process, `--legs` times each; every leg is `--steps` calls enqueued back to back after `--warmup` (wall clock,
as bench.py's headline); what a leg binds is bound before its warm-up:
  a_lightmapped_all    PTShadeLightmapped with the whole scene bound: every hit reads four texels, no lane asks the volume;
  b_baked              PTShadeBaked, the existing kernel: the baseline;
  c_lightmapped_mixed  PTShadeLightmapped with every second span of 4,096 primitives bound: waves with lanes of both kinds;
  d_lightmapped_none   PTShadeLightmapped with nothing bound: what the walk costs when there is nothing to find;
  e_lookup             PTLightmapLookup alone, the whole scene bound;
  f_frame_lightmapped  PTShadeLightmappedFrame, the whole scene bound;
  f_frame_baked        PTShadeBakedFrame.
The fused result with the whole scene bound is compared with the six-step composition bit for bit.  No ratio is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402
from lightmap_bench import grid_atlas  # noqa: E402
from shade_baked_bench import GRID, H, LEVELS, PROBES, RES, W, timed  # noqa: E402

ATLAS, SPP, SPAN = 2048, 4, 4096


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

    T = s.vertices.shape[0] // 3
    uvs, side = grid_atlas(T)
    d_uvs = torch.from_numpy(uvs).to(dev)
    image = pt.bake_lightmap(ATLAS, ATLAS, spp=SPP, uvs=d_uvs, dilate=2, params=p, as_tensor=True)
    whole = [pt.lightmap_binding(image, uvs=d_uvs, two_sided=True)]
    mixed = []
    for first in range(0, T, 2 * SPAN):
        if len(mixed) == abi.PT_LIGHTMAP_MAX_BINDINGS:
            break
        e = pt.lightmap_binding(image, uvs=d_uvs, two_sided=True)
        e["record"].firstPrim, e["record"].primCount = first, min(SPAN, T - first)
        e["record"].dUvs = d_uvs.data_ptr() + first * 24
        mixed.append(e)

    n = W * H
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    plugin.check(lib.PTShadeBakedFrame(pt.ctx, C.byref(p), C.byref(inputs), out.data_ptr(), rays.data_ptr()))
    pt.synchronize()
    hits, surf = pt.trace_rays(rays, surface=True)
    irr, which = torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def lightmapped():
        plugin.check(lib.PTShadeLightmapped(pt.ctx, C.byref(inputs), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr()))

    def baked():
        plugin.check(lib.PTShadeBaked(pt.ctx, C.byref(inputs), rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, out.data_ptr()))

    def lookup():
        plugin.check(lib.PTLightmapLookup(pt.ctx, rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, irr.data_ptr(), which.data_ptr()))

    def frame_lightmapped():
        plugin.check(lib.PTShadeLightmappedFrame(pt.ctx, C.byref(p), C.byref(inputs), out.data_ptr(), None))

    def frame_baked():
        plugin.check(lib.PTShadeBakedFrame(pt.ctx, C.byref(p), C.byref(inputs), out.data_ptr(), None))

    legs = {"a_lightmapped_all": (whole, lightmapped), "b_baked": ([], baked), "c_lightmapped_mixed": (mixed, lightmapped), "d_lightmapped_none": ([], lightmapped),
            "e_lookup": (whole, lookup), "f_frame_lightmapped": (whole, frame_lightmapped), "f_frame_baked": ([], frame_baked)}
    res = {k: [] for k in legs}
    found = {}
    for _ in range(args.legs):
        for name, (table, fn) in legs.items():
            pt.bind_lightmaps(table)
            ms = timed(pt, fn, args.steps, args.warmup)
            print(f"[lightmap_shade_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
            if name not in found:
                found[name] = int((pt.lightmap_lookup(rays, hits, surf)[1] != -1).sum())
    med = {k: float(np.median(x)) for k, x in res.items()}
    spread = {k: round(max(x) - min(x), 4) for k, x in res.items()}

    # the composition equality on this data, the whole scene bound
    pt.bind_lightmaps(whole)
    got = pt.shade_lightmapped(rays, hits, surf, volume, refl, dfg)
    _, terms, recv, qr = pt.shade_surfaces(rays, hits, surf, refl.probe_rows, refl.box_rows)
    E = volume.irradiance(receivers=recv)
    L, k = pt.lightmap_lookup(rays, hits, surf)
    E = torch.where((k != -1)[:, None], L, E)
    want = pt.shade_compose(terms, E, _reflection(pt, refl, qr), dfg)
    same = bool((got.cpu().numpy().view(np.uint32) == want.cpu().numpy().view(np.uint32)).all())
    pt.bind_lightmaps([])
    none_same = bool((pt.shade_lightmapped(rays, hits, surf, volume, refl, dfg).cpu().numpy().view(np.uint32) ==
                      pt.shade_baked(rays, hits, surf, volume, refl, dfg).cpu().numpy().view(np.uint32)).all())
    prim = hits.cpu().numpy().view(np.uint32)[:, 3]
    g = got.cpu().numpy()
    result = {"image": f"{W}x{H}", "entries": n, "first_hits": int((prim != 0xFFFFFFFF).sum()), "triangles": T, "atlas": ATLAS, "atlas_cells": [side, side],
              "lightmap_samples": SPP, "bindings": {"all": len(whole), "mixed": len(mixed), "span": SPAN}, "entries_that_found_a_lightmap": found,
              "grid": list(GRID), "probes": PROBES, "res": RES, "levels": LEVELS, "steps": args.steps, "warmup": args.warmup,
              "legs_ms_per_call": res, "median_ms_per_call": med, "spread_ms": spread,
              "a_over_b": round(med["a_lightmapped_all"] / med["b_baked"], 3), "d_minus_b_ms": round(med["d_lightmapped_none"] - med["b_baked"], 4),
              "a_faster_than_b_by_more_than_bs_spread": bool(med["b_baked"] - med["a_lightmapped_all"] > spread["b_baked"]),
              "d_exceeds_b_by_more_than_bs_spread": bool(med["d_lightmapped_none"] - med["b_baked"] > spread["b_baked"]),
              "frame_lightmapped_minus_baked_ms": round(med["f_frame_lightmapped"] - med["f_frame_baked"], 4),
              "lightmapped_equals_composition": same, "nothing_bound_equals_baked": none_same,
              "mean_rgb": [float(x) for x in g[:, :3].mean(axis=0)], "finite": bool(np.isfinite(g).all()), "device": torch.cuda.get_device_name(0)}
    del keep
    pt.close()
    print(json.dumps(result))


def _reflection(pt, refl, qr):
    """PTReflectionLookup of the queries PTShadeSurfaces wrote"""
    import torch
    spec = torch.empty((qr.shape[0], 4), dtype=torch.float32, device=qr.device)
    with pt._ordered(qr.device):
        plugin.check(pt.lib.PTReflectionLookup(pt.ctx, refl.maps.data_ptr(), refl.maps.shape[0], refl.res, refl.levels, refl.probe_rows.data_ptr(),
                                               refl.box_rows.data_ptr(), qr.data_ptr(), qr.shape[0], spec.data_ptr()))
    return spec


if __name__ == "__main__":
    main()
