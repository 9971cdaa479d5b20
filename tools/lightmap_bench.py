"""Lightmap bakes on the Sponza-class scene: one JSON line.

The atlas is synthetic and built here: one grid cell per pair of triangles, each cell padded by a tenth of its edge, so that at
1024^2 and 2048^2 almost every triangle is smaller than an 8x8 tile -- the first extreme of the rasteriser's workload.  The other
extreme, two triangles over the whole atlas, is the `quad` leg.  Legs, alternating in one process, `--legs` times each; every leg
is `--steps` calls after `--warmup`, wall clock around a final synchronise:
  raster_1024, raster_2048   PTRasterizeChart into preallocated arrays (coverage, compaction, the count's read-back, emit);
  quad_2048                  the same for a floor quad: 2 triangles, 4 M texels;
  resolve_d0, resolve_d4     PTResolveLightmap of the 1024^2 list with dilate 0 and 4;
  gather                     PTGatherIrradiance alone, 64 samples, over the 1024^2 chart's receivers;
  bake                       bake_lightmap at 1024^2, 64 samples, dilate 2: rasterise + the same gather + resolve;
  bake_after_update          PTUpdateGeometryDevice with displaced vertices, then the same bake, every call.
The host twin (PTRasterizeChartHost on the arrays PTReadGeometry returns) is timed once per atlas size and must return the same
list.  No ratio is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

SPP, BAKE = 64, 1024


def grid_atlas(triangles, pad=0.1):
    """(T, 6) float32: triangle 2k and 2k + 1 share cell k of a square grid, as the two halves of its padded square"""
    cells = (triangles + 1) // 2
    side = int(np.ceil(np.sqrt(cells)))
    k = np.arange(triangles) // 2
    x0, y0 = (k % side + pad) / side, (k // side + pad) / side
    x1, y1 = (k % side + 1 - pad) / side, (k // side + 1 - pad) / side
    lower = np.stack([x0, y0, x1, y0, x1, y1], axis=1)
    upper = np.stack([x0, y0, x1, y1, x0, y1], axis=1)
    return np.where((np.arange(triangles) % 2 == 0)[:, None], lower, upper).astype(np.float32), side


def quad_scene():
    sb = scenes.SoupBuilder()
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0), 1, 1, 0)
    verts, attrs = sb.finish()
    mats = np.stack([scenes.pack_material(color=(0.8, 0.8, 0.8, 1.0), roughness=1.0)])
    return scenes.Scene("floor_quad", verts, attrs, mats, np.zeros((0, 16), np.float32), np.zeros(0, np.uint32),
                        scenes.Camera(eye=(0.0, 3.0, -4.0), target=(0.0, 0.0, 0.0)), environment_mode=1)


def timed(tracers, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    for t in tracers:
        t.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    for t in tracers:
        t.synchronize()
    return round((time.perf_counter() - t0) / steps * 1e3, 3)


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--no-host", action="store_true", help="profiling runs: leave the host twin out")
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=256, height=256, samplesPerPass=1)
    quad = PathTracer(quad_scene(), width=64, height=64, samplesPerPass=1)
    lib = pt.lib
    dev = torch.device(f"cuda:{pt.device}")
    T = len(s.tri_attrs)
    uvs, side = grid_atlas(T)
    d_uvs = torch.from_numpy(uvs).to(dev)
    p = pt.params(seed=0x12345678)
    count = C.c_uint64()
    cap = 2048 * 2048
    texels = torch.empty((cap,), dtype=torch.int32, device=dev)
    recv = torch.empty((cap, 8), dtype=torch.float32, device=dev)
    verts = torch.from_numpy(s.vertices).to(dev)
    moved = [verts + 0.002 * torch.randn_like(verts) * torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    print(f"[lightmap_bench] {T} triangles, {side} x {side} cells", file=sys.stderr, flush=True)

    def raster(tracer, size, u):
        d = tracer._chart_desc(size, size, None, None, 0)
        plugin.check(lib.PTRasterizeChart(tracer.ctx, C.byref(d), None if u is None else u.data_ptr(), texels.data_ptr(), recv.data_ptr(), cap, C.byref(count)))
        return count.value

    # the list the resolve and the gather legs run over, and the host twin beside the device at both sizes
    covered, host_ms, host_equal = {}, {}, {}
    _, h_tris, h_attrs = pt.read_geometry()
    for size in (1024, 2048):
        covered[size] = raster(pt, size, d_uvs)
        if not args.no_host:
            t0 = time.perf_counter()
            ht, hr = plugin.rasterize_chart(h_tris, h_attrs, size, size, uvs=uvs)
            host_ms[size] = round((time.perf_counter() - t0) * 1e3, 1)            # two passes of the twin: the count, then the lists
            pt.synchronize()
            n = covered[size]
            host_equal[size] = bool(len(ht) == n and np.array_equal(ht.view(np.int32), texels[:n].cpu().numpy()) and
                                    np.array_equal(hr.view(np.uint32), recv[:n].cpu().numpy().view(np.uint32)))
            print(f"[lightmap_bench] host twin {size}: {host_ms[size]} ms, equal: {host_equal[size]}", file=sys.stderr, flush=True)
    n = raster(pt, BAKE, d_uvs)
    pt.synchronize()
    b_texels, b_recv = texels[:n].clone(), recv[:n].clone()
    irr = torch.empty((n, 4), dtype=torch.float32, device=dev)
    image = torch.empty((BAKE, BAKE, 4), dtype=torch.float32, device=dev)
    flip = [0]

    def gather():
        plugin.check(lib.PTGatherIrradiance(pt.ctx, C.byref(p), b_recv.data_ptr(), n, 0, SPP, irr.data_ptr()))

    def resolve(dilate):
        plugin.check(lib.PTResolveLightmap(pt.ctx, b_texels.data_ptr(), irr.data_ptr(), n, BAKE, BAKE, dilate, image.data_ptr()))

    def bake():
        return pt.bake_lightmap(BAKE, BAKE, spp=SPP, uvs=d_uvs, dilate=2, params=p, as_tensor=True)

    def bake_after_update():
        flip[0] ^= 1
        pt.update_geometry(moved[flip[0]])
        return bake()

    gather()
    pt.synchronize()
    legs = {"raster_1024": lambda: raster(pt, 1024, d_uvs), "raster_2048": lambda: raster(pt, 2048, d_uvs), "quad_2048": lambda: raster(quad, 2048, None),
            "resolve_d0": lambda: resolve(0), "resolve_d4": lambda: resolve(4), "gather": gather, "bake": bake, "bake_after_update": bake_after_update}
    res = {k: [] for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            ms = timed((pt, quad), fn, args.steps, args.warmup)
            print(f"[lightmap_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
    quad.synchronize()
    med = {k: float(np.median(v)) for k, v in res.items()}
    img = bake().cpu().numpy()
    result = {"triangles": T, "cells": [side, side], "covered": covered, "bake": {"atlas": BAKE, "samples": SPP, "dilate": 2, "receivers": n},
              "max_bounces": pt.maxRayBounces, "steps": args.steps, "warmup": args.warmup, "schedule": pt.schedule(),
              "host_twin_ms": host_ms, "host_twin_equal": host_equal, "legs_ms_per_call": res, "median_ms_per_call": med,
              "added_share_of_bake": round((med["bake"] - med["gather"]) / med["bake"], 4),
              "raster_plus_resolve_over_bake": round((med["raster_1024"] + med["resolve_d0"]) / med["bake"], 4),
              "baked_texels": int((img[..., 3] == 1).sum()), "dilated_texels": int((img[..., 3] == 0.5).sum()), "finite": bool(np.isfinite(img).all()),
              "device": torch.cuda.get_device_name(0)}
    pt.close()
    quad.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
