"""Lightmap UVs on the Sponza-class scene: one JSON line.

Legs, alternating in one process, `--legs` times each; every leg is `--steps` calls after `--warmup`, wall clock around a final
synchronise, for both corner sources (the caller's vertex array, and NULL: the triangle records):
  charts_*     PTUnwrapCharts into preallocated arrays (corners, three sorts, ids, the edge sort, the sweeps with their read-backs,
               the count's read-back, the records);
  emit_*       PTEmitChartUVs;
  unwrap_*     PathTracer.unwrap_lightmap at 2048^2 with the density fitted on the host: both calls, the packer and its bisection.
The host twins are timed once per source and must return the same bytes.  No ratio is asserted.

--ab: the comparison the unwrap exists for, as markdown on stdout.  Equal atlas (1024^2), equal samples (16 and 64), with and
without the lightmap denoiser: bake with tools/lightmap_bench.py's grid atlas and with the fitted unwrap, bind each bake to the whole
scene, read PTLightmapLookup at the first hits of the 1920 x 1080 frame, and report the relative mean square error against
PTGatherIrradiance at those same hits with 1,024 samples, the covered texels and the world area per texel."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402
from lightmap_bench import grid_atlas, timed  # noqa: E402

FIT, AB = 2048, 1024


def area_per_texel(vertices, uvs, size):
    """(5th, 50th, 95th percentile of the world area one texel stands for, over the atlas's texels; texels the UV triangles span)"""
    v = vertices.reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    world = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    u = uvs.reshape(-1, 3, 2).astype(np.float64) * size
    tex = 0.5 * np.abs((u[:, 1, 0] - u[:, 0, 0]) * (u[:, 2, 1] - u[:, 0, 1]) - (u[:, 1, 1] - u[:, 0, 1]) * (u[:, 2, 0] - u[:, 0, 0]))
    ok = np.isfinite(tex) & (tex > 0) & (world > 0)
    ratio, weight = world[ok] / tex[ok], tex[ok]
    order = np.argsort(ratio)
    cum = np.cumsum(weight[order]) / weight.sum()
    pick = lambda q: float(ratio[order][min(np.searchsorted(cum, q), len(order) - 1)])
    return [pick(0.05), pick(0.5), pick(0.95)], float(weight.sum())


def compare(args):
    import torch
    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=1920, height=1080, samplesPerPass=1)
    dev = torch.device(f"cuda:{pt.device}")
    T = len(s.tri_attrs)
    d_verts = torch.from_numpy(s.vertices).to(dev)
    cam = pt.camera_rays()
    rays = np.zeros((cam.shape[0], 8), np.float32)
    rays[:, 0:6], rays[:, 6] = cam[:, 0:6], 1e30
    d_rays = torch.from_numpy(rays).to(dev)
    hits, surf = pt.trace_rays(d_rays, surface=True)
    hit = hits.view(torch.int32)[:, 3] != -1
    recv = torch.zeros((int(hit.sum()), 8), dtype=torch.float32, device=dev)
    recv[:, 0:3], recv[:, 4:7] = surf[hit][:, 0:3], surf[hit][:, 4:7]
    recv.view(torch.int32)[:, 3] = torch.arange(recv.shape[0], dtype=torch.int32, device=dev)
    t0 = time.perf_counter()
    ref = pt.irradiance(receivers=recv, spp=args.ref_samples)[:, 0:3]
    pt.synchronize()
    ref_s = time.perf_counter() - t0
    g_uvs, side = grid_atlas(T)
    u = pt.unwrap_lightmap(AB, AB, vertices=d_verts)
    atlases = {"grid": torch.from_numpy(g_uvs).to(dev), "unwrap": u.uvs}
    print(f"# Grid atlas against the fitted unwrap, Sponza-class ({T} triangles), {AB} x {AB}\n")
    print(f"{torch.cuda.get_device_name(0)}; first hits of the 1920 x 1080 frame: {recv.shape[0]} of {rays.shape[0]} pixels; reference PTGatherIrradiance with "
          f"{args.ref_samples} samples ({ref_s:.1f} s); relative MSE = sum |lightmap - reference|^2 / sum |reference|^2 over the hits that found a texel\n")
    print(f"unwrap: {len(u.charts)} charts, {u.texels_per_unit:.4f} texels per unit, {u.rows_used} rows, stats {u.stats}; grid: {side} x {side} cells\n")
    print("| atlas | covered texels | world area per texel: 5 % | 50 % | 95 % |\n|---|---|---|---|---|")
    for name, uvs in atlases.items():
        pct, _ = area_per_texel(s.vertices, uvs.cpu().numpy(), AB)
        texels, _ = pt.chart_receivers(AB, AB, uvs=uvs)
        print(f"| {name} | {texels.shape[0]} | {pct[0]:.4e} | {pct[1]:.4e} | {pct[2]:.4e} |")
    print("\n| samples | denoise | atlas | hits that found a texel | relative MSE | bake ms |\n|---|---|---|---|---|---|")
    power = float((ref.double() ** 2).sum())
    for spp in (16, 64):
        for denoise in (None, 5):
            for name, uvs in atlases.items():
                pt.synchronize()
                t0 = time.perf_counter()
                image = pt.bake_lightmap(AB, AB, spp=spp, uvs=uvs, dilate=2, denoise=denoise, as_tensor=True)
                pt.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                pt.bind_lightmaps([pt.lightmap_binding(image, uvs=uvs, two_sided=True)])
                got, which = pt.lightmap_lookup(d_rays, hits, surf)
                found = (which[hit] == 0)
                err = float(((got[hit][:, 0:3].double() - ref.double())[found] ** 2).sum())
                base = float((ref.double()[found] ** 2).sum())
                print(f"| {spp} | {'yes' if denoise else 'no'} | {name} | {int(found.sum())} | {err / base:.5f} | {ms:.1f} |", flush=True)
    pt.bind_lightmaps([])
    print(f"\n(sum |reference|^2 over all hits: {power:.4e})")
    pt.close()


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--no-host", action="store_true", help="profiling runs: leave the host twins out")
    ap.add_argument("--ab", action="store_true", help="the grid atlas against the unwrap, as markdown")
    ap.add_argument("--ref-samples", type=int, default=1024)
    args = ap.parse_args()
    if args.ab:
        return compare(args)

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=256, height=256, samplesPerPass=1)
    lib = pt.lib
    dev = torch.device(f"cuda:{pt.device}")
    T = len(s.tri_attrs)
    d_verts = torch.from_numpy(s.vertices).to(dev)
    d = abi.unwrap_desc(T, pt._blas_offsets(None))
    cap = 1 << 16
    of = torch.empty((T,), dtype=torch.int32, device=dev)
    charts = torch.empty((cap, 8), dtype=torch.float32, device=dev)
    uvs = torch.empty((T, 6), dtype=torch.float32, device=dev)
    n, st = C.c_uint32(), abi.PTUnwrapStats()
    _, h_tris, _ = pt.read_geometry()
    sources = {"vertices": (d_verts, None, s.vertices), "records": (None, h_tris, None)}
    info, host_ms, host_equal, state = {}, {}, {}, {}

    def run_charts(v):
        plugin.check(lib.PTUnwrapCharts(pt.ctx, C.byref(d), None if v is None else v.data_ptr(), of.data_ptr(), charts.data_ptr(), cap, C.byref(n), C.byref(st)))

    for name, (v, tris, verts) in sources.items():
        run_charts(v)
        pt.synchronize()
        h_charts = charts[:n.value].cpu().numpy().view(abi.UNWRAP_CHART_DTYPE).reshape(-1).copy()
        tpu, _ = plugin.fit_chart_density(h_charts, FIT, FIT, 2)
        origins, rows = plugin.pack_charts(h_charts, FIT, FIT, tpu, 2)
        d_origins = torch.from_numpy(origins).to(dev)
        state[name] = (of.clone(), charts[:n.value].clone(), d_origins, tpu)
        info[name] = {"charts": n.value, "stats": st.as_dict(), "fitted_texels_per_unit": round(tpu, 4), "rows_used": rows}
        if not args.no_host:
            t0 = time.perf_counter()
            w_of, w_charts = plugin.unwrap_charts(tris, verts)
            t1 = time.perf_counter()
            w_uvs = plugin.emit_chart_uvs(tris, w_of, w_charts, origins, FIT, FIT, tpu, 2, vertices=verts)
            t2 = time.perf_counter()
            plugin.check(lib.PTEmitChartUVs(pt.ctx, C.byref(d), None if v is None else v.data_ptr(), of.data_ptr(), charts.data_ptr(), d_origins.data_ptr(), n.value,
                                            FIT, FIT, 2, tpu, uvs.data_ptr()))
            pt.synchronize()
            host_ms[name] = {"charts": round((t1 - t0) * 1e3, 1), "emit": round((t2 - t1) * 1e3, 1)}       # the charts twin runs twice: the count, then the records
            host_equal[name] = bool(np.array_equal(w_of, of.cpu().numpy().view(np.uint32)) and w_charts.tobytes() == h_charts.tobytes() and
                                    np.array_equal(w_uvs.view(np.uint32), uvs.cpu().numpy().view(np.uint32)))
        print(f"[unwrap_bench] {name}: {info[name]}, host {host_ms.get(name)}, equal {host_equal.get(name)}", file=sys.stderr, flush=True)

    def run_emit(name):
        v = sources[name][0]
        s_of, s_charts, s_origins, tpu = state[name]
        plugin.check(lib.PTEmitChartUVs(pt.ctx, C.byref(d), None if v is None else v.data_ptr(), s_of.data_ptr(), s_charts.data_ptr(), s_origins.data_ptr(),
                                        s_charts.shape[0], FIT, FIT, 2, tpu, uvs.data_ptr()))

    legs = {"charts_vertices": lambda: run_charts(d_verts), "charts_records": lambda: run_charts(None),
            "emit_vertices": lambda: run_emit("vertices"), "emit_records": lambda: run_emit("records"),
            "unwrap_vertices": lambda: pt.unwrap_lightmap(FIT, FIT, vertices=d_verts), "unwrap_records": lambda: pt.unwrap_lightmap(FIT, FIT)}
    res = {k: [] for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            ms = timed((pt,), fn, args.steps, args.warmup)
            print(f"[unwrap_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
    result = {"triangles": T, "atlas": FIT, "sources": info, "host_twin_ms": host_ms, "host_twin_equal": host_equal, "steps": args.steps, "warmup": args.warmup,
              "legs_ms_per_call": res, "median_ms_per_call": {k: float(np.median(v)) for k, v in res.items()},
              "work_bytes_per_triangle": 148, "device": torch.cuda.get_device_name(0)}
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
