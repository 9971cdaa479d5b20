"""Geometry updates on the Sponza-class scene (250k triangles): one JSON line.

update: one PTUpdateGeometry of the whole mesh in device events on the context's stream (which waits for the update),
  median over `--updates` back-to-back updates.  host_ms: host arrays (the copy into pinned staging and the upload
  included); device_ms: PTUpdateGeometryDevice (no staging); staging_ms: their difference; carry_over_copy_ms: a
  device-to-device copy of the carried-over bytes (nodes + triangles) timed alone, with the bandwidth it reaches;
  floor_ms: the bytes the kernels must move (triangle kernel: 16 + 48 B read, 48 B written per triangle; level kernels:
  80 B read, 64 + 24 B written per node) at that bandwidth.  The kernels' own times come from a kernel trace
  (profiles/geometry_kernel_stats.csv, profiles/geometry_update_launches.csv), taken in a run of its own.
against: the same vertices through CPU BuildBVH, PTBuildBVHDevice (kernels only) and PTSetScene of the whole scene.
every_pass: Mrays/s at 1920x1080, 8 spp per pass, 3 passes in flight with an update before every pass, against the static rate.
quality: Mrays/s and node visits per ray over the tree refitted to a deformation of 1 %, 5 % and 20 % of the scene's extent,
  against a fresh BuildBVH of the same vertices."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")       # as bench.py

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402


def deformed(v, amplitude, phase=0.0):
    """A smooth field of `amplitude` x the scene's extent"""
    p = v[:, :3].astype(np.float64)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    k = np.array([[2.1, 0.7, 1.3], [0.9, 2.6, 0.5], [1.7, 1.1, 2.3]]) * (2 * np.pi / ext)
    out = v.copy()
    out[:, :3] = (p + np.sin(p @ k + phase) * amplitude * ext).astype(np.float32)
    return out


def events(stream, fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def update_costs(pt, scene, updates):
    import torch
    dev = f"cuda:{pt.device}"
    s = torch.cuda.ExternalStream(pt.stream(), device=dev)
    W = [deformed(scene.vertices, 0.01, ph) for ph in (0.0, 1.0)]
    D = [torch.from_numpy(w).to(dev) for w in W]
    n = scene.tri_count
    lib = pt.lib
    for k in range(4):                                   # warm-up: allocations, the plan, the code objects
        plugin.check(lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, W[k & 1].ctypes.data, n, None))
        plugin.check(lib.PTUpdateGeometryDevice(pt.ctx, 0, 0, 0, D[k & 1].data_ptr(), n, None))
    pt.synchronize()
    k = [0]

    def host():
        k[0] += 1
        plugin.check(lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, W[k[0] & 1].ctypes.data, n, None))

    def device():
        k[0] += 1
        plugin.check(lib.PTUpdateGeometryDevice(pt.ctx, 0, 0, 0, D[k[0] & 1].data_ptr(), n, None))

    host_ms, device_ms = events(s, host, updates), events(s, device, updates)
    bvh = pt._bvhScene
    carry = bvh.bvh_nodes.nbytes + bvh.bvh_tris.nbytes
    src, dst = torch.empty(carry, dtype=torch.uint8, device=dev), torch.empty(carry, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(s):
        dst.copy_(src)
        copy_ms = events(s, lambda: dst.copy_(src), updates)
    bw = 2 * carry / (copy_ms * 1e-3)                   # read + written
    nodes = bvh.bvh_nodes.nbytes // 80
    tri_bytes, node_bytes = n * (16 + 48 + 48), nodes * (80 + 64 + 24)
    out = {"triangles": n, "nodes": nodes, "host_ms": round(host_ms, 4), "device_ms": round(device_ms, 4),
           "staging_ms": round(host_ms - device_ms, 4), "carry_over_bytes": carry, "carry_over_copy_ms": round(copy_ms, 4),
           "copy_gb_per_s": round(bw / 1e9, 1), "triangle_kernel_bytes": tri_bytes, "level_kernel_bytes": node_bytes,
           "floor_ms": {"triangle_kernel": round(tri_bytes / bw * 1e3, 4), "level_kernels": round(node_bytes / bw * 1e3, 4)}}
    cpu, gpu = {}, {}
    t = []
    for _ in range(3):
        plugin.build_cwbvh(W[0], timing=cpu)
        t.append(cpu["build_ms"])
    out["build_bvh_cpu_ms"] = round(float(np.median(t)), 2)
    plugin.build_cwbvh(W[0], device=pt.device, timing=gpu)
    t = []
    for _ in range(3):
        plugin.build_cwbvh(W[0], device=pt.device, timing=gpu)
        t.append(gpu["build_ms"])
    out["build_bvh_device_ms"] = round(float(np.median(t)), 3)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        bvh.PrepareShader(pt.ctx)
        t.append((time.perf_counter() - t0) * 1e3)
    out["set_scene_ms"] = round(float(np.median(t)), 2)
    return out


def throughput(pt, scene, W, H, SPP, steps, warmup, per_pass=None):
    """Mrays/s and node visits per ray of warmup + steps passes; per_pass(k) runs before pass k"""
    import torch
    frames = [torch.zeros((H, W, 4), dtype=torch.float32, device=f"cuda:{pt.device}") for _ in range(2)]
    torch.cuda.synchronize()
    cur = 0
    for k in range(warmup + steps):
        if k == warmup:
            pt.synchronize()
            torch.cuda.synchronize()
            pt.reset_stats()
            t0 = time.perf_counter()
        if per_pass:
            per_pass(k)
        p = scenes.frame_params(scene, W, H, spp=SPP, current_sample=k * SPP, seed=0x1234 + k)
        pt.render_pass_to(p, frames[cur].data_ptr(), frames[1 - cur].data_ptr() if k > 0 else 0)
        cur = 1 - cur
    pt.synchronize()
    dt = time.perf_counter() - t0
    st = pt.stats()
    return st.rays / dt / 1e6, st.nodeVisits / max(st.rays, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--detail", type=float, default=1.0)
    args = ap.parse_args()
    W, H, SPP = args.width, args.height, 8
    scene = scenes.sponza_atrium(tex_size=args.tex_size, detail=args.detail)
    pt = PathTracer(scene, width=W, height=H, samplesPerPass=SPP)
    pt.set_stats_level(1)
    out = {"metric": "geometry update costs", "update": update_costs(pt, scene, args.updates)}
    # an update before every pass, 3 passes in flight
    pt.set_passes_in_flight(3)
    n = scene.tri_count
    frames = [deformed(scene.vertices, 0.01, ph) for ph in np.linspace(0.0, 1.0, 4)]
    static, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
    dynamic, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup,
                            lambda k: plugin.check(pt.lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, frames[k % 4].ctypes.data, n, None)))
    pt._bvhScene.PrepareShader(pt.ctx)
    static2, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
    s = max(static, static2)
    out["every_pass"] = {"static_mrays_per_s": round(s, 1), "update_every_pass_mrays_per_s": round(dynamic, 1),
                         "cost_pct": round((1.0 - dynamic / s) * 100.0, 2), "passes_in_flight": 3}
    # tree quality after a refit against a rebuild
    out["quality"] = {}
    built = (pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris)
    for amp in (0.01, 0.05, 0.20):
        w = deformed(scene.vertices, amp)
        pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris = built
        pt._bvhScene.PrepareShader(pt.ctx)
        plugin.check(pt.lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, w.ctypes.data, n, None))
        r_rate, r_visits = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
        pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris = plugin.build_cwbvh(w)
        pt._bvhScene.PrepareShader(pt.ctx)
        f_rate, f_visits = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
        out["quality"][f"{amp:.2f}"] = {"refit_mrays_per_s": round(r_rate, 1), "rebuild_mrays_per_s": round(f_rate, 1),
                                         "refit_node_visits_per_ray": round(r_visits, 2), "rebuild_node_visits_per_ray": round(f_visits, 2)}
    pt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
