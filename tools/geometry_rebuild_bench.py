"""In-place geometry rebuilds on the Sponza-class scene (250k triangles): one JSON line.

rebuild: medians over `--rebuilds` back-to-back calls, in device events on the context's stream (which waits for the update),
  as tools/geometry_update_bench.py times the refit.  device_ms: PTRebuildGeometryDevice; host_ms: PTRebuildGeometry (the copy
  into pinned staging and the upload included); refit_device_ms: PTUpdateGeometryDevice of the same vertices;
  build_set_scene_ms: what a rebuild cost before -- PTBuildBVHDevice (upload, kernels, read-back of nodes and rows) followed by
  PTSetScene of the whole scene, host wall time with the context drained before and after, in this process; its two parts are
  given too.  levels / nodes / capacity: the rebuilt tree.
quality: at deformations of 1 %, 5 % and 20 % of the scene's extent, sahCost (PTMeasureGeometry) of the tree refitted from the
  rest pose and of the tree rebuilt in place, beside each tree's node visits per ray and Mrays/s at 1920x1080, 8 spp per pass.
every_pass: Mrays/s with 3 passes in flight and a rebuild before every pass, against the static rate and a refit before every pass."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")       # as bench.py

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geometry_update_bench import deformed, events, throughput  # noqa: E402
from unity_webgpu_pathtracer_amd import plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402


def rebuild_costs(pt, scene, reps):
    import torch
    dev = f"cuda:{pt.device}"
    s = torch.cuda.ExternalStream(pt.stream(), device=dev)
    W = [deformed(scene.vertices, 0.01, ph) for ph in (0.0, 1.0)]
    D = [torch.from_numpy(w).to(dev) for w in W]
    torch.cuda.synchronize()
    n = scene.tri_count
    lib = pt.lib
    for k in range(4):                                   # warm-up: allocations, the plan, the code objects
        plugin.check(lib.PTRebuildGeometry(pt.ctx, 0, 0, 0, W[k & 1].ctypes.data, n, None))
        plugin.check(lib.PTRebuildGeometryDevice(pt.ctx, 0, 0, 0, D[k & 1].data_ptr(), n, None))
        plugin.check(lib.PTUpdateGeometryDevice(pt.ctx, 0, 0, 0, D[k & 1].data_ptr(), n, None))
    pt.synchronize()
    k = [0]

    def call(fn, arrays, ptr):
        def run():
            k[0] += 1
            plugin.check(fn(pt.ctx, 0, 0, 0, ptr(arrays[k[0] & 1]), n, None))
        return run

    out = {"triangles": n,
           "device_ms": round(events(s, call(lib.PTRebuildGeometryDevice, D, lambda a: a.data_ptr()), reps), 4),
           "host_ms": round(events(s, call(lib.PTRebuildGeometry, W, lambda a: a.ctypes.data), reps), 4),
           "refit_device_ms": round(events(s, call(lib.PTUpdateGeometryDevice, D, lambda a: a.data_ptr()), reps), 4)}
    plugin.check(lib.PTRebuildGeometryDevice(pt.ctx, 0, 0, 0, D[0].data_ptr(), n, None))
    q = pt.geometry_quality()
    out.update({"nodes": q["nodeCount"], "capacity": q["nodeCapacity"], "levels": q["levels"]})
    # the path a rebuild took before: build on the device, read back, set the whole scene
    bvh = pt._bvhScene
    keep = (bvh.bvh_nodes, bvh.bvh_tris)
    total, build, setscene, kernels = [], [], [], []
    for r in range(5):
        pt.synchronize()
        timing = {}
        t0 = time.perf_counter()
        bvh.bvh_nodes, bvh.bvh_tris = plugin.build_cwbvh(W[r & 1], device=pt.device, timing=timing)
        t1 = time.perf_counter()
        bvh.PrepareShader(pt.ctx)
        pt.synchronize()
        t2 = time.perf_counter()
        total.append((t2 - t0) * 1e3), build.append((t1 - t0) * 1e3), setscene.append((t2 - t1) * 1e3), kernels.append(timing["build_ms"])
    out.update({"build_set_scene_ms": round(float(np.median(total)), 3), "build_and_read_back_ms": round(float(np.median(build)), 3),
                "build_kernels_ms": round(float(np.median(kernels)), 3), "set_scene_ms": round(float(np.median(setscene)), 3)})
    bvh.bvh_nodes, bvh.bvh_tris = keep
    bvh.PrepareShader(pt.ctx)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rebuilds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--node-capacity", type=float, default=1.5, help="factor on the built tree's node count: the span the rebuilds must fit")
    args = ap.parse_args()
    W, H, SPP = args.width, args.height, 8
    scene = scenes.sponza_atrium(tex_size=args.tex_size, detail=args.detail)
    pt = PathTracer(scene, width=W, height=H, samplesPerPass=SPP, build_device=0, node_capacity=args.node_capacity)
    pt.set_stats_level(1)
    n = scene.tri_count
    out = {"metric": "geometry rebuild costs", "rebuild": rebuild_costs(pt, scene, args.rebuilds)}
    # tree quality: refitted from the rest pose against rebuilt in place
    out["quality"] = {}
    built = pt.geometry_quality()
    out["built_sah_cost"] = round(built["sahCost"], 3)
    for amp in (0.01, 0.05, 0.20):
        w = deformed(scene.vertices, amp)
        pt._bvhScene.PrepareShader(pt.ctx)               # the rest pose's tree again
        plugin.check(pt.lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, w.ctypes.data, n, None))
        refit = pt.geometry_quality()
        r_rate, r_visits = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
        plugin.check(pt.lib.PTRebuildGeometry(pt.ctx, 0, 0, 0, w.ctypes.data, n, None))
        rebuilt = pt.geometry_quality()
        b_rate, b_visits = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
        out["quality"][f"{amp:.2f}"] = {"refit_sah_cost": round(refit["sahCost"], 3), "rebuild_sah_cost": round(rebuilt["sahCost"], 3),
                                         "refit_over_built": round(refit["sahCost"] / built["sahCost"], 4),
                                         "refit_node_visits_per_ray": round(r_visits, 2), "rebuild_node_visits_per_ray": round(b_visits, 2),
                                         "refit_mrays_per_s": round(r_rate, 1), "rebuild_mrays_per_s": round(b_rate, 1),
                                         "rebuild_nodes": rebuilt["nodeCount"]}
    # a rebuild before every pass, 3 passes in flight
    pt._bvhScene.PrepareShader(pt.ctx)
    pt.set_passes_in_flight(3)
    frames = [deformed(scene.vertices, 0.01, ph) for ph in np.linspace(0.0, 1.0, 4)]
    static, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
    refit, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup,
                          lambda k: plugin.check(pt.lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, frames[k % 4].ctypes.data, n, None)))
    rebuild, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup,
                            lambda k: plugin.check(pt.lib.PTRebuildGeometry(pt.ctx, 0, 0, 0, frames[k % 4].ctypes.data, n, None)))
    pt._bvhScene.PrepareShader(pt.ctx)
    static2, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
    s = max(static, static2)
    out["every_pass"] = {"static_mrays_per_s": round(s, 1), "refit_every_pass_mrays_per_s": round(refit, 1),
                         "rebuild_every_pass_mrays_per_s": round(rebuild, 1), "refit_cost_pct": round((1.0 - refit / s) * 100.0, 2),
                         "rebuild_cost_pct": round((1.0 - rebuild / s) * 100.0, 2), "passes_in_flight": 3}
    pt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
