"""Scene updates: one JSON line.

update_ms[n]: one PTUpdateInstances at n instances (201, 4,096, 65,536), timed with device events on the context's stream
  around `--updates` back-to-back updates (the host copy into the staging buffer included), against the two ways the same
  change is made without it: CPU BuildTLAS of the same records (build_tlas_ms) and PTSetScene of the whole scene
  (set_scene_ms).
instanced: Mrays/s of bench.py's `instanced` workload (200 instances, 1920x1080, 8 spp per pass, passes in flight, the
  accumulated frame ping-ponged as bench.py does) with the Bounce.cs motion applied through PTUpdateInstances before every
  pass, against the same passes on the static scene."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")       # as bench.py: the default number of passes in flight follows it

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402


def blas_records(bvh, scene, transforms):
    """BLASInstance records of `transforms`, computed as BVHScene.UpdateTLAS computes them."""
    rec = bvh.blas_instances.copy()
    for k, m in enumerate(transforms):
        t0, n = scene.mesh_ranges[scene.instances[k][0]]
        lo, hi = scenes.instance_world_bounds(scene.vertices[t0 * 3:(t0 + n) * 3], m)
        rec[k]["localToWorld"] = m.T.reshape(16).astype(np.float32)
        rec[k]["worldToLocal"] = np.linalg.inv(m).T.reshape(16).astype(np.float32)
        rec[k]["aabbMin"], rec[k]["aabbMax"] = lo, hi
    return rec


def update_costs(n, updates):
    import torch
    scene = scenes.instanced_scene(count=n - 1, detail=4)
    pt = PathTracer(scene, width=8, height=8)
    recs = [blas_records(pt._bvhScene, scene, scenes.bounce_transforms(scene, t)) for t in (0.3, 0.6)]
    s = torch.cuda.ExternalStream(pt.stream(), device="cuda:0")
    for k in range(4):
        plugin.check(pt.lib.PTUpdateInstances(pt.ctx, recs[k & 1].ctypes.data, n))
    pt.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for k in range(updates):
            plugin.check(pt.lib.PTUpdateInstances(pt.ctx, recs[k & 1].ctypes.data, n))
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b) / updates)
    cpu = []
    for _ in range(5):
        t0 = time.perf_counter()
        plugin.build_tlas(recs[0])
        cpu.append((time.perf_counter() - t0) * 1e3)
    ss = []
    for _ in range(3):
        t0 = time.perf_counter()
        pt._bvhScene.PrepareShader(pt.ctx)
        ss.append((time.perf_counter() - t0) * 1e3)
    pt.close()
    return {"update_ms": round(float(np.median(ms)), 4), "build_tlas_ms": round(float(np.median(cpu)), 4),
            "set_scene_ms": round(float(np.median(ss)), 3)}


def instanced_throughput(steps, warmup):
    import torch
    W, H, SPP = 1920, 1080, 8
    scene = scenes.make_scene("instanced", count=200, detail=48)
    pt = PathTracer(scene, width=W, height=H, samplesPerPass=SPP)
    frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    recs = [blas_records(pt._bvhScene, scene, scenes.bounce_transforms(scene, k / 60.0)) for k in range(steps + warmup)]
    n = recs[0].shape[0]
    torch.cuda.synchronize()

    def run(dynamic):
        cur = 0
        for k in range(warmup + steps):
            if k == warmup:
                pt.synchronize()
                torch.cuda.synchronize()
                pt.reset_stats()
                t0 = time.perf_counter()
            if dynamic:
                plugin.check(pt.lib.PTUpdateInstances(pt.ctx, recs[k].ctypes.data, n))
            p = scenes.frame_params(scene, W, H, spp=SPP, current_sample=k * SPP, seed=0x1234 + k)
            pt.render_pass_to(p, frames[cur].data_ptr(), frames[1 - cur].data_ptr() if k > 0 else 0)
            cur = 1 - cur
        pt.synchronize()
        dt = time.perf_counter() - t0
        return pt.stats().rays / dt / 1e6

    static = run(False)
    dynamic = run(True)
    static2 = run(False)
    inflight = pt.passes_in_flight()
    pt.close()
    s = max(static, static2)
    return {"static_mrays_per_s": round(s, 1), "update_every_pass_mrays_per_s": round(dynamic, 1),
            "cost_pct": round((1.0 - dynamic / s) * 100.0, 2), "passes_in_flight": inflight}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--sizes", default="201,4096,65536")
    args = ap.parse_args()
    out = {"metric": "scene update costs", "instances": {}}
    for n in [int(x) for x in args.sizes.split(",") if x]:
        out["instances"][str(n)] = update_costs(n, args.updates if n < 10000 else max(5, args.updates // 10))
    out["instanced"] = instanced_throughput(args.steps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
