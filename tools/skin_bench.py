"""Skinned geometry on the Sponza-class scene (250k triangles): one JSON line.

The skin is procedural: 64 joints spread along the scene's long axis, every vertex weighted to the four joints nearest to it along
that axis with smooth (hat-function) weights; a pose bends the joints by a few degrees.  All times are medians of `--updates`
calls in device events on the context's stream (which waits for the update), as tools/geometry_update_bench.py times, all in this
one process:
  skin_refit_ms / skin_rebuild_ms      PTSkinGeometry (host palette, no bounds read-back), refit and PT_SKIN_REBUILD
  skin_refit_attrs_ms                  the same refit with rest attributes (the attribute kernel and the attribute carry-over copy)
  device_refit_ms / device_rebuild_ms  PTUpdateGeometryDevice / PTRebuildGeometryDevice of vertices already on the device
  host_update_ms                       PTUpdateGeometry of host-skinned vertices; host_skinning_ms: the host twin's time to make them
                                       (PTSkinVerticesHost, one thread); host_path_ms: their sum, what a host-skinned frame costs
  skin_kernels_ms                      skin_refit_ms - device_refit_ms: the palette upload, pt_skin_vertices and the fold, by difference
  floor_ms                             the bytes pt_skin_vertices must move (56 B per vertex) at the bandwidth a device copy reaches
every_pass: Mrays/s at 1920x1080, 8 spp per pass, 3 passes in flight: a skin before every pass, a host update (host skinning
  included) before every pass, and static."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")       # as bench.py

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geometry_update_bench import events, throughput  # noqa: E402
from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

JOINTS = 64


def procedural_skin(vertices):
    """-> (joints (n, 4) uint16, weights (n, 4) float32, axis, joint positions along it)"""
    p = vertices[:, :3].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    axis = int(np.argmax(hi - lo))
    u = (p[:, axis] - lo[axis]) / (hi[axis] - lo[axis]) * (JOINTS - 1)          # in joint spacings
    first = np.clip(np.floor(u).astype(np.int64) - 1, 0, JOINTS - 4)
    joints = first[:, None] + np.arange(4)[None, :]
    w = np.maximum(0.0, 2.0 - np.abs(u[:, None] - joints)) ** 2                  # smooth, four influences
    w /= w.sum(axis=1, keepdims=True)
    return joints.astype(np.uint16), w.astype(np.float32), axis, np.linspace(lo[axis], hi[axis], JOINTS)


def pose(axis, centres, phase, degrees=3.0):
    """(J, 12) float32: joint j turns about an axis through its centre by a smooth angle"""
    out = np.zeros((JOINTS, 3, 4))
    a, b = (axis + 1) % 3, (axis + 2) % 3
    for j, c in enumerate(centres):
        t = np.radians(degrees) * np.sin(0.35 * j + phase)
        r = np.eye(3)
        r[axis, axis], r[axis, a], r[a, axis], r[a, a] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
        pivot = np.zeros(3)
        pivot[axis] = c
        out[j, :, :3] = r
        out[j, :, 3] = pivot - r @ pivot + 0.02 * np.sin(0.2 * j + phase) * np.eye(3)[b]
    return out.reshape(JOINTS, 12).astype(np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=20)
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
    lib, n = pt.lib, scene.tri_count
    rest = np.ascontiguousarray(scene.vertices, np.float32)
    joints, weights, axis, centres = procedural_skin(rest)
    poses = [pose(axis, centres, ph) for ph in np.linspace(0.0, 1.5, 4)]
    dev = f"cuda:{pt.device}"
    s = torch.cuda.ExternalStream(pt.stream(), device=dev)
    t0 = time.perf_counter()
    skinned = [plugin.skin_vertices(rest, joints, weights, m)[0] for m in poses[:2]]
    host_skinning_ms = (time.perf_counter() - t0) * 1e3 / 2
    D = [torch.from_numpy(v).to(dev) for v in skinned]
    torch.cuda.synchronize()
    k = [0]

    def skin(flags):
        def run():
            k[0] += 1
            plugin.check(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, poses[k[0] & 1].ctypes.data, JOINTS, flags, None))
        return run

    def arrays(fn, ptrs):
        def run():
            k[0] += 1
            plugin.check(fn(pt.ctx, 0, 0, 0, ptrs[k[0] & 1], n, None))
        return run

    calls = {"skin_refit_ms": skin(0), "skin_rebuild_ms": skin(abi.PT_SKIN_REBUILD),
             "device_refit_ms": arrays(lib.PTUpdateGeometryDevice, [d.data_ptr() for d in D]),
             "device_rebuild_ms": arrays(lib.PTRebuildGeometryDevice, [d.data_ptr() for d in D]),
             "host_update_ms": arrays(lib.PTUpdateGeometry, [v.ctypes.data for v in skinned])}
    pt.set_skin(rest, joints, weights, joint_count=JOINTS)
    for fn in calls.values():                               # warm-up: allocations, the plan, the code objects
        fn(), fn()
    pt.synchronize()
    out = {"triangles": n, "joints": JOINTS, "host_skinning_ms": round(host_skinning_ms, 3)}
    for name, fn in calls.items():
        out[name] = round(events(s, fn, args.updates), 4)
    out["skin_kernels_ms"] = round(out["skin_refit_ms"] - out["device_refit_ms"], 4)
    out["host_path_ms"] = round(out["host_update_ms"] + host_skinning_ms, 3)
    # a refit after the rebuilds above leaves every variant the same tree to refit; the attributes last (they stay on)
    pt.set_skin(rest, joints, weights, rest_attrs=scene.tri_attrs, joint_count=JOINTS)
    fn = skin(0)
    fn(), fn()
    pt.synchronize()
    out["skin_refit_attrs_ms"] = round(events(s, fn, args.updates), 4)
    size = n * 3 * 56
    src, dst = torch.empty(size // 2, dtype=torch.uint8, device=dev), torch.empty(size // 2, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(s):
        dst.copy_(src)
        copy_ms = events(s, lambda: dst.copy_(src), args.updates)
    out.update({"skin_vertex_bytes": size, "skin_attr_bytes": n * 256, "copy_gb_per_s": round(size / (copy_ms * 1e-3) / 1e9, 1), "floor_ms": round(copy_ms, 4)})
    result = {"metric": "skinned geometry costs", "skin": out}
    # a skin before every pass against a host update before every pass against static, 3 passes in flight
    pt.set_skin(rest, joints, weights, joint_count=JOINTS)
    pt.set_passes_in_flight(3)
    static, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
    skin_rate, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup,
                              lambda i: plugin.check(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, poses[i % 4].ctypes.data, JOINTS, 0, None)))

    def host_pass(i):
        v = plugin.skin_vertices(rest, joints, weights, poses[i % 4])[0]
        plugin.check(lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, v.ctypes.data, n, None))

    host_rate, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup, host_pass)
    plugin.check(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (JOINTS, 1)).ctypes.data, JOINTS, 0, None))
    static2, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
    st = max(static, static2)
    result["every_pass"] = {"static_mrays_per_s": round(st, 1), "skin_every_pass_mrays_per_s": round(skin_rate, 1),
                            "host_update_every_pass_mrays_per_s": round(host_rate, 1), "skin_cost_pct": round((1.0 - skin_rate / st) * 100.0, 2),
                            "host_update_cost_pct": round((1.0 - host_rate / st) * 100.0, 2), "passes_in_flight": 3}
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
