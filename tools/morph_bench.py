"""Morph targets on the Sponza-class scene (250k triangles): one JSON line.

Two procedural morphs.  "dense": 8 targets, every corner lists every target (a dense glTF target), smooth displacement fields of a
few millimetres.  "sparse": 64 targets, each listing the corners of one slab across the scene's long axis, about 2 % of them (what a
sparse accessor of a local shape holds); the slabs of neighbouring targets overlap.  The skin is tools/skin_bench.py's (64 joints).
All times are medians of `--updates` calls in device events on the context's stream (which waits for the update), as
tools/skin_bench.py times, all in this one process.  Per case:
  listed_entries / stored_entries / padding_ratio   the position stream as CSR and as laid out on the device (stored / listed)
  morph_refit_ms / morph_rebuild_ms    PTMorphGeometry (host weights, no palette, no bounds read-back), refit and PT_SKIN_REBUILD
  morph_skin_refit_ms                  the same refit with a palette: morph, then skin, in one kernel
  morph_refit_attrs_ms                 the refit with rest attributes and a normal stream of the same sparsity (the attribute kernel
                                       and the attribute carry-over copy)
  device_refit_ms                      PTUpdateGeometryDevice of vertices already on the device
  morph_kernels_ms                     morph_refit_ms - device_refit_ms: the weight upload, pt_morph_vertices and the fold, by difference
  host_morphing_ms                     the host twin's time to make the vertices (PTMorphVerticesHost, one thread);
  host_update_ms / host_path_ms        PTUpdateGeometry of host-morphed vertices; their sum, what a host-morphed frame costs
  vertex_bytes / floor_ms              what pt_morph_vertices must move (rest 16 + output 16 + count 4 per corner, 16 per stored entry)
                                       and a device-to-device copy of that many bytes in this process
every_pass (per case): Mrays/s at 1920x1080, 8 spp per pass, 3 passes in flight: a morph before every pass, a host update (host
  morphing included) before every pass, and static."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")       # as bench.py

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geometry_update_bench import events, throughput  # noqa: E402
from skin_bench import JOINTS, pose, procedural_skin  # noqa: E402
from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402


def dense_morph(vertices, targets, seed):
    """CSR stream in which every corner lists every target: smooth fields, amplitude 5 mm"""
    p = vertices[:, :3].astype(np.float64)
    rng = np.random.RandomState(seed)
    n = len(p)
    ent = np.zeros((n, targets), abi.MORPH_ENTRY)
    for k in range(targets):
        f, ph = rng.uniform(0.3, 1.5, 3), rng.uniform(0, 6.28, 3)
        for a, name in enumerate(("dx", "dy", "dz")):
            ent[name][:, k] = 0.005 * np.sin(p[:, (a + 1) % 3] * f[a] + ph[a])
        ent["target"][:, k] = k
    return np.arange(n + 1, dtype=np.uint32) * np.uint32(targets), ent.reshape(-1)


def sparse_morph(vertices, targets, coverage, seed):
    """CSR stream: target k lists the corners whose position along the long axis lies in its slab (`coverage` of the corners each)"""
    p = vertices[:, :3].astype(np.float64)
    rng = np.random.RandomState(seed)
    n = len(p)
    axis = int(np.argmax(p.max(axis=0) - p.min(axis=0)))
    rank = np.argsort(np.argsort(p[:, axis], kind="stable"), kind="stable")          # each corner's place along the axis
    width = int(n * coverage)
    corners, ks = [], []
    for k in range(targets):
        first = int((n - width) * k / max(targets - 1, 1) * 0.5)                    # slabs over half the scene: neighbours overlap
        c = np.nonzero((rank >= first) & (rank < first + width))[0]
        corners.append(c)
        ks.append(np.full(len(c), k))
    corner, target = np.concatenate(corners), np.concatenate(ks)
    order = np.lexsort((target, corner))
    corner, target = corner[order], target[order]
    ent = np.zeros(len(corner), abi.MORPH_ENTRY)
    for name in ("dx", "dy", "dz"):
        ent[name] = rng.uniform(-0.005, 0.005, len(corner))
    ent["target"] = target
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(corner, minlength=n))
    return off, ent


def other_deltas(stream, seed, scale):
    """The same sparsity with other deltas (a normal stream)"""
    ent = stream[1].copy()
    rng = np.random.RandomState(seed)
    for name in ("dx", "dy", "dz"):
        ent[name] = rng.uniform(-scale, scale, len(ent))
    return stream[0], ent


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
    ap.add_argument("--cases", default="dense,sparse")
    args = ap.parse_args()
    W, H, SPP = args.width, args.height, 8
    scene = scenes.sponza_atrium(tex_size=args.tex_size, detail=args.detail)
    pt = PathTracer(scene, width=W, height=H, samplesPerPass=SPP, build_device=0, node_capacity=args.node_capacity)
    pt.set_stats_level(1)
    lib, n = pt.lib, scene.tri_count
    rest = np.ascontiguousarray(scene.vertices, np.float32)
    joints, sweights, axis, centres = procedural_skin(rest)
    poses = [pose(axis, centres, ph) for ph in (0.0, 1.5)]
    dev = f"cuda:{pt.device}"
    s = torch.cuda.ExternalStream(pt.stream(), device=dev)
    pt.set_skin(rest, joints, sweights, joint_count=JOINTS)
    result = {"metric": "morph target costs", "triangles": n, "joints": JOINTS}
    k = [0]
    for case in args.cases.split(","):
        targets = 8 if case == "dense" else 64
        position = dense_morph(rest, targets, 1) if case == "dense" else sparse_morph(rest, targets, 0.02, 1)
        normal = other_deltas(position, 2, 0.05)
        rng = np.random.RandomState(3)
        ws = [rng.uniform(0, 1, targets).astype(np.float32) for _ in range(4)]
        listed = len(position[1])
        stored = int(lib.PTMorphLayoutHost(position[0].ctypes.data, position[1].ctypes.data, n * 3, None, None, None))
        out = {"targets": targets, "listed_entries": listed, "stored_entries": stored, "padding_ratio": round(stored / max(listed, 1), 3)}
        t0 = time.perf_counter()
        morphed = [plugin.morph_vertices(rest, position, w)[0] for w in ws[:2]]
        out["host_morphing_ms"] = round((time.perf_counter() - t0) * 1e3 / 2, 3)
        D = [torch.from_numpy(v).to(dev) for v in morphed]
        torch.cuda.synchronize()

        def morph(flags, palette):
            def run():
                k[0] += 1
                m = poses[k[0] & 1] if palette else None
                plugin.check(lib.PTMorphGeometry(pt.ctx, 0, 0, 0, ws[k[0] & 1].ctypes.data, targets, None if m is None else m.ctypes.data,
                                                 JOINTS if palette else 0, flags, None))
            return run

        def arrays(fn, ptrs):
            def run():
                k[0] += 1
                plugin.check(fn(pt.ctx, 0, 0, 0, ptrs[k[0] & 1], n, None))
            return run

        calls = {"morph_refit_ms": morph(0, False), "morph_skin_refit_ms": morph(0, True), "morph_rebuild_ms": morph(abi.PT_SKIN_REBUILD, False),
                 "device_refit_ms": arrays(lib.PTUpdateGeometryDevice, [d.data_ptr() for d in D]),
                 "host_update_ms": arrays(lib.PTUpdateGeometry, [v.ctypes.data for v in morphed])}
        pt.set_morph(rest, position, target_count=targets)
        for fn in calls.values():                               # warm-up: allocations, the plan, the code objects
            fn(), fn()
        pt.synchronize()
        for name, fn in calls.items():
            out[name] = round(events(s, fn, args.updates), 4)
        out["morph_kernels_ms"] = round(out["morph_refit_ms"] - out["device_refit_ms"], 4)
        out["host_path_ms"] = round(out["host_update_ms"] + out["host_morphing_ms"], 3)
        # a refit after the rebuilds above leaves every variant the same tree to refit; the attributes last (they stay on)
        pt.set_morph(rest, position, normal, rest_attrs=scene.tri_attrs, target_count=targets)
        fn = morph(0, False)
        fn(), fn()
        pt.synchronize()
        out["morph_refit_attrs_ms"] = round(events(s, fn, args.updates), 4)
        size = n * 3 * 36 + stored * 16
        src, dst = torch.empty(size // 2, dtype=torch.uint8, device=dev), torch.empty(size // 2, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(s):
            dst.copy_(src)
            copy_ms = events(s, lambda: dst.copy_(src), args.updates)
        del src, dst
        out.update({"vertex_bytes": size, "copy_gb_per_s": round(size / (copy_ms * 1e-3) / 1e9, 1), "floor_ms": round(copy_ms, 4)})
        result[case] = out
        # a morph before every pass against a host update before every pass against static, 3 passes in flight
        pt.set_morph(rest, position, target_count=targets)
        pt.set_passes_in_flight(3)
        static, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
        rate, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup,
                             lambda i: plugin.check(lib.PTMorphGeometry(pt.ctx, 0, 0, 0, ws[i % 4].ctypes.data, targets, None, 0, 0, None)))

        def host_pass(i):
            v = plugin.morph_vertices(rest, position, ws[i % 4])[0]
            plugin.check(lib.PTUpdateGeometry(pt.ctx, 0, 0, 0, v.ctypes.data, n, None))

        host_rate, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup, host_pass)
        zero = np.zeros(targets, np.float32)
        plugin.check(lib.PTMorphGeometry(pt.ctx, 0, 0, 0, zero.ctypes.data, targets, None, 0, 0, None))
        static2, _ = throughput(pt, scene, W, H, SPP, args.steps, args.warmup)
        st = max(static, static2)
        out["every_pass"] = {"static_mrays_per_s": round(st, 1), "morph_every_pass_mrays_per_s": round(rate, 1),
                             "host_update_every_pass_mrays_per_s": round(host_rate, 1), "morph_cost_pct": round((1.0 - rate / st) * 100.0, 2),
                             "host_update_cost_pct": round((1.0 - host_rate / st) * 100.0, 2), "passes_in_flight": 3}
        pt.set_passes_in_flight(0)
        del D
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
