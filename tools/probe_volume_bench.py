"""Probe volumes on the Sponza-class scene: one JSON line.

Queries: the first hits of the 1920x1080 camera rays (trace_rays(surface=True)), normals turned towards the camera.  The volume: a
16 x 8 x 16 grid over the box those hits span, baked once (64 SH samples, 256 depth samples per probe).  Legs, alternating in one
process, `--legs` times each; every leg is `--steps` calls enqueued back to back after `--warmup` (wall clock):
  depth          PTProbeDepth, 4,096 probes x 256 samples (probes 0.25 above 4,096 of the first hits), maxDistance as the volume's;
  lookup_off     PTProbeGridIrradiance over all first hits, both flags off (trilinear only);
  lookup_on      the same with PT_GRID_WRAP | PT_GRID_VISIBILITY;
  nearest        PTProbeIrradiance over the same points, each with the index of its nearest probe (Part 15's call);
  composed       the host-composed route to the depth records the call replaces, once: PTProbeRays, the rays turned into PTRay rows
                 with numpy, PTTraceRays, the cos^32-weighted sums in numpy.
No ratio is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H = 1920, 1080
DEPTH = (4096, 256)
COUNTS = (16, 8, 16)


def timed(pt, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    pt.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    pt.synchronize()
    return round((time.perf_counter() - t0) / steps * 1e3, 4)


def texel_directions():
    l = np.arange(64)
    a, b = ((l % 8) + 0.5) * 0.25 - 1.0, ((l // 8) + 0.5) * 0.25 - 1.0
    z = 1.0 - np.abs(a) - np.abs(b)
    x = np.where(z < 0, (1.0 - np.abs(b)) * np.sign(a), a)
    y = np.where(z < 0, (1.0 - np.abs(a)) * np.sign(b), b)
    d = np.stack([x, y, z], axis=1)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--volume-only", action="store_true", help="profiling runs: the timed legs without the host-composed route")
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=8)
    lib = pt.lib
    dev = f"cuda:{pt.device}"
    p = pt.params(seed=0x12345678)

    rays = pt.camera_rays(pixels=torch.arange(W * H, dtype=torch.int32, device=dev), params=p)
    q = rays.clone()
    q[:, 6], q[:, 7] = 1.0e5, 0.0
    hits, surf = pt.trace_rays(q, surface=True)
    ok = hits[:, 3].contiguous().view(torch.int32) != -1
    pos, nrm = surf[ok, 0:3].contiguous(), surf[ok, 4:7].contiguous()
    back = (nrm * rays[ok, 3:6]).sum(dim=1) > 0
    nrm[back] = -nrm[back]
    n = pos.shape[0]
    lo, hi = pos.min(dim=0).values.cpu().numpy(), pos.max(dim=0).values.cpu().numpy()

    t0 = time.perf_counter()
    vol = pt.bake_probe_volume(lo, hi, COUNTS, spp=64, depth_spp=256)
    pt.synchronize()
    bake_ms = round((time.perf_counter() - t0) * 1e3, 1)
    probes = vol.sh.shape[0]
    recv = pt._receivers(pos, nrm, None)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    grids = {}
    for name, on in (("lookup_off", False), ("lookup_on", True)):
        g = abi.PTProbeGrid.from_buffer_copy(vol.grid)
        g.flags = (abi.PT_GRID_WRAP | abi.PT_GRID_VISIBILITY) if on else 0
        g.normalBias = vol.default_normal_bias()
        grids[name] = g
    # the nearest probe of every point
    org = torch.tensor([vol.grid.origin[a] for a in range(3)], device=dev)
    spc = torch.tensor([vol.grid.spacing[a] for a in range(3)], device=dev)
    cnt = torch.tensor(COUNTS, device=dev)
    idx = torch.minimum(torch.clamp(torch.round((pos - org) / spc), min=0).long(), cnt - 1)
    near = ((idx[:, 2] * COUNTS[1] + idx[:, 1]) * COUNTS[0] + idx[:, 0]).to(torch.int32)
    queries = torch.empty((n, 4), dtype=torch.float32, device=dev)
    queries[:, :3] = nrm
    queries.view(torch.int32)[:, 3] = near
    near_out = torch.empty((n, 4), dtype=torch.float32, device=dev)

    pick = torch.linspace(0, n - 1, DEPTH[0], device=dev).long()
    d_probes = pt._probes((pos[pick] + 0.25 * nrm[pick]).contiguous(), None)
    d_depth = torch.empty((DEPTH[0], 64, 2), dtype=torch.float32, device=dev)
    max_d = vol.max_distance
    torch.cuda.synchronize()

    def depth():
        plugin.check(lib.PTProbeDepth(pt.ctx, d_probes.data_ptr(), DEPTH[0], 0, DEPTH[1], max_d, d_depth.data_ptr()))

    def lookup(name):
        return lambda: plugin.check(lib.PTProbeGridIrradiance(pt.ctx, C.byref(grids[name]), vol._rows.data_ptr(), vol._depth.data_ptr(), recv.data_ptr(), n,
                                                              out.data_ptr()))

    def nearest():
        plugin.check(lib.PTProbeIrradiance(pt.ctx, vol._rows.data_ptr(), probes, queries.data_ptr(), n, near_out.data_ptr()))

    def composed():
        cnt_, spp = DEPTH
        pr = pt.probe_rays(d_probes[:, :3].contiguous(), spp=spp).cpu().numpy()
        h = np.zeros((cnt_ * spp, 8), np.float32)
        h[:, 0:6], h[:, 6] = pr[:, 0:6], max_d
        t = pt.trace_rays(h)[:, 0].reshape(cnt_, spp)
        w = pr[:, 3:6].reshape(cnt_, spp, 3)
        wt = np.maximum(np.einsum("lk,nsk->nsl", texel_directions(), w), 0.0) ** 32
        sw = wt.sum(axis=1)
        with np.errstate(all="ignore"):
            mean = np.where(sw > 0, np.einsum("nsl,ns->nl", wt, t) / sw, max_d)
            mean2 = np.where(sw > 0, np.einsum("nsl,ns->nl", wt, t * t) / sw, max_d * max_d)
        return np.stack([mean, mean2], axis=2)

    legs = {"depth": depth, "lookup_off": lookup("lookup_off"), "lookup_on": lookup("lookup_on"), "nearest": nearest}
    res = {k: [] for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            ms = timed(pt, fn, args.steps, args.warmup)
            print(f"[probe_volume_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
    composed_ms, composed_diff = None, None
    if not args.volume_only:
        t0 = time.perf_counter()
        host = composed()
        composed_ms = round((time.perf_counter() - t0) * 1e3, 1)
        composed_diff = float(np.abs(host[..., 0] - d_depth.cpu().numpy()[..., 0]).max())
        print(f"[probe_volume_bench] composed: {composed_ms} ms", file=sys.stderr, flush=True)
    # what the weights do on this scene
    lookup("lookup_on")()
    pt.synchronize()
    on = out.cpu().numpy().copy()
    lookup("lookup_off")()
    pt.synchronize()
    off = out.cpu().numpy()
    med = {k: float(np.median(v)) for k, v in res.items()}
    result = {"image": f"{W}x{H}", "queries": n, "grid": list(COUNTS), "probes": probes, "depth_list": list(DEPTH), "max_distance": max_d,
              "bake_ms_once": bake_ms, "steps": args.steps, "warmup": args.warmup, "legs": res, "median_ms_per_call": med,
              "lookup_on_over_nearest": round(med["lookup_on"] / med["nearest"], 2) if "nearest" in med else None,
              "composed_ms_once": composed_ms, "composed_max_abs_diff_mean": composed_diff,
              "mean_support_on": float(on[:, 3].mean()), "queries_without_support_on": int((on[:, 3] == 0).sum()),
              "mean_irradiance_off": [float(v) for v in off[:, :3].mean(axis=0)], "mean_irradiance_on": [float(v) for v in on[:, :3].mean(axis=0)],
              "finite": bool(np.isfinite(on).all() and np.isfinite(off).all() and np.isfinite(d_depth.cpu().numpy()).all()),
              "device": torch.cuda.get_device_name(0)}
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
