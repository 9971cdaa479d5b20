"""Irradiance gathers on the Sponza-class scene: one JSON line.

Receivers: the first hits of the 1920x1080 camera rays (trace_rays(surface=True)), normals turned towards the camera.  Legs,
alternating in one process, `--legs` times each; every leg is `--steps` calls enqueued back to back after `--warmup` (wall clock,
as bench.py's headline; Mrays/s = rays traced / elapsed from PTStats at level 0):
  gather        PTGatherIrradiance, 8 samples per receiver: directions made and receivers lit on the GPU;
  render        PTRenderPassTo over the same frame with SamplesPerPass = 8: the same number of paths;
  composed      the workaround the gather replaces: cosine-weighted directions made with numpy on the host, 32 bytes per sample
                uploaded, PTTraceRadiance over receivers x 8 rays, the mean taken by the caller (no light at the receiver);
  short_gather  4,096 receivers x 4,096 samples in one call: every sample a slot of its own.  (The same probes as a ray list with
                one slot each and the samples one after another are 4,095 x 6 dependent trace + shade rounds per call: minutes, not
                timed here.)
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

from unity_webgpu_pathtracer_amd import plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H, SPP = 1920, 1080, 8
SHORT = 4096


def timed(pt, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    pt.synchronize()
    pt.reset_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    pt.synchronize()
    elapsed = time.perf_counter() - t0
    st = pt.stats()
    return round(st.rays / elapsed / 1e6, 1), round(elapsed / steps * 1e3, 3), int(st.paths // steps)


def host_directions(nrm, spp, rng):
    """cosine-weighted directions about each normal, numpy on the host: (n * spp, 3) float32"""
    n = nrm.shape[0]
    r1, r2 = rng.random((n, spp), dtype=np.float32), rng.random((n, spp), dtype=np.float32)
    r, phi = np.sqrt(r1), np.float32(2.0 * np.pi) * r2
    x, y = r * np.cos(phi), r * np.sin(phi)
    z = np.sqrt(np.maximum(0.0, 1.0 - r1)).astype(np.float32)
    a = np.where(np.abs(nrm[:, :1]) > 0.9, np.float32([0, 1, 0]), np.float32([1, 0, 0]))
    t = np.cross(nrm, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    d = x[..., None] * t[:, None, :] + y[..., None] * b[:, None, :] + z[..., None] * nrm[:, None, :]
    return d.reshape(n * spp, 3).astype(np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--gather-only", action="store_true", help="profiling runs: only the legs that launch the gather kernels, and the render")
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=SPP)
    lib = pt.lib
    dev = f"cuda:{pt.device}"
    p = pt.params(seed=0x12345678)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)

    # receivers: first hits of the camera rays
    rays = pt.camera_rays(pixels=torch.arange(W * H, dtype=torch.int32, device=dev), params=p)
    q = rays.clone()
    q[:, 6], q[:, 7] = 1.0e5, 0.0
    hits, surf = pt.trace_rays(q, surface=True)
    ok = hits[:, 3].contiguous().view(torch.int32) != -1
    pos, nrm = surf[ok, 0:3].contiguous(), surf[ok, 4:7].contiguous()
    back = (nrm * rays[ok, 3:6]).sum(dim=1) > 0
    nrm[back] = -nrm[back]
    n = pos.shape[0]
    recv = pt._receivers(pos, nrm, None)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    short_recv = recv[torch.linspace(0, n - 1, SHORT, device=dev).long()].contiguous()
    short_out = torch.empty((SHORT, 4), dtype=torch.float32, device=dev)
    p_one = pt._radiance_params(p, spp=1)
    h_pos, h_nrm = pos.cpu().numpy(), nrm.cpu().numpy()
    host_rng = np.random.default_rng(1)
    d_rays = torch.zeros((n * SPP, 8), dtype=torch.float32, device=dev)
    d_rad = torch.empty((n * SPP, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    print(f"[gather_bench] {n} receivers", file=sys.stderr, flush=True)

    def gather():
        plugin.check(lib.PTGatherIrradiance(pt.ctx, C.byref(p), recv.data_ptr(), n, 0, SPP, out.data_ptr()))

    def short_gather():
        plugin.check(lib.PTGatherIrradiance(pt.ctx, C.byref(p), short_recv.data_ptr(), SHORT, 0, SHORT, short_out.data_ptr()))

    def composed():
        d = host_directions(h_nrm, SPP, host_rng)
        h = np.zeros((n * SPP, 8), np.float32)
        h[:, 0:3] = np.repeat(h_pos, SPP, axis=0) + d * np.float32(1.0e-4)
        h[:, 3:6] = d
        h[:, 6] = host_rng.integers(0, 2 ** 32, n * SPP, dtype=np.uint32).view(np.float32)
        d_rays.copy_(torch.from_numpy(h))
        torch.cuda.synchronize()
        plugin.check(lib.PTTraceRadiance(pt.ctx, C.byref(p_one), d_rays.data_ptr(), n * SPP, d_rad.data_ptr()))
        pt.synchronize()
        return d_rad[:, :3].reshape(n, SPP, 3).mean(dim=1) * np.pi

    # priming as bench.py: every state set in use allocated and touched
    for _ in range(max(12, pt.passes_in_flight())):
        pt.render_pass_to(p, frame.data_ptr(), 0)
    pt.synchronize()

    # (leg, calls timed, warm-up calls): a call of the composed leg is several seconds of numpy -- one timed call, no warm-up
    legs = {"gather": (gather, args.steps, args.warmup), "render": (lambda: pt.render_pass_to(p, frame.data_ptr(), 0), args.steps, args.warmup),
            "composed": (composed, 1, 0), "short_gather": (short_gather, args.steps, args.warmup)}
    if args.gather_only:
        legs = {k: v for k, v in legs.items() if k in ("gather", "render", "short_gather")}
    res = {k: {"mrays": [], "ms_per_call": [], "paths_per_call": 0} for k in legs}
    for _ in range(args.legs):
        for name, (fn, steps, warmup) in legs.items():
            mrays, ms, paths = timed(pt, fn, steps, warmup)
            print(f"[gather_bench] {name}: {ms} ms per call, {mrays} Mrays/s", file=sys.stderr, flush=True)
            res[name]["mrays"].append(mrays)
            res[name]["ms_per_call"].append(ms)
            res[name]["paths_per_call"] = paths
    torch.cuda.synchronize()
    e = out.cpu().numpy()
    result = {"image": f"{W}x{H}", "receivers": n, "samples": SPP, "short_list": [SHORT, SHORT], "max_bounces": pt.maxRayBounces,
              "steps": args.steps, "warmup": args.warmup, "schedule": pt.schedule(), "passes_in_flight": pt.passes_in_flight(),
              "mean_irradiance": [float(v) for v in e[:, :3].mean(axis=0)], "finite": bool(np.isfinite(e).all()), "legs": res,
              "median_ms_per_call": {k: float(np.median(v["ms_per_call"])) for k, v in res.items()},
              "device": torch.cuda.get_device_name(0)}
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
