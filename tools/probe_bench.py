"""SH light probes on the Sponza-class scene: one JSON line.

Probes: first hits of the 1920x1080 camera rays (trace_rays(surface=True)), lifted 0.25 off the surface along the normal turned
towards the camera.  Legs, alternating in one process, `--legs` times each; every leg is `--steps` calls enqueued back to back after
`--warmup` (wall clock, as bench.py's headline; Mrays/s = rays traced / elapsed from PTStats at level 0):
  probe_long     PTProbeSH, 4,096 probes x 4,096 samples, delta lights on;
  gather_long    PTGatherIrradiance of the same counts at the surface points: the same number of paths through the same trace,
                 shade and cleanup kernels, its own first and last kernel;
  probe_short    PTProbeSH, 32,768 probes x 256 samples;
  composed       the workaround the call replaces, once: sphere directions made with numpy on the host, 32 bytes per sample
                 uploaded, PTTraceRadiance over 32,768 x 256 rays, the projection in numpy (no delta lights: no ray hits one);
  evaluate       PTProbeIrradiance over 2^21 queries into the 32,768 probes.
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
LONG = (4096, 4096)
SHORT = (32768, 256)
QUERIES = 1 << 21
Y = (0.28209479, 0.48860251, 1.09254843, 0.31539157, 0.54627422)


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


def host_project(d, c):
    """the projection a host would write: float32 numpy, one sum per coefficient"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    basis = np.stack([np.full_like(x, Y[0]), Y[1] * y, Y[1] * z, Y[1] * x, Y[2] * x * y, Y[2] * y * z, Y[3] * (3 * z * z - 1), Y[2] * x * z,
                      Y[4] * (x * x - y * y)], axis=-1).astype(np.float32)
    return np.einsum("nsk,nsc->nkc", basis, c) * np.float32(4.0 * np.pi / d.shape[1])


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--probe-only", action="store_true", help="profiling runs: only the legs that launch the probe kernels")
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=8)
    lib = pt.lib
    dev = f"cuda:{pt.device}"
    p = pt.params(seed=0x12345678)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)

    rays = pt.camera_rays(pixels=torch.arange(W * H, dtype=torch.int32, device=dev), params=p)
    q = rays.clone()
    q[:, 6], q[:, 7] = 1.0e5, 0.0
    hits, surf = pt.trace_rays(q, surface=True)
    ok = hits[:, 3].contiguous().view(torch.int32) != -1
    pos, nrm = surf[ok, 0:3].contiguous(), surf[ok, 4:7].contiguous()
    back = (nrm * rays[ok, 3:6]).sum(dim=1) > 0
    nrm[back] = -nrm[back]
    n = pos.shape[0]

    def pick(count):
        idx = torch.linspace(0, n - 1, count, device=dev).long()
        return pos[idx].contiguous(), nrm[idx].contiguous()

    long_pos, long_nrm = pick(LONG[0])
    short_pos, short_nrm = pick(SHORT[0])
    long_probes = pt._probes((long_pos + 0.25 * long_nrm).contiguous(), None)
    short_probes = pt._probes((short_pos + 0.25 * short_nrm).contiguous(), None)
    long_recv = pt._receivers(long_pos, long_nrm, None)
    long_out = torch.empty((LONG[0], 28), dtype=torch.float32, device=dev)
    short_out = torch.empty((SHORT[0], 28), dtype=torch.float32, device=dev)
    gather_out = torch.empty((LONG[0], 4), dtype=torch.float32, device=dev)
    p_one = pt._radiance_params(p, spp=1)
    gen = torch.Generator(device=dev).manual_seed(5)
    qn = torch.randn((QUERIES, 3), device=dev, generator=gen)
    queries = torch.empty((QUERIES, 4), dtype=torch.float32, device=dev)
    queries[:, :3] = qn / qn.norm(dim=1, keepdim=True)
    queries.view(torch.int32)[:, 3] = torch.randint(0, SHORT[0], (QUERIES,), device=dev, generator=gen, dtype=torch.int32)
    eval_out = torch.empty((QUERIES, 4), dtype=torch.float32, device=dev)
    h_pos = short_probes[:, :3].cpu().numpy()
    host_rng = np.random.default_rng(1)
    d_rays = torch.zeros((SHORT[0] * SHORT[1], 8), dtype=torch.float32, device=dev)
    d_rad = torch.empty((SHORT[0] * SHORT[1], 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def probe_long():
        plugin.check(lib.PTProbeSH(pt.ctx, C.byref(p), long_probes.data_ptr(), LONG[0], 0, LONG[1], abi.PT_PROBE_DELTA_LIGHTS, long_out.data_ptr()))

    def probe_short():
        plugin.check(lib.PTProbeSH(pt.ctx, C.byref(p), short_probes.data_ptr(), SHORT[0], 0, SHORT[1], abi.PT_PROBE_DELTA_LIGHTS, short_out.data_ptr()))

    def gather_long():
        plugin.check(lib.PTGatherIrradiance(pt.ctx, C.byref(p), long_recv.data_ptr(), LONG[0], 0, LONG[1], gather_out.data_ptr()))

    def evaluate():
        plugin.check(lib.PTProbeIrradiance(pt.ctx, short_out.data_ptr(), SHORT[0], queries.data_ptr(), QUERIES, eval_out.data_ptr()))

    def composed():
        cnt, spp = SHORT
        z = (1.0 - 2.0 * host_rng.random((cnt, spp), dtype=np.float32)).astype(np.float32)
        rho, phi = np.sqrt(np.maximum(0.0, 1.0 - z * z)), np.float32(2.0 * np.pi) * host_rng.random((cnt, spp), dtype=np.float32)
        d = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=-1).astype(np.float32)
        h = np.zeros((cnt * spp, 8), np.float32)
        h[:, 0:3] = np.repeat(h_pos, spp, axis=0)
        h[:, 3:6] = d.reshape(-1, 3)
        h[:, 6] = host_rng.integers(0, 2 ** 32, cnt * spp, dtype=np.uint32).view(np.float32)
        d_rays.copy_(torch.from_numpy(h))
        torch.cuda.synchronize()
        plugin.check(lib.PTTraceRadiance(pt.ctx, C.byref(p_one), d_rays.data_ptr(), cnt * spp, d_rad.data_ptr()))
        pt.synchronize()
        return host_project(d, d_rad[:, :3].cpu().numpy().reshape(cnt, spp, 3))

    # priming as bench.py: every state set in use allocated and touched
    for _ in range(max(12, pt.passes_in_flight())):
        pt.render_pass_to(p, frame.data_ptr(), 0)
    pt.synchronize()

    # (leg, calls timed, warm-up calls): the composed leg is seconds of numpy -- one timed call in all, no warm-up
    legs = {"probe_long": (probe_long, args.steps, args.warmup), "gather_long": (gather_long, args.steps, args.warmup),
            "probe_short": (probe_short, args.steps, args.warmup), "evaluate": (evaluate, args.steps, args.warmup)}
    if args.probe_only:
        legs = {k: v for k, v in legs.items() if k != "gather_long"}
    res = {k: {"mrays": [], "ms_per_call": [], "paths_per_call": 0} for k in legs}
    for _ in range(args.legs):
        for name, (fn, steps, warmup) in legs.items():
            mrays, ms, paths = timed(pt, fn, steps, warmup)
            print(f"[probe_bench] {name}: {ms} ms per call, {mrays} Mrays/s", file=sys.stderr, flush=True)
            res[name]["mrays"].append(mrays)
            res[name]["ms_per_call"].append(ms)
            res[name]["paths_per_call"] = paths
    composed_ms = None
    if not args.probe_only:
        t0 = time.perf_counter()
        sh_host = composed()
        composed_ms = round((time.perf_counter() - t0) * 1e3, 1)
        print(f"[probe_bench] composed: {composed_ms} ms", file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    sh = short_out.cpu().numpy()
    result = {"image": f"{W}x{H}", "long_list": list(LONG), "short_list": list(SHORT), "queries": QUERIES, "lights": int(s.lights.shape[0]),
              "max_bounces": pt.maxRayBounces, "steps": args.steps, "warmup": args.warmup, "schedule": pt.schedule(),
              "passes_in_flight": pt.passes_in_flight(), "mean_band0": [float(v) for v in sh[:, 0:3].mean(axis=0)],
              "finite": bool(np.isfinite(sh).all() and np.isfinite(eval_out.cpu().numpy()).all()), "legs": res,
              "median_ms_per_call": {k: float(np.median(v["ms_per_call"])) for k, v in res.items()}, "composed_ms_once": composed_ms,
              "device": torch.cuda.get_device_name(0)}
    if composed_ms is not None:
        result["composed_mean_band0"] = [float(v) for v in sh_host[:, 0, :].mean(axis=0)]
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
