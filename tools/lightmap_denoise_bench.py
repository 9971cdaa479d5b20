"""The lightmap denoiser on the Sponza-class charts of tools/lightmap_bench.py: one JSON line.

Legs, alternating in one process, `--legs` times each; every leg is `--steps` calls after `--warmup`, wall clock around a final
synchronise:
  filter_1024, filter_2048   PTDenoiseLightmap at 5 levels over the 1024^2 and the 2048^2 chart's gathered list;
  levels0_1024               the same call with 0 levels: scatter, footprint and collect alone;
  gather64, gather16         PTGatherIrradiance alone over the 1024^2 chart's receivers at 64 and at 16 samples.
Then the claim the filter is for, on the 1024^2 chart against a `--reference`-sample bake of the same receivers (samples the other
bakes do not use): the mean squared error of 16 samples, of 16 samples filtered, and of 64 samples.  The host twin is run once on
the 1024^2 list and must return the device's bytes (`--no-host` leaves it out).  Nothing is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import abi, plugin, scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402
from lightmap_bench import grid_atlas, timed  # noqa: E402

LEVELS = 5


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    ap.add_argument("--reference", type=int, default=4096, help="samples of the reference bake (0: no error figures)")
    ap.add_argument("--no-host", action="store_true", help="profiling runs: leave the host twin out")
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=256, height=256, samplesPerPass=1)
    lib = pt.lib
    dev = torch.device(f"cuda:{pt.device}")
    uvs, side = grid_atlas(len(s.tri_attrs))
    d_uvs = torch.from_numpy(uvs).to(dev)
    p = pt.params(seed=0x12345678)

    lists = {}
    for size in (1024, 2048):
        texels, recv = pt.chart_receivers(size, size, uvs=d_uvs)
        irr = pt.irradiance(receivers=recv, spp=16, params=p)
        lists[size] = (texels, recv, irr, torch.empty_like(irr))
        print(f"[lightmap_denoise_bench] {size}: {texels.shape[0]} receivers", file=sys.stderr, flush=True)
    pt.synchronize()

    def denoise(size, levels):
        texels, recv, irr, out = lists[size]
        prm = abi.lightmap_denoise_params(16, levels)
        plugin.check(lib.PTDenoiseLightmap(pt.ctx, C.byref(prm), texels.data_ptr(), recv.data_ptr(), irr.data_ptr(), texels.shape[0], size, size, out.data_ptr()))

    def gather(spp):
        _, recv, _, out = lists[1024]
        plugin.check(lib.PTGatherIrradiance(pt.ctx, C.byref(p), recv.data_ptr(), recv.shape[0], 0, spp, out.data_ptr()))

    legs = {"filter_1024": lambda: denoise(1024, LEVELS), "filter_2048": lambda: denoise(2048, LEVELS), "levels0_1024": lambda: denoise(1024, 0),
            "gather64": lambda: gather(64), "gather16": lambda: gather(16)}
    res = {k: [] for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            ms = timed((pt,), fn, args.steps, args.warmup)
            print(f"[lightmap_denoise_bench] {name}: {ms} ms per call", file=sys.stderr, flush=True)
            res[name].append(ms)
    med = {k: float(np.median(v)) for k, v in res.items()}

    texels, recv, irr16, _ = lists[1024]
    den16 = pt.denoise_lightmap(texels, recv, irr16, 1024, 1024, 16, iterations=LEVELS)
    errors, host = {}, {}
    if args.reference:
        irr64 = pt.irradiance(receivers=recv, spp=64, params=p)
        ref = pt.irradiance(receivers=recv, spp=args.reference, first_sample=1 << 20, params=p)[:, :3].double()
        for name, e in (("16", irr16), ("16_filtered", den16), ("64", irr64)):
            errors[name] = float(((e[:, :3].double() - ref) ** 2).mean().item())
        errors["reference_mean_square"] = float((ref ** 2).mean().item())
    if not args.no_host:
        t0 = time.perf_counter()
        twin = plugin.denoise_lightmap(texels.cpu().numpy().view(np.uint32), recv.cpu().numpy(), irr16.cpu().numpy(), 1024, 1024, 16, iterations=LEVELS)
        host = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "equal": bool(np.array_equal(twin.view(np.uint32), den16.cpu().numpy().view(np.uint32)))}
    texel_bytes = {size: size * size * (16 + LEVELS * 3 * 16) for size in lists}       # the flags' clear, then per level the guides and a state image read once
    result = {"levels": LEVELS, "samples": 16, "receivers": {size: int(v[0].shape[0]) for size, v in lists.items()}, "steps": args.steps,
              "warmup": args.warmup, "legs_ms_per_call": res, "median_ms_per_call": med,
              "filter_over_gather64": round(med["filter_1024"] / med["gather64"], 4),
              "filter16_plus_gather16_over_gather64": round((med["filter_1024"] + med["gather16"]) / med["gather64"], 4),
              "compulsory_GBps": {size: round(texel_bytes[size] / (med[f"filter_{size}"] * 1e-3) / 1e9, 1) for size in lists},
              "mse_against_reference": errors, "reference_samples": args.reference, "host_twin": host,
              "finite": bool(torch.isfinite(den16).all().item()), "device": torch.cuda.get_device_name(0)}
    pt.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
