"""Radiance queries on the Sponza-class scene: one JSON line.

Three legs, alternating in one process, `--legs` times each; every leg is `--steps` calls enqueued back to back after `--warmup`
(wall clock, as bench.py's headline; Mrays/s = rays traced / elapsed, PTStats at level 0 counts closest-hit and shadow rays):
  frame_order   PTTraceRadiance over the 1920x1080 camera rays of PTCameraRays (2,073,600 entries), in pixel-index order;
  shuffled      the same rays in a random order: what incoherent neighbours in a wave and in the slot arrays cost;
  render        PTRenderPassTo over the same frame with SamplesPerPass = 1, CurrentSample = 0: the same paths, bit for bit, with
                16x16-block slot order, passes in flight overlapping, and a frame written instead of a list.
No ratio is asserted: nobody has measured these before."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # as bench.py: the host's choice, before the first HIP call

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unity_webgpu_pathtracer_amd import scenes  # noqa: E402
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer  # noqa: E402

W, H = 1920, 1080


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


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", type=int, default=3, help="legs of each kind, alternating")
    args = ap.parse_args()

    s = scenes.sponza_atrium()
    pt = PathTracer(s, width=W, height=H, samplesPerPass=1)
    dev = f"cuda:{pt.device}"
    p = pt.params(seed=0x12345678)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    ordered = pt.camera_rays(pixels=torch.arange(W * H, dtype=torch.int32, device=dev), params=p)
    perm = torch.randperm(W * H, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    shuffled = ordered[perm].contiguous()
    torch.cuda.synchronize()

    # the two orders give the same results, and those are the frame's (checked here on the full-size problem; the tests hold it at 40x24)
    a = pt.radiance(ordered, spp=1, params=p)
    b = pt.radiance(shuffled, spp=1, params=p)
    pt.render_pass_to(p, frame.data_ptr(), 0)
    pt.synchronize()
    same_order = bool((a[perm].view(torch.int32) == b.view(torch.int32)).all().item())
    same_frame = bool((a[:, :3].contiguous().view(torch.int32) == frame.view(-1, 4)[:, :3].contiguous().view(torch.int32)).all().item())
    del a, b

    # priming as bench.py: every state set in use allocated and touched
    for _ in range(max(12, pt.passes_in_flight())):
        pt.render_pass_to(p, frame.data_ptr(), 0)
    pt.synchronize()

    legs = {"frame_order": lambda: pt.radiance(ordered, spp=1, params=p),
            "shuffled": lambda: pt.radiance(shuffled, spp=1, params=p),
            "render": lambda: pt.render_pass_to(p, frame.data_ptr(), 0)}
    res = {k: {"mrays": [], "ms_per_call": [], "paths_per_call": 0} for k in legs}
    for _ in range(args.legs):
        for name, fn in legs.items():
            mrays, ms, paths = timed(pt, fn, args.steps, args.warmup)
            res[name]["mrays"].append(mrays)
            res[name]["ms_per_call"].append(ms)
            res[name]["paths_per_call"] = paths
    out = {"image": f"{W}x{H}", "rays": W * H, "spp": 1, "max_bounces": pt.maxRayBounces, "steps": args.steps, "warmup": args.warmup,
           "schedule": pt.schedule(), "passes_in_flight": pt.passes_in_flight(), "shuffled_equals_frame_order": same_order,
           "frame_order_equals_render": same_frame, "legs": res,
           "median_ms_per_call": {k: float(np.median(v["ms_per_call"])) for k, v in res.items()},
           "device": torch.cuda.get_device_name(0)}
    pt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
