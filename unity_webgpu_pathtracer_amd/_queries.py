"""PathTracer's ray and radiance queries (include/ptmi_plugin.h Parts 3 and 8), the camera's rays, pick and focus."""
import ctypes as C

import numpy as np

from . import abi
from ._hostcalls import HostCalls, address, torch


class Queries(HostCalls):
    # ---- ray queries (include/ptmi_plugin.h Part 3)
    def trace_rays(self, rays, any_hit: bool = False, surface: bool = False):
        """Trace a batch of rays against the context's scene on the GPU.

        rays: (n, 8) float32 -- origin xyz, direction xyz, tmax, reserved (0) per row (PTRay).
          numpy array  -> PTTraceRaysHost, returns numpy arrays;
          torch tensor on this context's device -> PTTraceRays zero-copy, ordered against torch's current stream both ways
          (no host synchronisation), returns device tensors.
        Returns hits (n, 4) float32 = t, u, v, prim bits (view column 3 as uint32; 0xFFFFFFFF = miss), and with surface=True
        (closest hits only) also the surface records (n, 12) float32 = position xyz, t, normal xyz, materialIndex bits,
        uv, instance bits, prim bits -- written only where a hit was found (zeros elsewhere)."""
        if any_hit and surface:
            raise ValueError("surface records need closest-hit queries")
        flags = (abi.PT_QUERY_ANY_HIT if any_hit else abi.PT_QUERY_CLOSEST) | (abi.PT_QUERY_SURFACE if surface else 0)
        r, _ = self._as_rows(rays, 8, stage=False, strict=True)
        n = r.shape[0]
        hits, surf = self._twin_call(self.lib.PTTraceRays, self.lib.PTTraceRaysHost, r, [((n, 4), "float32"), ((n, 12), "float32", 0) if surface else None],
                                     tail=(flags,))
        return (hits, surf) if surface else hits

    # ---- radiance queries (include/ptmi_plugin.h Part 8)
    def camera_rays(self, pixels=None, seed: int = 0, current_sample: int = 0, params: abi.PTFrameParams = None):
        """PTCameraRays: the rays the render starts the first sample of its pixels with, as radiance() takes them.

        pixels: None = every pixel in index order (k = y * width + x); else pixel indices (uint32), as a numpy array or as a torch
          tensor on this context's device (int32 or uint32 storage).  An index outside the frame gives a NaN direction and rng 0.
        The camera, frame size, seed and CurrentSample are those of `params` when given, else of this tracer with `seed` and
        `current_sample`.  Returns (n, 8) float32 rows -- origin xyz, direction xyz, RNG state bits, 0 -- as a device tensor when
        `pixels` is a tensor, else as numpy."""
        p = self._radiance_params(params, seed, current_sample)
        as_numpy = not isinstance(pixels, torch.Tensor)
        if pixels is None:
            idx, n = None, p.OutputWidth * p.OutputHeight
        elif as_numpy:
            idx, _ = self._as_rows(np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1).view(np.int32), dtype=np.int32)
            n = idx.numel()
        else:
            assert pixels.device == self._device and pixels.dim() == 1 and pixels.is_contiguous() and pixels.element_size() == 4, (pixels.device, pixels.shape, pixels.dtype)
            idx, n = pixels, pixels.numel()
        return self._device_call(self.lib.PTCameraRays, [C.byref(p), None if idx is None else address(idx, "null"), n], [((n, 8), "float32")], as_numpy)

    def radiance(self, rays, spp: int = 1, params: abi.PTFrameParams = None):
        """Path-trace the radiance arriving along a batch of rays on the GPU, with the render's own code and settings.

        rays: (n, 8) float32 -- origin xyz, unit direction xyz, RNG state, reserved (0) per row (PTRadianceRay; columns 6 and 7
          are uint32 bits).  `spp` samples per ray; bounces, roulette, firefly filter from `params` (default: this tracer's).
          numpy array  -> PTTraceRadianceHost, returns numpy;
          torch tensor on this context's device -> PTTraceRadiance zero-copy, ordered against torch's current stream both ways
          (no host synchronisation), returns a device tensor.
        Returns (n, 4) float32 = mean rgb, RNG state after the last sample (view column 3 as uint32); feeding that state back in
        column 6 continues the chain."""
        p = self._radiance_params(params, spp=spp)
        r, _ = self._as_rows(rays, 8, stage=False, strict=True)
        return self._twin_call(self.lib.PTTraceRadiance, self.lib.PTTraceRadianceHost, r, [((r.shape[0], 4), "float32")], head=(C.byref(p),))

    def camera_ray(self, x: float, y: float, params: abi.PTFrameParams = None) -> np.ndarray:
        """The pinhole ray through the centre of pixel (x, y): util/camera.hlsl:13-42 without jitter and lens, in float32 with
        the device's operation order.  Returns one (8,) float32 ray row with tmax = PT_FAR_PLANE."""
        p = params or self.params(seed=0)
        f = np.float32
        inv = np.array(p.CamInvProj[:], np.float32)
        c2w = np.array(p.CamToWorld[:], np.float32)

        def mul44(m, v):
            return np.array([m[r] * v[0] + m[4 + r] * v[1] + m[8 + r] * v[2] + m[12 + r] * v[3] for r in range(4)], np.float32)
        o4 = mul44(c2w, np.array([0, 0, 0, 1], np.float32))
        uvx = (f(x) + f(0.5)) / f(p.OutputWidth) * f(2.0) - f(1.0)
        uvy = (f(y) + f(0.5)) / f(p.OutputHeight) * f(2.0) - f(1.0)
        d4 = mul44(inv, np.array([uvx, uvy, 0, 1], np.float32))
        w4 = mul44(c2w, np.array([d4[0], d4[1], d4[2], 0], np.float32))
        w = w4[:3]
        d = w * (f(1.0) / np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]))
        ray = np.zeros(8, np.float32)
        ray[0:3], ray[3:6], ray[6] = o4[:3], d, abi.PT_FAR_PLANE
        return ray

    def pick(self, x: float, y: float, params: abi.PTFrameParams = None):
        """What the camera sees through the centre of pixel (x, y): a dict with distance, position, normal, material,
        instance (None outside HAS_TLAS scenes), prim and uv -- or None when the ray misses the scene."""
        hits, surf = self.trace_rays(self.camera_ray(x, y, params)[None], surface=True)
        prim = int(hits[0, 3:4].view(np.uint32)[0])
        if prim == abi.PT_MISS:
            return None
        s = surf[0]
        inst = int(s[10:11].view(np.uint32)[0])
        return {"distance": float(hits[0, 0]), "position": s[0:3].copy(), "normal": s[4:7].copy(),
                "material": int(s[7:8].view(np.int32)[0]), "instance": None if inst == abi.PT_MISS else inst,
                "prim": prim, "uv": s[8:10].copy()}

    def camera_forward(self, params: abi.PTFrameParams = None) -> np.ndarray:
        """Unit view direction of the camera (the ray through the centre of the screen)."""
        p = params or self.params(seed=0)
        inv = np.array(p.CamInvProj[:], np.float64).reshape(4, 4).T
        c2w = np.array(p.CamToWorld[:], np.float64).reshape(4, 4).T
        d = inv @ np.array([0.0, 0.0, 0.0, 1.0])
        w = (c2w @ np.array([d[0], d[1], d[2], 0.0]))[:3]
        return w / np.linalg.norm(w)

    def focus_distance(self, x: float, y: float, params: abi.PTFrameParams = None):
        """Autofocus: the distance, along the camera's forward axis, of what pixel (x, y) sees (a thin-lens focalLength);
        None when it sees nothing."""
        hit = self.pick(x, y, params)
        if hit is None:
            return None
        d = self.camera_ray(x, y, params)[3:6].astype(np.float64)
        return float(hit["distance"] * np.dot(d, self.camera_forward(params)))
