"""Host-side mirror of the reference's render driver for the hot path.

`PathTracer` reproduces the caller contract of Assets/Scripts/PathTracer.cs (the C# MonoBehaviour cannot run
here): the inspector fields (PathTracer.cs:24-50), one `OnRenderImage` = one pass with the uniform block of
PathTracer.cs:230-249, the ping-pong / `_currentSample` bookkeeping of :268-272 and `Reset()` (:318-322).
`BVHScene` mirrors what BVHScene.cs does with the native plugin: BuildBVH -> sizes -> borrowed pointers ->
upload (BVHScene.cs:629-667), then binds the buffers (BVHScene.cs:140-167) through PTSetScene.

All compute goes through the C-ABI of libunity-webgpu-pathtracer-plugin.so (include/ptmi_plugin.h); nothing
here renders, traverses or shades on the host.
"""
import contextlib
import ctypes as C

import numpy as np

from . import abi, plugin
from .scenes import Scene, frame_params


class BVHScene:
    """Scene buffers as BVHScene.cs holds them, uploaded into HBM by PTSetScene."""

    def __init__(self, scene: Scene, build_device: int = None, node_capacity=None):
        """build_device = None: BuildBVH (the reference's CPU builder, byte-identical); k: PTBuildBVHDevice on HIP device k.
        node_capacity: room for in-place rebuilds (PTRebuildGeometry) -- a float factor >= 1 on every BLAS's node count (rounded
        up), or one absolute node count per BLAS (a number for a flat scene, a sequence per mesh otherwise); each BLAS's node span
        is padded with zero nodes and later offsets follow.  None: today's bytes."""
        self.scene = scene
        self.build_device = build_device
        self.node_capacity = node_capacity
        self.build_ms = {}
        self.tlas_data = None
        self.tlas_index_offset = 0
        self.gpu_instances = None
        if scene.use_tlas:
            self._build_two_level(scene)
        else:
            # BVHScene.cs:629-659: BuildBVH over the world-space triangle soup, copy node/triangle bytes out
            self.bvh_nodes, self.bvh_tris = plugin.build_cwbvh(scene.vertices, device=build_device, timing=self.build_ms)
            self.bvh_nodes = self._padded(self.bvh_nodes, 0)
            self.blas_spans = [(0, self.bvh_nodes.nbytes // 80, 0, self.bvh_tris.nbytes // 48)]
        self.tri_attrs = np.ascontiguousarray(scene.tri_attrs)
        self.materials = np.ascontiguousarray(scene.materials, dtype=np.float32)
        self.lights = np.ascontiguousarray(scene.lights, dtype=np.float32)
        self.texture_data = np.ascontiguousarray(scene.texture_data, dtype=np.uint32)

    def _padded(self, nodes: np.ndarray, blas: int) -> np.ndarray:
        """nodes with zero nodes appended up to node_capacity's count for BLAS number `blas`"""
        cap = self.node_capacity
        if cap is None:
            return nodes
        count = nodes.nbytes // 80
        if isinstance(cap, float):
            assert cap >= 1.0, "node_capacity as a factor must be >= 1"
            want = int(np.ceil(count * cap))
        else:
            want = int(cap[blas] if np.ndim(cap) else cap)
        assert want >= count, f"node_capacity {want} is below the BLAS's {count} nodes"
        return np.concatenate([nodes, np.zeros((want - count) * 80, np.uint8)])

    def _build_two_level(self, scene: Scene):
        """BVHScene.cs:600-758 with _useTLAS: one BLAS per unique mesh (local space), node / triangle buffers back to
        back, one GPUInstance + BLASInstance per renderer, BuildTLAS over the renderers' world bounds, TLASData =
        TLAS nodes followed by the instance indices at TLASIndexOffset."""
        from .scenes import instance_world_bounds
        nodes, tris, node_off, tri_off = [], [], [], []
        n_off = t_off = 0
        for t0, n in scene.mesh_ranges:
            nb, tb = plugin.build_cwbvh(scene.vertices[t0 * 3:(t0 + n) * 3], device=self.build_device)
            nb = self._padded(nb, len(nodes))
            nodes.append(nb)
            tris.append(tb)
            node_off.append(n_off)
            tri_off.append(t_off)
            n_off += nb.nbytes
            t_off += tb.nbytes
        self.bvh_nodes = np.concatenate(nodes)
        self.bvh_tris = np.concatenate(tris)
        self.blas_spans = [(node_off[m] // 80, nodes[m].nbytes // 80, tri_off[m] // 16, tris[m].nbytes // 48) for m in range(len(nodes))]
        gi = np.zeros(len(scene.instances), dtype=abi.GPU_INSTANCE)
        bi = np.zeros(len(scene.instances), dtype=abi.BLAS_INSTANCE)
        for k, (mesh, l2w, material) in enumerate(scene.instances):
            w2l = np.linalg.inv(l2w)
            gi[k]["localToWorld"] = l2w.T.reshape(16).astype(np.float32)       # Matrix4x4 memory order: (r, c) at c*4 + r
            gi[k]["worldToLocal"] = w2l.T.reshape(16).astype(np.float32)
            gi[k]["bvhOffset"] = node_off[mesh] // 80                            # kBVHNodeSize
            gi[k]["triOffset"] = tri_off[mesh] // 16                             # kBVHTriSize: float4 units
            gi[k]["triAttributeOffset"] = scene.mesh_ranges[mesh][0]             # in triangles
            gi[k]["materialIndex"] = material
            t0, n = scene.mesh_ranges[mesh]
            lo, hi = instance_world_bounds(scene.vertices[t0 * 3:(t0 + n) * 3], l2w)
            bi[k]["localToWorld"], bi[k]["worldToLocal"] = gi[k]["localToWorld"], gi[k]["worldToLocal"]
            bi[k]["aabbMin"], bi[k]["aabbMax"], bi[k]["blasIndex"] = lo, hi, k
        tlas_nodes, tlas_idx = plugin.build_tlas(bi)
        self.tlas_index_offset = tlas_nodes.nbytes // 4
        self.tlas_data = np.concatenate([tlas_nodes.view(np.float32), tlas_idx.view(np.float32)])
        self.gpu_instances = gi
        self.blas_instances = bi

    def desc(self) -> abi.PTSceneDesc:
        d = abi.PTSceneDesc()
        d.bvhNodes = self.bvh_nodes.ctypes.data
        d.bvhNodesBytes = self.bvh_nodes.nbytes
        d.bvhTris = self.bvh_tris.ctypes.data
        d.bvhTrisBytes = self.bvh_tris.nbytes
        d.triAttrs = self.tri_attrs.ctypes.data
        d.triAttrsBytes = self.tri_attrs.nbytes
        d.materials = self.materials.ctypes.data
        d.materialCount = self.materials.shape[0]
        d.lights = self.lights.ctypes.data if self.lights.size else None
        d.lightCount = self.lights.shape[0]
        d.textureData = self.texture_data.ctypes.data if self.texture_data.size else None
        d.textureDataUints = self.texture_data.size
        d.features = self.scene.features
        if self.tlas_data is not None:
            d.tlasData = self.tlas_data.ctypes.data
            d.tlasDataFloats = self.tlas_data.size
            d.tlasIndexOffset = self.tlas_index_offset
            d.instanceCount = self.gpu_instances.shape[0]
            d.gpuInstances = self.gpu_instances.ctypes.data
        if self.scene.environment_texture is not None:
            self.env_texture = np.ascontiguousarray(self.scene.environment_texture, dtype=np.float32)
            d.envTexture = self.env_texture.ctypes.data
            d.envHeight, d.envWidth = self.env_texture.shape[:2]
        return d

    def UpdateTLAS(self, ctx, local_to_world) -> bool:
        """BVHScene.UpdateTLAS (BVHScene.cs:769-841): for every instance whose localToWorld changed, recompute worldToLocal and
        the world bounds as _build_two_level does, rewrite its BLASInstance / GPUInstance records, then rebuild the TLAS --
        on the GPU, through PTUpdateInstances.  local_to_world: one 4x4 per instance.  Returns whether anything changed."""
        from .scenes import instance_world_bounds
        assert self.gpu_instances is not None, "UpdateTLAS needs a HAS_TLAS scene"
        assert len(local_to_world) == self.gpu_instances.shape[0]
        dirty = False
        for k, l2w in enumerate(local_to_world):
            l2w = np.asarray(l2w, np.float64)
            packed = l2w.T.reshape(16).astype(np.float32)
            if np.array_equal(packed.view(np.uint32), self.gpu_instances[k]["localToWorld"].view(np.uint32)):
                continue
            dirty = True
            mesh = self.scene.instances[k][0]
            w2l = np.linalg.inv(l2w)
            t0, n = self.scene.mesh_ranges[mesh]
            lo, hi = instance_world_bounds(self.scene.vertices[t0 * 3:(t0 + n) * 3], l2w)
            for rec in (self.gpu_instances[k], self.blas_instances[k]):
                rec["localToWorld"] = packed
                rec["worldToLocal"] = w2l.T.reshape(16).astype(np.float32)
            self.blas_instances[k]["aabbMin"], self.blas_instances[k]["aabbMax"] = lo, hi
        if dirty:
            plugin.check(plugin.load_library().PTUpdateInstances(ctx, self.blas_instances.ctypes.data, self.blas_instances.shape[0]))
        return dirty

    def PrepareShader(self, ctx):
        """BVHScene.PrepareShader (BVHScene.cs:140-167): bind the buffers to the kernel."""
        plugin.check(plugin.load_library().PTSetScene(ctx, C.byref(self.desc())))


def probe_grid(lo, hi, counts) -> np.ndarray:
    """Probe positions on a regular grid: counts = (nx, ny, nz) points from corner lo to corner hi inclusive (a count of 1 sits in
    the middle of its axis).  Returns (nx * ny * nz, 3) float32, x fastest, as probe_sh() takes them."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    counts = [int(c) for c in counts]
    assert len(counts) == 3 and min(counts) >= 1, counts
    axes = [np.linspace(lo[a], hi[a], counts[a]) if counts[a] > 1 else np.array([0.5 * (lo[a] + hi[a])]) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.float32)


class PathTracer:
    """One render context on one GPU, driven exactly as PathTracer.cs drives the compute shader."""

    def __init__(self, scene: Scene, device: int = 0, width: int = 256, height: int = 256,
                 samplesPerPass: int = 1, maxSamples: int = 100000, maxRayBounces: int = 4,
                 useRussianRoulette: bool = True, fireflyFilter: bool = False, maxFireflyLuminance: float = 10.0,
                 rank: int = 0, world_size: int = 1, reference_dispatch: bool = False, schedule: int = None,
                 build_device: int = None, track_noise: bool = False, node_capacity=None):
        self.lib = plugin.load_library()
        self.track_noise = track_noise          # OnRenderImage records every pass in the moments (PTAccumulateMoments)
        self.scene = scene
        self.width, self.height = width, height
        # inspector fields (PathTracer.cs:24-50)
        self.samplesPerPass = samplesPerPass
        self.maxSamples = maxSamples
        self.maxRayBounces = maxRayBounces
        self.useRussianRoulette = useRussianRoulette
        self.fireflyFilter = fireflyFilter
        self.maxFireflyLuminance = maxFireflyLuminance
        self.reference_dispatch = reference_dispatch
        # tonemapping settings (PathTracer.cs:41-48)
        self.tonemapMode = abi.TONEMAP_LOTTES
        self.sRGB = False
        self.exposure, self.brightness, self.contrast, self.saturation, self.vignette = 1.0, 1.0, 1.0, 1.0, 0.0
        self._currentSample = 0
        ctx = C.c_void_p()
        plugin.check(self.lib.PTCreate(device, C.byref(ctx)))
        self.ctx = ctx
        self.device = device
        self._bvhScene = BVHScene(scene, build_device=build_device, node_capacity=node_capacity)
        self._builtCost = {}                    # per BLAS: sahCost after its last build or rebuild (update_geometry's rebuild_above)
        self._bvhScene.PrepareShader(self.ctx)
        if world_size > 1:
            plugin.check(self.lib.PTSetTileOwnership(self.ctx, rank, world_size))
        self.rank, self.world_size = rank, world_size
        if schedule is not None:
            self.set_schedule(schedule)

    # ---- PathTracer.cs:318-322
    def Reset(self):
        self._currentSample = 0
        plugin.check(self.lib.PTResetFrames(self.ctx))

    def params(self, seed: int) -> abi.PTFrameParams:
        groups = (0, 0)
        if self.reference_dispatch:
            # Mathf.CeilToInt(_outputWidth / dx) with integer operands (PathTracer.cs:207-208): floor division
            groups = (self.width // 8, self.height // 8)
        return frame_params(self.scene, self.width, self.height, spp=self.samplesPerPass,
                            current_sample=self._currentSample, seed=seed, max_bounces=self.maxRayBounces,
                            russian_roulette=self.useRussianRoulette, firefly=self.fireflyFilter,
                            max_firefly_luminance=self.maxFireflyLuminance, dispatch_groups=groups)

    # ---- PathTracer.cs:188-280 (the render half; the tonemap blit is out of scope)
    def OnRenderImage(self, seed: int):
        """One progressive pass.  `seed` is RngSeedRoot (the C# host draws a fresh random value per frame, :233)."""
        if self._currentSample < self.maxSamples:
            p = self.params(seed)
            plugin.check(self.lib.PTRenderPass(self.ctx, C.byref(p)))
            if self.track_noise:
                plugin.check(self.lib.PTAccumulateMoments(self.ctx, C.byref(p), 1))       # after the pass, before the flip
        if self._currentSample < self.maxSamples:
            self._currentSample += max(1, self.samplesPerPass)
        if self._currentSample < self.maxSamples:
            plugin.check(self.lib.PTFlipFrames(self.ctx))
            self._flipped = True
        else:
            self._flipped = False

    def render_pass(self, p: abi.PTFrameParams):
        """Raw access: one pass with explicit params into the internal ping-pong frames (no bookkeeping)."""
        plugin.check(self.lib.PTRenderPass(self.ctx, C.byref(p)))

    def render_pass_to(self, p: abi.PTFrameParams, d_output: int, d_accumulated: int = 0):
        plugin.check(self.lib.PTRenderPassTo(self.ctx, C.byref(p), C.c_void_p(d_output), C.c_void_p(d_accumulated or None)))

    def render_batch_to(self, params, d_output: int, d_accumulated: int = 0):
        """PTRenderPassBatchTo: `params` = list of PTFrameParams (1..8 passes differing in RngSeedRoot / CurrentSample only)."""
        arr = (abi.PTFrameParams * len(params))(*params)
        plugin.check(self.lib.PTRenderPassBatchTo(self.ctx, arr, len(params), C.c_void_p(d_output), C.c_void_p(d_accumulated or None)))

    def flip(self):
        plugin.check(self.lib.PTFlipFrames(self.ctx))

    def synchronize(self):
        plugin.check(self.lib.PTSynchronize(self.ctx))

    def readback(self, last_output: bool = True) -> np.ndarray:
        """Current Output frame as (H, W, 4) float32.  After OnRenderImage flipped the targets the most recent
        output is frame[1-cur]; `last_output` accounts for that."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        flipped = last_output and getattr(self, "_flipped", False)
        if flipped:
            plugin.check(self.lib.PTFlipFrames(self.ctx))
        try:
            plugin.check(self.lib.PTReadback(self.ctx, out.ctypes.data_as(C.c_void_p), out.size))
        finally:
            if flipped:
                plugin.check(self.lib.PTFlipFrames(self.ctx))
        return out

    def frame_pointer(self, which: int = -1) -> int:
        return self.lib.PTGetFramePointer(self.ctx, which)

    def stream(self) -> int:
        return self.lib.PTGetStream(self.ctx)

    def set_stats_level(self, level: int):
        plugin.check(self.lib.PTSetStatsLevel(self.ctx, level))

    def stats(self) -> abi.PTStats:
        st = abi.PTStats()
        plugin.check(self.lib.PTGetStats(self.ctx, C.byref(st)))
        return st

    def reset_stats(self):
        plugin.check(self.lib.PTResetStats(self.ctx))

    def repack_stats(self) -> abi.PTRepackStats:
        """PTGetRepackStats: launch sequences with a repack candidate, candidates, repacks done and live slots moved"""
        st = abi.PTRepackStats()
        plugin.check(self.lib.PTGetRepackStats(self.ctx, C.byref(st)))
        return st

    def set_profiling(self, on: bool):
        plugin.check(self.lib.PTSetProfiling(self.ctx, 1 if on else 0))

    def timings(self) -> abi.PTTimings:
        t = abi.PTTimings()
        plugin.check(self.lib.PTGetTimings(self.ctx, C.byref(t)))
        return t

    def reset_timings(self):
        plugin.check(self.lib.PTResetTimings(self.ctx))

    # ---- PathTracer.cs:255-266: the presentation blit of _outputRT[_currentRT]
    def present_params(self) -> abi.PTPresentParams:
        q = abi.PTPresentParams()
        q.OutputWidth, q.OutputHeight = self.width, self.height
        q.Mode, q.sRGB = int(self.tonemapMode), 1 if self.sRGB else 0
        q.Exposure, q.Brightness, q.Contrast, q.Saturation, q.Vignette = (self.exposure, self.brightness, self.contrast,
                                                                          self.saturation, self.vignette)
        return q

    def present(self, q: abi.PTPresentParams = None) -> np.ndarray:
        """The displayable image of the current Output frame, (H, W, 4) float32."""
        q = q or self.present_params()
        out = np.empty((q.OutputHeight, q.OutputWidth, 4), dtype=np.float32)
        plugin.check(self.lib.PTPresentToHost(self.ctx, C.byref(q), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def present_to(self, q: abi.PTPresentParams, d_src: int, d_dst: int):
        plugin.check(self.lib.PTPresent(self.ctx, C.byref(q), C.c_void_p(d_src) if d_src else None, C.c_void_p(d_dst)))

    def set_schedule(self, schedule: int):
        plugin.check(self.lib.PTSetSchedule(self.ctx, schedule))

    def schedule(self) -> int:
        """The schedule the next pass runs with (auto resolved against the current scene)."""
        rc = self.lib.PTGetSchedule(self.ctx)
        if rc < 0:
            plugin.check(rc)
        return rc

    def set_wavefront_iterations(self, n: int):
        plugin.check(self.lib.PTSetWavefrontIterations(self.ctx, n))

    def set_passes_in_flight(self, n: int):
        """0 = default for the hardware queues the process asked for (GPU_MAX_HW_QUEUES); 1 = passes back to back."""
        plugin.check(self.lib.PTSetPassesInFlight(self.ctx, n))

    def set_sub_frames(self, n: int):
        """PTSetSubFrames: cut every pass into n interleaved sub-frames with their own launch sequences (1 = off)."""
        plugin.check(self.lib.PTSetSubFrames(self.ctx, n))

    def passes_in_flight(self) -> int:
        return self.lib.PTGetPassesInFlight(self.ctx)

    # ---- what the calls that take or return device tensors share
    @contextlib.contextmanager
    def _ordered(self, dev):
        """Orders what the block enqueues on the context stream against torch's current stream on `dev`, both ways, without a
        host synchronisation."""
        import torch
        cur = torch.cuda.current_stream(dev)
        ext = torch.cuda.ExternalStream(self.stream(), device=dev)
        ext.wait_stream(cur)                   # the inputs and the fresh outputs are ready before the call's work runs
        yield
        cur.wait_stream(ext)                   # torch's later work sees the results -- and any reuse of these buffers comes after

    @staticmethod
    def _seed_bits(seeds, n, dev):
        """(n,) int32 on `dev` holding the bits of uint32 seeds; None = the entry index"""
        import torch
        if seeds is None:
            return torch.arange(n, dtype=torch.int32, device=dev)
        sd = torch.as_tensor(seeds, device=dev).reshape(n).to(torch.int64).bitwise_and(0xFFFFFFFF)
        return torch.where(sd >= 2 ** 31, sd - 2 ** 32, sd).to(torch.int32)

    def _sample_rays(self, fn, rows, p, first_sample, spp):
        """PTGatherRays / PTProbeRays (`fn`) over receiver / probe rows: the (n * spp, 8) ray rows, numpy for numpy rows (uploaded
        and read back), else a device tensor"""
        import torch
        as_numpy = isinstance(rows, np.ndarray)
        dev = torch.device(f"cuda:{self.device}")
        d_rows = torch.from_numpy(rows).to(dev) if as_numpy else rows
        n = rows.shape[0]
        rays = torch.empty((n * max(spp, 0), 8), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(fn(self.ctx, C.byref(p), d_rows.data_ptr(), n, first_sample & 0xFFFFFFFF, spp, rays.data_ptr()))
        return rays.cpu().numpy() if as_numpy else rays

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
        if isinstance(rays, np.ndarray):
            r = np.ascontiguousarray(rays, dtype=np.float32)
            assert r.ndim == 2 and r.shape[1] == 8, r.shape
            n = r.shape[0]
            hits = np.empty((n, 4), np.float32)
            surf = np.zeros((n, 12), np.float32) if surface else None
            plugin.check(self.lib.PTTraceRaysHost(self.ctx, r.ctypes.data, n, flags, hits.ctypes.data,
                                                  surf.ctypes.data if surface else None))
            return (hits, surf) if surface else hits
        import torch
        assert rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8 and rays.is_contiguous(), (rays.dtype, rays.shape)
        dev = rays.device
        n = rays.shape[0]
        hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
        surf = torch.zeros((n, 12), dtype=torch.float32, device=dev) if surface else None
        with self._ordered(dev):
            plugin.check(self.lib.PTTraceRays(self.ctx, rays.data_ptr(), n, flags, hits.data_ptr(), surf.data_ptr() if surface else None))
        return (hits, surf) if surface else hits

    # ---- radiance queries (include/ptmi_plugin.h Part 8)
    def _radiance_params(self, params, seed=0, current_sample=0, spp=None):
        p = abi.PTFrameParams()
        C.memmove(C.byref(p), C.byref(params or self.params(seed=seed)), C.sizeof(p))
        if params is None:
            p.RngSeedRoot, p.CurrentSample = seed & 0xFFFFFFFF, current_sample
        if spp is not None:
            p.SamplesPerPass = spp
        return p

    def camera_rays(self, pixels=None, seed: int = 0, current_sample: int = 0, params: abi.PTFrameParams = None):
        """PTCameraRays: the rays the render starts the first sample of its pixels with, as radiance() takes them.

        pixels: None = every pixel in index order (k = y * width + x); else pixel indices (uint32), as a numpy array or as a torch
          tensor on this context's device (int32 or uint32 storage).  An index outside the frame gives a NaN direction and rng 0.
        The camera, frame size, seed and CurrentSample are those of `params` when given, else of this tracer with `seed` and
        `current_sample`.  Returns (n, 8) float32 rows -- origin xyz, direction xyz, RNG state bits, 0 -- as a device tensor when
        `pixels` is a tensor, else as numpy."""
        import torch
        p = self._radiance_params(params, seed, current_sample)
        dev = torch.device(f"cuda:{self.device}")
        as_numpy = not isinstance(pixels, torch.Tensor)
        if pixels is None:
            idx, n = None, p.OutputWidth * p.OutputHeight
        elif as_numpy:
            idx = torch.from_numpy(np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)
            n = idx.numel()
        else:
            assert pixels.device == dev and pixels.dim() == 1 and pixels.is_contiguous() and pixels.element_size() == 4, (pixels.device, pixels.shape, pixels.dtype)
            idx, n = pixels, pixels.numel()
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(self.lib.PTCameraRays(self.ctx, C.byref(p), idx.data_ptr() if idx is not None and n else None, n, rays.data_ptr()))
        return rays.cpu().numpy() if as_numpy else rays

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
        if isinstance(rays, np.ndarray):
            r = np.ascontiguousarray(rays, dtype=np.float32)
            assert r.ndim == 2 and r.shape[1] == 8, r.shape
            n = r.shape[0]
            out = np.empty((n, 4), np.float32)
            plugin.check(self.lib.PTTraceRadianceHost(self.ctx, C.byref(p), r.ctypes.data, n, out.ctypes.data))
            return out
        import torch
        assert rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8 and rays.is_contiguous(), (rays.dtype, rays.shape)
        dev = rays.device
        n = rays.shape[0]
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(self.lib.PTTraceRadiance(self.ctx, C.byref(p), rays.data_ptr(), n, out.data_ptr()))
        return out

    # ---- irradiance gathers (include/ptmi_plugin.h Part 13)
    def _receivers(self, positions, normals, seeds):
        """(n, 8) float32 PTReceiver rows -- position xyz, seed bits, normal xyz, 0 -- of the kind the positions are (numpy or a
        device tensor); seeds None = the entry index."""
        if isinstance(positions, np.ndarray) or not hasattr(positions, "device"):
            pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
            nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            assert pos.shape == nrm.shape, (pos.shape, nrm.shape)
            n = pos.shape[0]
            recv = np.zeros((n, 8), np.float32)
            recv[:, 0:3], recv[:, 4:7] = pos, nrm
            sd = np.arange(n, dtype=np.uint32) if seeds is None else np.ascontiguousarray(np.asarray(seeds).astype(np.uint32)).reshape(n)
            recv[:, 3] = sd.view(np.float32)
            return recv
        import torch
        assert positions.dtype == torch.float32 and normals.dtype == torch.float32 and positions.shape == normals.shape, (positions.shape, normals.shape)
        n = positions.reshape(-1, 3).shape[0]
        recv = torch.zeros((n, 8), dtype=torch.float32, device=positions.device)
        recv[:, 0:3], recv[:, 4:7] = positions.reshape(-1, 3), normals.reshape(-1, 3).to(positions.device)
        recv.view(torch.int32)[:, 3] = self._seed_bits(seeds, n, positions.device)
        return recv

    def irradiance(self, positions=None, normals=None, spp: int = 64, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None, receivers=None):
        """Irradiance at surface points on the GPU: lightmap texels, light probes.  Every receiver is a white Lambertian point;
        its `spp` samples run in parallel, lit directly by every light type (NEE at the receiver) and by the render's own paths
        from there on (bounces -- the receiver counts as the first --, roulette, firefly filter from `params`, default this tracer's).

        positions, normals: (n, 3) float32, unit normals; seeds: (n,) uint32, None = the entry index.  Samples
        [first_sample, first_sample + spp) of an entry are the same whatever calls they are split into.
          numpy arrays -> PTGatherIrradianceHost, returns numpy;
          torch tensors on this context's device -> PTGatherIrradiance zero-copy, ordered against torch's current stream both ways.
        receivers (instead of positions, normals and seeds): ready-made (n, 8) float32 PTReceiver rows, as chart_receivers returns them.
        Returns (n, 4) float32: irradiance rgb (mean over the samples) and m2, the sum of the samples' squared luminance."""
        p = self._radiance_params(params)
        if receivers is not None:
            assert positions is None and normals is None and seeds is None, "receivers come instead of positions, normals and seeds"
            assert receivers.dtype == np.float32 or str(receivers.dtype) == "torch.float32", receivers.dtype
            assert receivers.ndim == 2 and receivers.shape[1] == 8, receivers.shape
            recv = np.ascontiguousarray(receivers) if isinstance(receivers, np.ndarray) else receivers.contiguous()
        else:
            recv = self._receivers(positions, normals, seeds)
        n = recv.shape[0]
        if isinstance(recv, np.ndarray):
            out = np.empty((n, 4), np.float32)
            plugin.check(self.lib.PTGatherIrradianceHost(self.ctx, C.byref(p), recv.ctypes.data, n, first_sample & 0xFFFFFFFF, spp, out.ctypes.data))
            return out
        import torch
        out = torch.empty((n, 4), dtype=torch.float32, device=recv.device)
        with self._ordered(recv.device):
            plugin.check(self.lib.PTGatherIrradiance(self.ctx, C.byref(p), recv.data_ptr(), n, first_sample & 0xFFFFFFFF, spp, out.data_ptr()))
        return out

    # ---- adaptive gathers (include/ptmi_plugin.h Part 19)
    def irradiance_adaptive(self, positions=None, normals=None, threshold: float = None, min_samples: int = 16, add_samples: int = 16,
                            max_samples: int = 1024, dark_floor: float = None, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None,
                            receivers=None):
        """irradiance() with more samples only where the result is still noisy (PTGatherIrradianceAdaptive; Part 19 has the rule):
        `min_samples` of every receiver, then rounds of `add_samples` for the receivers whose relative standard error of the mean
        luminance is above `threshold`, until none is left or `max_samples` would be passed.  A receiver that stops stays stopped.
        Every round is irradiance() over the receivers still active, so the result of a receiver is the fold (plugin.fold_irradiance)
        of irradiance() results over the same sample ranges, bit for bit.

        Inputs as irradiance(): numpy -> PTGatherIrradianceAdaptiveHost, returns numpy; device tensors -> zero-copy, ordered
        against torch's current stream both ways (the call itself synchronises once per round).
        dark_floor: the luminance below which the error is measured against dark_floor instead of the receiver's own luminance
        (a black receiver would never converge relatively).  None: 1 % of the mean luminance of the finite entries of a
        `min_samples` gather -- computed here by running round 0 through irradiance() first and passing the number down, so the
        C call keeps one contract; that costs one extra round 0.
        Returns (irradiance (n, 4) float32: rgb and m2 over the receiver's own samples, counts (n,) int32 / uint32: samples per
        receiver, stats: a dict of PTAdaptiveGatherStats -- rounds, samples, stoppedThreshold, stoppedMaxSamples, stoppedNonFinite,
        maxCount -- and darkFloor)."""
        assert threshold is not None, "threshold: the relative standard error to reach"
        p = self._radiance_params(params)
        if receivers is not None:
            assert positions is None and normals is None and seeds is None, "receivers come instead of positions, normals and seeds"
            assert receivers.dtype == np.float32 or str(receivers.dtype) == "torch.float32", receivers.dtype
            assert receivers.ndim == 2 and receivers.shape[1] == 8, receivers.shape
            recv = np.ascontiguousarray(receivers) if isinstance(receivers, np.ndarray) else receivers.contiguous()
        else:
            recv = self._receivers(positions, normals, seeds)
        n = recv.shape[0]
        if dark_floor is None:
            first = self.irradiance(receivers=recv, spp=min_samples, first_sample=first_sample, params=p) if n else np.zeros((0, 4), np.float32)
            first = first if isinstance(first, np.ndarray) else first.cpu().numpy()
            rgb = first[np.isfinite(first).all(axis=1), :3].astype(np.float64)
            dark_floor = 0.01 * float((rgb @ np.array([0.299, 0.587, 0.114])).mean()) if len(rgb) else 0.0
            dark_floor = dark_floor if np.isfinite(dark_floor) and dark_floor > 0.0 else 0.0
        a = abi.adaptive_gather(threshold, min_samples, add_samples, max_samples, dark_floor, first_sample)
        st = abi.PTAdaptiveGatherStats()
        if isinstance(recv, np.ndarray):
            out, counts = np.empty((n, 4), np.float32), np.empty(n, np.uint32)
            plugin.check(self.lib.PTGatherIrradianceAdaptiveHost(self.ctx, C.byref(p), C.byref(a), recv.ctypes.data, n, out.ctypes.data, counts.ctypes.data,
                                                                 C.byref(st)))
        else:
            import torch
            out = torch.empty((n, 4), dtype=torch.float32, device=recv.device)
            counts = torch.empty((n,), dtype=torch.int32, device=recv.device)
            with self._ordered(recv.device):
                plugin.check(self.lib.PTGatherIrradianceAdaptive(self.ctx, C.byref(p), C.byref(a), recv.data_ptr(), n, out.data_ptr(), counts.data_ptr(),
                                                                 C.byref(st)))
        return out, counts, dict(st.as_dict(), darkFloor=float(a.darkFloor))

    def equalise_irradiance(self, irradiance, counts, samples_eq: int):
        """PTEqualiseIrradiance: rewrites m2 of an irradiance_adaptive() list (device tensors: (n, 4) float32 and (n,) int32 counts) so
        that denoise_lightmap(..., samples=samples_eq) recovers every entry's own variance of the mean.  Returns a new (n, 4) tensor."""
        import torch
        n = irradiance.shape[0]
        assert irradiance.dtype == torch.float32 and irradiance.is_contiguous() and irradiance.shape == (n, 4), irradiance.shape
        assert counts.element_size() == 4 and counts.is_contiguous() and counts.shape == (n,), counts.shape
        out = torch.empty_like(irradiance)
        with self._ordered(irradiance.device):
            plugin.check(self.lib.PTEqualiseIrradiance(self.ctx, irradiance.data_ptr() if n else None, counts.data_ptr() if n else None, n, int(samples_eq),
                                                       out.data_ptr() if n else None))
        return out

    def gather_rays(self, positions, normals, spp: int = 64, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None):
        """PTGatherRays: the gather ray and RNG state each sample of irradiance() leaves the receiver with, as radiance() takes
        them: (n * spp, 8) float32 rows, entry-major (row i * spp + j = sample first_sample + j of entry i); a sample that ended at
        the receiver has a NaN direction.  numpy in, numpy out; device tensors in, a device tensor out."""
        return self._sample_rays(self.lib.PTGatherRays, self._receivers(positions, normals, seeds), self._radiance_params(params), first_sample, spp)

    # ---- SH light probes (include/ptmi_plugin.h Part 15)
    def _probes(self, positions, seeds):
        """(n, 4) float32 PTProbe rows -- position xyz, seed bits -- of the kind the positions are; seeds None = the probe index."""
        if isinstance(positions, np.ndarray) or not hasattr(positions, "device"):
            return plugin.probe_rows(positions, seeds)
        import torch
        assert positions.dtype == torch.float32, positions.dtype
        pos = positions.reshape(-1, 3)
        n = pos.shape[0]
        rows = torch.empty((n, 4), dtype=torch.float32, device=pos.device)
        rows[:, 0:3] = pos
        rows.view(torch.int32)[:, 3] = self._seed_bits(seeds, n, pos.device)
        return rows

    def probe_sh(self, positions, spp: int = 256, first_sample: int = 0, seeds=None, delta_lights: bool = True, params: abi.PTFrameParams = None):
        """SH light probes on the GPU: what lights an object that moves through a baked scene.  Every probe is a point without a
        normal; its `spp` samples -- uniform directions made on the GPU, each a path of the render's own (bounces, roulette, firefly
        filter from `params`, default this tracer's) -- run in parallel and are projected onto real SH bands 0 to 2.  delta_lights:
        add the direct light of point and spot lights, which no path can hit (one shadow ray per probe and light).

        positions: (n, 3) float32; seeds: (n,) uint32, None = the probe index.  Samples [first_sample, first_sample + spp) of a
        probe are the same whatever calls they are split into (average the coefficients of equal-sized calls).
          numpy array -> PTProbeSHHost, returns numpy;
          torch tensor on this context's device -> PTProbeSH zero-copy, ordered against torch's current stream both ways.
        Returns (sh, m2): sh (n, 9, 3) float32, coefficient k and channel c; m2 (n,) the sum of the samples' squared luminance."""
        p = self._radiance_params(params)
        rows = self._probes(positions, seeds)
        n = rows.shape[0]
        flags = abi.PT_PROBE_DELTA_LIGHTS if delta_lights else 0
        if isinstance(rows, np.ndarray):
            out = np.empty((n, 28), np.float32)
            plugin.check(self.lib.PTProbeSHHost(self.ctx, C.byref(p), rows.ctypes.data, n, first_sample & 0xFFFFFFFF, spp, flags, out.ctypes.data))
            return out[:, :27].reshape(n, 9, 3).copy(), out[:, 27].copy()
        import torch
        out = torch.empty((n, 28), dtype=torch.float32, device=rows.device)
        with self._ordered(rows.device):
            plugin.check(self.lib.PTProbeSH(self.ctx, C.byref(p), rows.data_ptr(), n, first_sample & 0xFFFFFFFF, spp, flags, out.data_ptr()))
        return out[:, :27].reshape(n, 9, 3), out[:, 27]

    def probe_rays(self, positions, spp: int = 256, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None):
        """PTProbeRays: the ray and RNG state each sample of probe_sh() starts with, as radiance() takes them: (n * spp, 8) float32
        rows, entry-major (row i * spp + j = sample first_sample + j of probe i).  numpy in, numpy out; a device tensor in, a
        device tensor out."""
        return self._sample_rays(self.lib.PTProbeRays, self._probes(positions, seeds), self._radiance_params(params), first_sample, spp)

    def probe_irradiance(self, sh, normals, probes):
        """PTProbeIrradiance: the irradiance the coefficients of probe_sh() give for unit normals.  sh (n, 9, 3), normals (q, 3),
        probes (q,) indices into sh (an index >= n gives zeros).  Returns (q, 4) float32 PTIrradiance rows, m2 = 0.  numpy in, numpy
        out; device tensors in, a device tensor out."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        as_numpy = isinstance(sh, np.ndarray) or not hasattr(sh, "device")
        if as_numpy:
            d_sh = torch.from_numpy(plugin.probe_coeff_rows(sh)).to(dev)
            d_q = torch.from_numpy(plugin.probe_query_rows(normals, probes)).to(dev)
        else:
            assert sh.dtype == torch.float32 and normals.dtype == torch.float32, (sh.dtype, normals.dtype)
            d_sh = torch.zeros((sh.reshape(-1, 27).shape[0], 28), dtype=torch.float32, device=dev)
            d_sh[:, :27] = sh.reshape(-1, 27)
            nrm = normals.reshape(-1, 3)
            d_q = torch.empty((nrm.shape[0], 4), dtype=torch.float32, device=dev)
            d_q[:, 0:3] = nrm
            d_q.view(torch.int32)[:, 3] = self._seed_bits(probes, -1, dev)
        q = d_q.shape[0]
        out = torch.empty((q, 4), dtype=torch.float32, device=dev)
        if q:
            with self._ordered(dev):
                plugin.check(self.lib.PTProbeIrradiance(self.ctx, d_sh.data_ptr() if d_sh.shape[0] else None, d_sh.shape[0], d_q.data_ptr(), q, out.data_ptr()))
        return out.cpu().numpy() if as_numpy else out

    probe_grid = staticmethod(probe_grid)

    # ---- probe volumes (include/ptmi_plugin.h Part 16)
    def probe_depth(self, positions, spp: int = 256, max_distance: float = 1.0, first_sample: int = 0, seeds=None):
        """PTProbeDepth: an 8 x 8 octahedral map of the distances each probe sees, what a probe volume's lookup keeps light from
        leaking through walls with.  Sample j of a probe has probe_sh()'s direction; its ray is a closest-hit query that ends at
        max_distance, and every texel keeps the cos^32-weighted mean distance and mean squared distance of all samples.

        positions: (n, 3) float32; seeds: (n,) uint32, None = the probe index.
          numpy array -> PTProbeDepthHost, returns numpy;
          torch tensor on this context's device -> PTProbeDepth zero-copy, ordered against torch's current stream both ways.
        Returns (n, 64, 2) float32: texel v * 8 + u, mean and mean square."""
        rows = self._probes(positions, seeds)
        n = rows.shape[0]
        if isinstance(rows, np.ndarray):
            out = np.empty((n, 64, 2), np.float32)
            plugin.check(self.lib.PTProbeDepthHost(self.ctx, rows.ctypes.data, n, first_sample & 0xFFFFFFFF, spp, max_distance, out.ctypes.data))
            return out
        import torch
        out = torch.empty((n, 64, 2), dtype=torch.float32, device=rows.device)
        with self._ordered(rows.device):
            plugin.check(self.lib.PTProbeDepth(self.ctx, rows.data_ptr(), n, first_sample & 0xFFFFFFFF, spp, max_distance, out.data_ptr()))
        return out

    # ---- reflection probes (include/ptmi_plugin.h Part 20)
    def reflection_rays(self, positions, res: int = 64, spp: int = 16, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None):
        """PTReflectionRays: the ray and RNG state each sample of capture_reflection_probes() starts with, as radiance() takes them:
        (n * res * res * spp, 8) float32 rows, slot-major (row (i * res * res + t) * spp + j = sample first_sample + j of texel t of
        probe i).  numpy in, numpy out; a device tensor in, a device tensor out."""
        import torch
        p = self._radiance_params(params)
        rows = self._probes(positions, seeds)
        as_numpy = isinstance(rows, np.ndarray)
        dev = torch.device(f"cuda:{self.device}")
        d_rows = torch.from_numpy(rows).to(dev) if as_numpy else rows
        n = rows.shape[0]
        ok = abi.PT_REFLECTION_MIN_RES <= res <= abi.PT_REFLECTION_MAX_RES and 0 <= spp <= 65536     # (the call refuses the rest itself)
        rays = torch.empty((n * res * res * spp if ok else 0, 8), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(self.lib.PTReflectionRays(self.ctx, C.byref(p), d_rows.data_ptr() or 16, n, res, first_sample & 0xFFFFFFFF, spp, rays.data_ptr() or 16))
        return rays.cpu().numpy() if as_numpy else rays            # (`or 16`: an empty tensor has no address, and count == 0 reads none)

    def capture_reflection_base(self, positions, res: int = 64, spp: int = 16, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None):
        """PTReflectionCapture: the base maps alone, (n, res * res, 4) float32 -- mean radiance rgb and the sum of the samples' squared
        luminances per texel v * res + u of the octahedral map.  numpy positions -> PTReflectionCaptureHost, returns numpy; a device
        tensor -> PTReflectionCapture zero-copy, ordered against torch's current stream both ways, returns a device tensor."""
        p = self._radiance_params(params)
        rows = self._probes(positions, seeds)
        n = rows.shape[0]
        ok = abi.PT_REFLECTION_MIN_RES <= res <= abi.PT_REFLECTION_MAX_RES
        shape = (n, res * res if ok else 1, 4)
        if isinstance(rows, np.ndarray):
            out = np.empty(shape, np.float32)
            plugin.check(self.lib.PTReflectionCaptureHost(self.ctx, C.byref(p), rows.ctypes.data, n, res, first_sample & 0xFFFFFFFF, spp, out.ctypes.data))
            return out
        import torch
        out = torch.empty(shape, dtype=torch.float32, device=rows.device)
        with self._ordered(rows.device):
            plugin.check(self.lib.PTReflectionCapture(self.ctx, C.byref(p), rows.data_ptr() or 16, n, res, first_sample & 0xFFFFFFFF, spp, out.data_ptr() or 16))
        return out

    def prefilter_reflection(self, base, res: int, levels: int):
        """PTReflectionPrefilter: base maps (n, res * res, 4) float32 -> whole maps (n, plugin.reflection_texel_count(res, levels), 4),
        level k filtered with the GGX lobe of roughness k / (levels - 1).  numpy in, numpy out; a device tensor in, a device tensor
        out."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        as_numpy = isinstance(base, np.ndarray)
        d_base = torch.from_numpy(np.ascontiguousarray(base, dtype=np.float32)).to(dev) if as_numpy else base.contiguous()
        assert d_base.dtype == torch.float32 and d_base.dim() == 3 and d_base.shape[2] == 4, (d_base.dtype, d_base.shape)
        n = d_base.shape[0]
        ok = abi.PT_REFLECTION_MIN_RES <= res <= abi.PT_REFLECTION_MAX_RES and 1 <= levels <= 8
        out = torch.empty((n, plugin.reflection_texel_count(res, levels) if ok else 1, 4), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(self.lib.PTReflectionPrefilter(self.ctx, d_base.data_ptr() or 16, n, res, levels, out.data_ptr() or 32))
        return out.cpu().numpy() if as_numpy else out

    def capture_reflection_probes(self, positions, res: int = 64, spp: int = 16, levels: int = 5, first_sample: int = 0, seeds=None, boxes=None,
                                  params: abi.PTFrameParams = None):
        """Reflection probes on the GPU: what a glossy object that moves through a baked scene reads.  Every probe is an octahedral
        radiance map of res x res texels around a point, `spp` paths of the render's own per texel (jittered inside the texel;
        bounces, roulette, firefly filter from `params`, default this tracer's), prefiltered into `levels` levels of roughness
        0 ... 1 with the GGX lobe.  boxes: None, or (bmin, bmax), each (n, 3) or (3,): the box each probe's surroundings stand for,
        which lookup() projects directions onto (parallax correction).

        positions: (n, 3) float32, numpy or a tensor on this context's device; seeds: (n,) uint32, None = the probe index.  Returns a
        ReflectionProbes, whose maps stay on the device."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        rows = self._probes(positions, seeds)
        d_rows = torch.from_numpy(rows).to(dev) if isinstance(rows, np.ndarray) else rows
        base = self.capture_reflection_base(d_rows[:, 0:3].contiguous(), res, spp, first_sample, d_rows.view(torch.int32)[:, 3], params)
        maps = self.prefilter_reflection(base, res, levels)
        d_boxes = None
        if boxes is not None:
            n = d_rows.shape[0]
            lo, hi = (np.broadcast_to(np.asarray(b, np.float32), (n, 3)) for b in boxes)
            d_boxes = torch.from_numpy(plugin.reflection_box_rows(lo, hi)).to(dev)
        return ReflectionProbes(self, res, levels, maps, d_rows, d_boxes)

    # ---- shading from the bakes (include/ptmi_plugin.h Part 21)
    def _to_device(self, x, cols=None):
        """(tensor on this context's device, was numpy): float32, contiguous, (n, cols) when cols is given"""
        import torch
        as_numpy = isinstance(x, np.ndarray)
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.device(f"cuda:{self.device}")) if as_numpy else x.contiguous()
        assert t.dtype == torch.float32 and (cols is None or (t.dim() == 2 and t.shape[1] == cols)), (t.dtype, t.shape, cols)
        return t, as_numpy

    def bake_dfg(self, res: int = 32):
        """PTBakeDFG: the split-sum table of the specular BRDF on the GPU, a (res, res, 2) float32 device tensor -- row j =
        perceptual roughness (j + 0.5) / res, column i = N.V (i + 0.5) / res, {scale, bias} of F0; plugin.bake_dfg is its twin."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        ok = int(res) in abi.PT_SHADE_DFG_RES                                 # (the call refuses another res itself)
        out = torch.empty((res, res, 2) if ok else (1, 1, 2), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(self.lib.PTBakeDFG(self.ctx, int(res), out.data_ptr()))
        return out

    def shade_surfaces(self, rays, hits, surfaces, probes=None, boxes=None):
        """PTShadeSurfaces: from what trace_rays(rays, surface=True) took and returned to what the bakes are asked -- the material
        record the render's own fetch gives for every hit (n, 12), the shading terms (n, 12), the PTReceiver rows (n, 8) a probe
        volume takes and the PTReflectionQuery rows (n, 8) reflection probes take.  probes: (k, 4) PTProbe rows or (k, 3)
        positions, or None; boxes: (k, 8) PTReflectionBox rows or None.  numpy in, numpy out; device tensors in, device tensors
        out."""
        import torch
        r, as_numpy = self._to_device(rays, 8)
        h, _ = self._to_device(hits, 4)
        s, _ = self._to_device(surfaces, 12)
        n, dev = r.shape[0], r.device
        assert h.shape[0] == n and s.shape[0] == n, (r.shape, h.shape, s.shape)
        pr = None
        if probes is not None:
            pr = self._to_device(probes if probes.shape[1] == 4 else self._probes(probes, None), 4)[0]
        bx = None if boxes is None else self._to_device(boxes, 8)[0]
        k = 0 if pr is None else pr.shape[0]
        outs = [torch.empty((n, c), dtype=torch.float32, device=dev) for c in (12, 12, 8, 8)]
        if n:
            with self._ordered(dev):
                plugin.check(self.lib.PTShadeSurfaces(self.ctx, r.data_ptr(), h.data_ptr(), s.data_ptr(), n, pr.data_ptr() if k else None,
                                                      None if bx is None else bx.data_ptr(), k, *[o.data_ptr() for o in outs]))
        return tuple(o.cpu().numpy() for o in outs) if as_numpy else tuple(outs)

    def shade_compose(self, terms, irradiance, reflection, dfg):
        """PTShadeCompose: emission + occlusion * (diffuse * E / pi + spec * (f0 * A + B)) per entry, (A, B) bilinear in the DFG
        table at (N.V, roughness).  terms (n, 12), irradiance (n, 4), reflection (n, 4), dfg (res, res, 2).  Returns (n, 4): rgb and
        1, zeros for a miss.  numpy in, numpy out; device tensors in, a device tensor out."""
        import torch
        t, as_numpy = self._to_device(terms, 12)
        e, _ = self._to_device(irradiance, 4)
        s, _ = self._to_device(reflection, 4)
        d, _ = self._to_device(dfg)
        n = t.shape[0]
        assert e.shape[0] == n and s.shape[0] == n and d.dim() == 3 and d.shape[0] == d.shape[1] and d.shape[2] == 2, (t.shape, e.shape, s.shape, d.shape)
        out = torch.empty((n, 4), dtype=torch.float32, device=t.device)
        if n:
            with self._ordered(t.device):
                plugin.check(self.lib.PTShadeCompose(self.ctx, t.data_ptr(), e.data_ptr(), s.data_ptr(), n, d.data_ptr(), d.shape[0], out.data_ptr()))
        return out.cpu().numpy() if as_numpy else out

    def _shade_inputs(self, volume, reflections, dfg, wrap=True, visibility=True, normal_bias=None, placement=True, boxes=True):
        """(PTShadeInputs, the tensors it points into) from a ProbeVolume, a ReflectionProbes or None (no probes: the specular term
        reads zeros) and a DFG table or None (a 32 x 32 table, baked once per context)"""
        if dfg is None:
            if getattr(self, "_dfg", None) is None:
                self._dfg = self.bake_dfg(32)
            dfg = self._dfg
        d, _ = self._to_device(dfg)
        s = abi.PTShadeInputs()
        s.grid = abi.PTProbeGrid.from_buffer_copy(volume.grid)
        s.grid.flags = (abi.PT_GRID_WRAP if wrap else 0) | (abi.PT_GRID_VISIBILITY if visibility else 0)
        s.grid.normalBias = volume.default_normal_bias() if normal_bias is None else float(normal_bias)
        s.dSH, s.dDepth = volume._rows.data_ptr(), volume._depth.data_ptr()
        s.dPlacement = volume.placement.data_ptr() if placement and volume.placement is not None else None
        s.res, s.levels = 8, 2
        if reflections is not None and reflections.probe_rows.shape[0]:
            s.dMaps, s.dProbes = reflections.maps.data_ptr(), reflections.probe_rows.data_ptr()
            s.dBoxes = reflections.box_rows.data_ptr() if boxes and reflections.box_rows is not None else None
            s.probeCount, s.res, s.levels = reflections.probe_rows.shape[0], reflections.res, reflections.levels
        s.dDFG, s.dfgRes = d.data_ptr(), d.shape[0]
        return s, (d, volume, reflections)

    def shade_baked(self, rays, hits, surfaces, volume, reflections=None, dfg=None, **options):
        """PTShadeBaked: the first hits of trace_rays(rays, surface=True) shaded from a ProbeVolume and a ReflectionProbes in one
        kernel -- the material fetch, the terms, the volume's lookup (the placed one for a volume with a placement), the nearest
        reflection probe's lookup (the nearest whose box holds the point, with boxes) and the compose step, bit for bit what
        shade_surfaces, volume.irradiance, reflections.lookup and shade_compose give one after the other.  options: wrap,
        visibility, normal_bias as ProbeVolume.irradiance takes them; placement=False, boxes=False leave those out.  Returns
        (n, 4) float32: rgb and 1, zeros for a miss.  numpy in, numpy out; device tensors in, a device tensor out."""
        import torch
        r, as_numpy = self._to_device(rays, 8)
        h, _ = self._to_device(hits, 4)
        sf, _ = self._to_device(surfaces, 12)
        n = r.shape[0]
        assert h.shape[0] == n and sf.shape[0] == n, (r.shape, h.shape, sf.shape)
        s, keep = self._shade_inputs(volume, reflections, dfg, **options)
        out = torch.empty((n, 4), dtype=torch.float32, device=r.device)
        if n:
            with self._ordered(r.device):
                plugin.check(self.lib.PTShadeBaked(self.ctx, C.byref(s), r.data_ptr(), h.data_ptr(), sf.data_ptr(), n, out.data_ptr()))
        del keep
        return out.cpu().numpy() if as_numpy else out

    def render_baked(self, params: abi.PTFrameParams, volume, reflections=None, dfg=None, return_rays: bool = False, **options):
        """PTShadeBakedFrame: the frame `params` describes (None: this tracer's), every pixel's centre ray traced to its first hit
        and shaded from the bakes: a view of the scene lit by a ProbeVolume and a ReflectionProbes, as they are returned by
        bake_probe_volume and capture_reflection_probes.  dfg: a DFG table, None = a 32 x 32 one baked once per context.  Returns
        the (height, width, 4) float32 device tensor, and with return_rays the (height * width, 8) PTRay rows it traced."""
        import torch
        p = params or self.params(seed=0)
        dev = torch.device(f"cuda:{self.device}")
        s, keep = self._shade_inputs(volume, reflections, dfg, **options)
        w, h = int(p.OutputWidth), int(p.OutputHeight)
        out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
        rays = torch.empty((h * w, 8), dtype=torch.float32, device=dev) if return_rays else None
        with self._ordered(dev):
            plugin.check(self.lib.PTShadeBakedFrame(self.ctx, C.byref(p), C.byref(s), out.data_ptr(), rays.data_ptr() if return_rays else None))
        del keep
        return (out, rays) if return_rays else out

    # ---- first hits shaded from baked lightmaps (include/ptmi_plugin.h Part 22)
    def lightmap_binding(self, image, mesh: int = None, instance: int = None, uvs=None, two_sided: bool = False):
        """One entry for bind_lightmaps: `image`, an (height, width, 4) float32 lightmap as bake_lightmap / resolve_lightmap return it
        (numpy, or a tensor on this context's device; w > 0 marks a filled texel), bound to the primitives of one mesh.  mesh names
        the BLAS as chart_receivers does (None on a flat scene: the whole scene).  instance: None = whichever instance was hit (the
        only choice on a flat scene), else only hits of that instance read this image.  uvs: the (T, 6) float32 lightmap UVs the
        image was baked with, None = the attribute records' uv0 .. uv2.  two_sided: hits seen from behind read it too.  The entry
        keeps its tensors alive."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        img = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(dev)
        img = img.contiguous()
        assert img.dtype == torch.float32 and img.dim() == 3 and img.shape[2] == 4 and img.device == dev, (img.shape, img.dtype, img.device)
        bvh = self._bvhScene
        assert bvh.gpu_instances is not None or instance is None, "a flat scene has no instances"
        first, count = self._blas_offsets(mesh)[2], bvh.blas_spans[0 if mesh is None else mesh][3]
        d_uvs = None
        if uvs is not None:
            d_uvs = (uvs if isinstance(uvs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(uvs, dtype=np.float32)).to(dev)).contiguous()
            assert d_uvs.dtype == torch.float32 and d_uvs.numel() == count * 6 and d_uvs.device == dev, (d_uvs.shape, d_uvs.dtype)
        b = abi.PTLightmapBinding()
        b.firstPrim, b.primCount = int(first), int(count)
        b.instance = abi.PT_LIGHTMAP_NONE if instance is None else int(instance)
        b.flags = abi.PT_LIGHTMAP_TWO_SIDED if two_sided else 0
        b.height, b.width = int(img.shape[0]), int(img.shape[1])
        b.dImage = img.data_ptr()
        b.dUvs = None if d_uvs is None else d_uvs.data_ptr()
        return {"record": b, "image": img, "uvs": d_uvs, "mesh": mesh, "instance": instance, "two_sided": bool(two_sided)}

    def bind_lightmaps(self, bindings):
        """PTBindLightmaps: the list of lightmap_binding entries (at most 64; the first one that matches a hit wins) replaces what
        was bound; an empty list unbinds.  Stream-ordered with the shading calls; the entries' tensors stay alive while bound."""
        import torch
        bindings = list(bindings or [])
        table = (abi.PTLightmapBinding * max(len(bindings), 1))(*[b["record"] for b in bindings])
        with self._ordered(torch.device(f"cuda:{self.device}")):
            plugin.check(self.lib.PTBindLightmaps(self.ctx, table if bindings else None, len(bindings)))
        self._lightmaps = bindings

    @property
    def lightmaps(self):
        """the entries last bound through bind_lightmaps"""
        return list(getattr(self, "_lightmaps", []))

    def lightmap_lookup(self, rays, hits, surfaces):
        """PTLightmapLookup: what the bound lightmaps hold at the first hits of trace_rays(rays, surface=True).  Returns
        (irradiance (n, 4) float32, binding (n,)): rgb and 0 where a lightmap was found, with the index of its binding; zero bits and
        PT_LIGHTMAP_NONE elsewhere.  plugin.lightmap_lookup is its twin.  numpy in, numpy out (the index as uint32); device tensors
        in, device tensors out (the index as int32, PT_LIGHTMAP_NONE reading -1)."""
        import torch
        r, as_numpy = self._to_device(rays, 8)
        h, _ = self._to_device(hits, 4)
        s, _ = self._to_device(surfaces, 12)
        n = r.shape[0]
        assert h.shape[0] == n and s.shape[0] == n, (r.shape, h.shape, s.shape)
        out = torch.empty((n, 4), dtype=torch.float32, device=r.device)
        which = torch.empty((n,), dtype=torch.int32, device=r.device)
        if n:
            with self._ordered(r.device):
                plugin.check(self.lib.PTLightmapLookup(self.ctx, r.data_ptr(), h.data_ptr(), s.data_ptr(), n, out.data_ptr(), which.data_ptr()))
        return (out.cpu().numpy(), which.cpu().numpy().view(np.uint32)) if as_numpy else (out, which)

    def shade_lightmapped(self, rays, hits, surfaces, volume, reflections=None, dfg=None, **options):
        """PTShadeLightmapped: shade_baked, but a hit inside a bound lightmap's span reads its irradiance from the lightmap (four
        texels) instead of the probe volume; every other hit falls back to the volume.  Arguments, options and result as
        shade_baked's; with nothing bound the two are equal bit for bit."""
        import torch
        r, as_numpy = self._to_device(rays, 8)
        h, _ = self._to_device(hits, 4)
        sf, _ = self._to_device(surfaces, 12)
        n = r.shape[0]
        assert h.shape[0] == n and sf.shape[0] == n, (r.shape, h.shape, sf.shape)
        s, keep = self._shade_inputs(volume, reflections, dfg, **options)
        out = torch.empty((n, 4), dtype=torch.float32, device=r.device)
        if n:
            with self._ordered(r.device):
                plugin.check(self.lib.PTShadeLightmapped(self.ctx, C.byref(s), r.data_ptr(), h.data_ptr(), sf.data_ptr(), n, out.data_ptr()))
        del keep
        return out.cpu().numpy() if as_numpy else out

    def render_lightmapped(self, params: abi.PTFrameParams, volume, reflections=None, dfg=None, return_rays: bool = False, **options):
        """PTShadeLightmappedFrame: render_baked with the bound lightmaps as the diffuse source of the surfaces they cover: static
        surfaces read their lightmap, everything else the probe volume.  Arguments and result as render_baked's."""
        import torch
        p = params or self.params(seed=0)
        dev = torch.device(f"cuda:{self.device}")
        s, keep = self._shade_inputs(volume, reflections, dfg, **options)
        w, h = int(p.OutputWidth), int(p.OutputHeight)
        out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
        rays = torch.empty((h * w, 8), dtype=torch.float32, device=dev) if return_rays else None
        with self._ordered(dev):
            plugin.check(self.lib.PTShadeLightmappedFrame(self.ctx, C.byref(p), C.byref(s), out.data_ptr(), rays.data_ptr() if return_rays else None))
        del keep
        return (out, rays) if return_rays else out

    # ---- probe placement (include/ptmi_plugin.h Part 18)
    def place_probes(self, positions, spacing, spp: int = 64, iterations: int = 4, max_distance: float = None, min_front_distance: float = None,
                     backface_share: float = 0.25, max_offset: float = 0.45, first_sample: int = 0, seeds=None, start=None, stats: bool = False):
        """PTProbePlace: move the probes of a grid out of geometry and mark the buried ones, before the bake.  Each of the
        `iterations` relocation steps traces `spp` closest-hit rays with surface records from every probe (probe_sh()'s directions),
        counts the faces seen from behind, and moves a probe through the nearest such face when more than `backface_share` of its
        samples see one (it is inside an object), or straight away from a face nearer than `min_front_distance`; a move that would
        take the probe further than `max_offset` x spacing from its grid position on an axis is refused.  One more trace classifies
        the final positions.

        positions: (n, 3) float32; spacing: the grid's, one number or three; seeds: (n,) uint32, None = the probe index.
        Defaults: max_distance = the spacing's diagonal, min_front_distance = 0.2 x the smallest spacing.
        start: (n, 3) offsets to start from (PT_PLACE_KEEP_OFFSETS: placing again after a geometry update), None = zeros.
          numpy array -> PTProbePlaceHost, returns numpy;
          torch tensor on this context's device -> PTProbePlace zero-copy, ordered against torch's current stream both ways.
        Returns (offsets (n, 3) float32, states (n,): 0 live, abi.PT_PROBE_INSIDE buried -- uint32 in numpy, int32 on the device),
        and with stats=True also the (n,) numpy records of abi.PLACE_STATS_DTYPE that describe the final positions."""
        q = abi.probe_place_params(spacing, max_distance, min_front_distance, backface_share, max_offset, iterations)
        rows = self._probes(positions, seeds)
        n = rows.shape[0]
        flags = 0 if start is None else abi.PT_PLACE_KEEP_OFFSETS
        if isinstance(rows, np.ndarray):
            out = plugin.probe_placement_rows(start, None, n)
            assert out.shape[0] == n, (out.shape, n)
            st = np.zeros(n, abi.PLACE_STATS_DTYPE)
            plugin.check(self.lib.PTProbePlaceHost(self.ctx, rows.ctypes.data, n, first_sample & 0xFFFFFFFF, spp, C.byref(q), flags, out.ctypes.data,
                                                   st.ctypes.data if stats else None))
            res = (out[:, 0:3].copy(), out[:, 3].copy().view(np.uint32))
            return res + (st,) if stats else res
        import torch
        out = torch.zeros((n, 4), dtype=torch.float32, device=rows.device)
        if start is not None:
            out[:, 0:3] = torch.as_tensor(start, dtype=torch.float32, device=rows.device).reshape(n, 3)
        d_st = torch.zeros((n, 8), dtype=torch.int32, device=rows.device) if stats else None
        with self._ordered(rows.device):
            plugin.check(self.lib.PTProbePlace(self.ctx, rows.data_ptr(), n, first_sample & 0xFFFFFFFF, spp, C.byref(q), flags, out.data_ptr(),
                                               d_st.data_ptr() if stats else None))
        res = (out[:, 0:3], out.view(torch.int32)[:, 3])
        return res + (d_st.cpu().numpy().view(abi.PLACE_STATS_DTYPE).reshape(n),) if stats else res

    def bake_probe_volume(self, lo, hi, counts, spp: int = 256, depth_spp: int = 256, max_distance: float = None, first_sample: int = 0, seeds=None,
                          delta_lights: bool = True, params: abi.PTFrameParams = None, relocate=None) -> "ProbeVolume":
        """A probe volume over the box lo ... hi: counts = (nx, ny, nz) probes, the outer ones on the box's faces (a count of 1 sits
        in the middle of its axis).  Bakes probe_sh(spp) and probe_depth(depth_spp) at plugin.probe_grid_positions of the grid; both
        stay on the device.  max_distance: where a depth ray ends, default 1.5 x the diagonal of a cell.
        relocate: None or False -- the probes stay on the grid; True, or a dict of place_probes() arguments -- place_probes() runs
        first (the grid's spacing, first_sample and seeds), both bakes are made at position + offset (one float32 add per component,
        on the host), and the placement stays on the device for the lookup (ProbeVolume.placement).  Returns a ProbeVolume."""
        import torch
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        counts = [int(c) for c in counts]
        assert len(counts) == 3 and min(counts) >= 1 and (hi >= lo).all(), (counts, lo, hi)
        origin = [lo[a] if counts[a] > 1 else 0.5 * (lo[a] + hi[a]) for a in range(3)]
        spacing = [(hi[a] - lo[a]) / (counts[a] - 1) if counts[a] > 1 else (hi[a] - lo[a] if hi[a] > lo[a] else 1.0) for a in range(3)]
        grid = plugin.probe_grid_desc(origin, spacing, counts)
        if max_distance is None:
            max_distance = 1.5 * float(np.linalg.norm([grid.spacing[a] for a in range(3)]))
        dev = torch.device(f"cuda:{self.device}")
        h_pos = plugin.probe_grid_positions(grid)
        pos = torch.from_numpy(h_pos).to(dev)
        d_seeds = None if seeds is None else torch.from_numpy(np.asarray(seeds).astype(np.int64)).to(dev)
        placement = None
        if relocate is not None and relocate is not False:
            args = dict(first_sample=first_sample)
            args.update({} if relocate is True else dict(relocate))
            offsets, states = self.place_probes(pos, [grid.spacing[a] for a in range(3)], seeds=d_seeds, **args)[:2]
            placement = torch.zeros((pos.shape[0], 4), dtype=torch.float32, device=dev)
            placement[:, 0:3] = offsets
            placement.view(torch.int32)[:, 3] = states
            pos = torch.from_numpy((h_pos + offsets.cpu().numpy()).astype(np.float32)).to(dev)
        sh, m2 = self.probe_sh(pos, spp=spp, first_sample=first_sample, seeds=d_seeds, delta_lights=delta_lights, params=params)
        depth = self.probe_depth(pos, spp=depth_spp, max_distance=max_distance, first_sample=first_sample, seeds=d_seeds)
        return ProbeVolume(self, grid, sh, m2, depth, max_distance, placement)

    # ---- lightmap charts (include/ptmi_plugin.h Part 14)
    def _chart_desc(self, width, height, mesh, instance, seed) -> abi.PTChartDesc:
        bvh = self._bvhScene
        off = self._blas_offsets(mesh)
        if bvh.gpu_instances is None:
            assert instance in (None, -1), "a flat scene has no instances"
            inst = -1
        elif instance is None:
            inst = [i for i, rec in enumerate(self.scene.instances) if rec[0] == mesh][0]      # the mesh's first instance
        else:
            inst = int(instance)
        return abi.chart_desc(width, height, bvh.blas_spans[0 if mesh is None else mesh][3], off, inst, seed)

    def chart_receivers(self, width: int, height: int, mesh: int = None, instance: int = None, uvs=None, seed: int = 0):
        """PTRasterizeChart: the lightmap receivers of one mesh, made on the GPU from the scene's CURRENT geometry (after any
        update_geometry / skin_geometry / morph_geometry).  One receiver per texel of the width x height atlas whose centre the
        mesh's UV chart covers; where triangles overlap in UV space the one with the lowest primitive index owns the texel.

        mesh names the BLAS as update_geometry does (None on a flat scene).  HAS_TLAS: `instance` picks whose transform places the
        receivers (default: the mesh's first instance; -1: the mesh's local space).  uvs: (T, 6) float32 lightmap UVs per primitive
        (u0 v0 u1 v1 u2 v2; numpy, or a float32 tensor on this context's device), None = the attribute records' uv0 .. uv2; a
        triangle with a NaN UV is left out.  seed: receiver i gets seed + its texel index.
        Returns (texels, receivers): device tensors, (n,) int32 holding the texel indices y * width + x in ascending order (all
        < 2^26), and (n, 8) float32 PTReceiver rows that irradiance() takes as `receivers=`.  Synchronises (the count is read back).
        Several meshes in one atlas are the caller's business: concatenate the lists of several calls (torch.cat) and resolve once;
        texels two meshes both cover then appear twice, and resolve_lightmap writes one of them."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        d = self._chart_desc(width, height, mesh, instance, seed)
        d_uvs = None
        if uvs is not None:
            d_uvs = uvs if isinstance(uvs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(uvs, dtype=np.float32)).to(dev)
            assert d_uvs.dtype == torch.float32 and d_uvs.is_contiguous() and d_uvs.numel() == d.triangleCount * 6 and d_uvs.device == dev, (d_uvs.shape, d_uvs.dtype)
        with self._ordered(dev):
            count = C.c_uint64()
            uv_ptr = None if d_uvs is None else d_uvs.data_ptr()
            # a small atlas: arrays for every texel, one call; a large one: count first
            cap = int(width) * int(height)
            if not (0 < cap <= 1 << 22):
                plugin.check(self.lib.PTRasterizeChart(self.ctx, C.byref(d), uv_ptr, None, None, 0, C.byref(count)))
                cap = count.value
            texels = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev)
            recv = torch.empty((max(cap, 1), 8), dtype=torch.float32, device=dev)
            plugin.check(self.lib.PTRasterizeChart(self.ctx, C.byref(d), uv_ptr, texels.data_ptr(), recv.data_ptr(), cap, C.byref(count)))
        return texels[:count.value], recv[:count.value]

    def resolve_lightmap(self, texels, irradiance, width: int, height: int, dilate: int = 2):
        """PTResolveLightmap: scatter gathered irradiance back into an atlas and dilate the chart borders, on the GPU.  texels: (n,)
        int32 / uint32 device tensor of unique texel indices (chart_receivers'), irradiance: (n, 4) float32 device tensor
        (irradiance()'s).  Returns an (height, width, 4) float32 device tensor: rgb, and w = 1 on the list's texels, 0.5 on texels a
        dilation pass filled (the mean of the filled ones among the 8 neighbours), 0 elsewhere.  dilate: 0 ... 16 passes."""
        import torch
        assert texels.element_size() == 4 and texels.dim() == 1 and texels.is_contiguous(), (texels.dtype, texels.shape)
        assert irradiance.dtype == torch.float32 and irradiance.is_contiguous() and irradiance.shape == (texels.shape[0], 4), irradiance.shape
        dev = texels.device
        n = texels.shape[0]
        image = torch.empty((max(int(height), 1), max(int(width), 1), 4), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(self.lib.PTResolveLightmap(self.ctx, texels.data_ptr() if n else None, irradiance.data_ptr() if n else None, n, int(width), int(height),
                                                    int(dilate), image.data_ptr()))
        return image

    def denoise_lightmap(self, texels, receivers, irradiance, width: int, height: int, samples: int, iterations: int = 5, params=None):
        """PTDenoiseLightmap: a chart-aware a-trous filter over a gathered list, in texel space, on the GPU (Part 17 has the rule).
        texels: (n,) int32 / uint32 device tensor of unique texel indices and receivers: (n, 8) float32 PTReceiver rows
        (chart_receivers'), irradiance: (n, 4) float32 (irradiance()'s, of `samples` samples per texel, 2 or more).  iterations:
        0 ... 8 levels; params: a dict of abi.lightmap_denoise_params' keywords (sigma_luminance, sigma_position, sigma_plane,
        normal_power, iterations) or a PTLightmapDenoiseParams.  Returns an (n, 4) float32 device tensor that resolve_lightmap
        takes: the filtered rgb, and in m2's place the variance estimate of the filtered luminance.  Texels that touch in the atlas
        but not in the world do not mix.  Ordered against torch's current stream both ways."""
        import torch
        assert texels.element_size() == 4 and texels.dim() == 1 and texels.is_contiguous(), (texels.dtype, texels.shape)
        n = texels.shape[0]
        assert receivers.dtype == torch.float32 and receivers.is_contiguous() and receivers.shape == (n, 8), receivers.shape
        assert irradiance.dtype == torch.float32 and irradiance.is_contiguous() and irradiance.shape == (n, 4), irradiance.shape
        p = plugin.lightmap_denoise_params(samples, iterations, params)
        dev = texels.device
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(self.lib.PTDenoiseLightmap(self.ctx, C.byref(p), texels.data_ptr() if n else None, receivers.data_ptr() if n else None,
                                                    irradiance.data_ptr() if n else None, n, int(width), int(height), out.data_ptr() if n else None))
        return out

    def bake_lightmap(self, width: int, height: int, spp: int = 64, mesh: int = None, instance: int = None, uvs=None, dilate: int = 2, seed: int = 0,
                      first_sample: int = 0, params: abi.PTFrameParams = None, as_tensor: bool = False, denoise=None, adaptive=None,
                      return_counts: bool = False):
        """A lightmap of one mesh: chart_receivers, PTGatherIrradiance over them, resolve_lightmap -- nothing but the final image
        leaves the device.  spp, first_sample and params are irradiance()'s (samples [first_sample, first_sample + spp) of every
        texel; the gathered lists of two bakes over disjoint ranges fold by plugin.fold_irradiance), the rest chart_receivers' and
        resolve_lightmap's.
        denoise: None, or what denoise_lightmap runs between the gather and the resolve: a number of levels, or a dict of its parameters.
        adaptive: None, or what replaces the gather by irradiance_adaptive(): a number (the threshold) or a dict of its keywords
        (threshold, min_samples, add_samples, max_samples, dark_floor); spp is then max_samples unless the dict says otherwise.  With
        denoise also given, the list is equalised to max_samples (equalise_irradiance) and the denoiser runs with samples = max_samples.
        return_counts: also a (height, width) int32 image of the samples every texel got (spp without adaptive), 0 outside the chart.
        Returns (height, width, 4) float32 -- numpy, or with as_tensor a device tensor; w tells baked (1), dilated (0.5), empty (0)."""
        import torch
        texels, recv = self.chart_receivers(width, height, mesh=mesh, instance=instance, uvs=uvs, seed=seed)
        counts = None
        if adaptive is not None:
            kw = dict(adaptive) if isinstance(adaptive, dict) else {"threshold": float(adaptive)}
            kw.setdefault("max_samples", spp)
            spp = int(kw["max_samples"])
        if not recv.shape[0]:                                       # a chart that covers nothing: an empty image
            irr = recv.new_empty((0, 4))
        elif adaptive is None:
            irr = self.irradiance(receivers=recv, spp=spp, first_sample=first_sample, params=params)
        else:
            irr, counts, _ = self.irradiance_adaptive(receivers=recv, first_sample=first_sample, params=params, **kw)
            if denoise is not None:
                irr = self.equalise_irradiance(irr, counts, spp)
        if denoise is not None and recv.shape[0]:
            irr = self.denoise_lightmap(texels, recv, irr, width, height, spp, params=plugin.lightmap_denoise_params(spp, 5, denoise))
        image = self.resolve_lightmap(texels, irr, width, height, dilate=dilate)
        image = image if as_tensor else image.cpu().numpy()
        if not return_counts:
            return image
        count_image = torch.zeros((max(int(height), 1) * max(int(width), 1),), dtype=torch.int32, device=texels.device)
        if recv.shape[0]:
            count_image[texels.long()] = counts.to(torch.int32) if counts is not None else torch.full_like(texels, spp, dtype=torch.int32)
        count_image = count_image.reshape(max(int(height), 1), max(int(width), 1))
        return image, (count_image if as_tensor else count_image.cpu().numpy())

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

    # ---- guides and denoising (include/ptmi_plugin.h Part 4)
    def render_guides(self, samples: int = 1, params: abi.PTFrameParams = None):
        """PTRenderGuides: first-hit albedo / normal / depth guides for the camera of `params` (default: this tracer's),
        `samples` = 1, 4 or 16 sub-pixel rays per pixel.  Stream-ordered; guides() reads them back."""
        p = params or self.params(seed=0)
        plugin.check(self.lib.PTRenderGuides(self.ctx, C.byref(p), samples))
        self._guide_size = (p.OutputHeight, p.OutputWidth)

    def guide_pointer(self, which: int) -> int:
        """Device pointer of guide 0 (albedo + coverage) or 1 (normal + depth); 0 before render_guides."""
        return self.lib.PTGetGuidePointer(self.ctx, which) or 0

    def guides(self):
        """The guides as numpy arrays: albedo (H, W, 4) = base colour rgb + coverage, normal+depth (H, W, 4)."""
        h, w = self._guide_size
        self.synchronize()
        out = []
        for which in (0, 1):
            ptr = self.guide_pointer(which)
            if not ptr:
                raise RuntimeError("render_guides() has not been called")
            out.append(_device_to_numpy(ptr, (h, w, 4)))
        return out[0], out[1]

    def denoise(self, dp: abi.PTDenoiseParams = None, d_src: int = 0, d_dst: int = 0, variance: str = "spatial"):
        """PTDenoise with `dp` (default abi.denoise_params()).  d_src = 0 reads the current Output frame.  With d_dst = 0 the
        result comes back as (H, W, 4) float32 numpy (PTDenoiseToHost when d_src is 0 too); else it is written to d_dst.
        variance: "spatial" = PTDenoise (the 3x3 luminance variance); "moments" = PTDenoiseMoments (the variance of the mean
        from the tracked passes; d_src = 0 then reads the frame last accumulated); "auto" = the moments from 4 observations
        on, else spatial (SVGF's fallback rule)."""
        if variance not in ("spatial", "moments", "auto"):
            raise ValueError(f"variance = {variance!r}")
        if variance == "auto":
            variance = "moments" if self.moments_info()[0] >= 4 else "spatial"
        fn, fn_host = ((self.lib.PTDenoiseMoments, self.lib.PTDenoiseMomentsToHost) if variance == "moments"
                       else (self.lib.PTDenoise, self.lib.PTDenoiseToHost))
        dp = dp or abi.denoise_params()
        if d_dst:
            plugin.check(fn(self.ctx, C.byref(dp), C.c_void_p(d_src) if d_src else None, C.c_void_p(d_dst)))
            return None
        h, w = self._guide_size
        out = np.empty((h, w, 4), dtype=np.float32)
        if not d_src:
            plugin.check(fn_host(self.ctx, C.byref(dp), out.ctypes.data_as(C.c_void_p), out.size))
            return out
        import torch
        dst = torch.empty((h, w, 4), dtype=torch.float32, device=f"cuda:{self.device}")
        torch.cuda.synchronize(dst.device)
        plugin.check(fn(self.ctx, C.byref(dp), C.c_void_p(d_src), C.c_void_p(dst.data_ptr())))
        self.synchronize()
        return dst.cpu().numpy()

    # ---- variance across passes (include/ptmi_plugin.h Part 6)
    def accumulate_moments(self, p: abi.PTFrameParams, count: int = 1, d_output: int = 0, d_accumulated: int = 0):
        """PTAccumulateMoments: record the `count` passes just enqueued with `p` as one observation -- over the internal frames
        (call it before flip()), or over caller-owned device frames when d_output is given (PTAccumulateMomentsTo)."""
        if d_output:
            plugin.check(self.lib.PTAccumulateMomentsTo(self.ctx, C.byref(p), count, C.c_void_p(d_output), C.c_void_p(d_accumulated or None)))
        else:
            plugin.check(self.lib.PTAccumulateMoments(self.ctx, C.byref(p), count))

    def moments_info(self):
        """(observations, samples, width, height) of the moments; zeros before the first accumulation."""
        k, w, h, n = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        plugin.check(self.lib.PTGetMomentsInfo(self.ctx, C.byref(k), C.byref(n), C.byref(w), C.byref(h)))
        return k.value, n.value, w.value, h.value

    def moments_pointer(self, which: int) -> int:
        return self.lib.PTGetMomentsPointer(self.ctx, which) or 0

    def moments(self):
        """The two moment planes as (H, W, 4) float32 numpy arrays: (Srr, Sgg, Sbb, Sll) and (Srg, Srb, Sgb, 0)."""
        _, _, w, h = self.moments_info()
        if not w:
            raise RuntimeError("nothing accumulated yet")
        self.synchronize()
        return tuple(_device_to_numpy(self.moments_pointer(k), (h, w, 4)) for k in (0, 1))

    def noise(self, threshold: float = 0.02, percentile: float = 0.95, rel_floor: float = 0.01, d_frame: int = 0) -> abi.PTNoiseStats:
        """PTMeasureNoise over the frame last accumulated (or d_frame): the statistics of the per-pixel relative standard
        error of the mean.  Synchronous."""
        st = abi.noise_stats()
        q = abi.noise_params(rel_floor, threshold, percentile)
        plugin.check(self.lib.PTMeasureNoise(self.ctx, C.byref(q), C.c_void_p(d_frame) if d_frame else None, C.byref(st)))
        return st

    def noise_tiles(self) -> np.ndarray:
        """The mean error of every 16x16 block after noise(): (ceil(H/16), ceil(W/16)) float32, 0 for other ranks' blocks."""
        ptr = self.lib.PTGetNoiseTilePointer(self.ctx)
        if not ptr:
            raise RuntimeError("noise() has not been called")
        _, _, w, h = self.moments_info()
        return _device_to_numpy(ptr, ((h + 15) // 16, (w + 15) // 16))

    def render_until(self, noise: float, percentile: float = 0.95, max_samples: int = None, seed0: int = 0, check_every: int = 4):
        """Reset(), then OnRenderImage(seed0 + k) with every pass tracked, until a check -- every `check_every` passes -- finds
        the `percentile` of the relative error below `noise`, or `max_samples` (default maxSamples) are reached.  The frame is
        the one the same number of plain OnRenderImage calls gives.  Returns (passes rendered, the last PTNoiseStats or None)."""
        limit = min(self.maxSamples, max_samples if max_samples is not None else self.maxSamples)
        was, self.track_noise = self.track_noise, True
        st, k = None, 0
        try:
            self.Reset()
            while self._currentSample < limit:
                self.OnRenderImage(seed0 + k)
                k += 1
                if k >= 2 and k % max(1, check_every) == 0:
                    st = self.noise(threshold=noise, percentile=percentile)
                    if st.percentileError < noise:
                        break
        finally:
            self.track_noise = was
        return k, st

    # ---- adaptive sampling (include/ptmi_plugin.h Part 7)
    def block_grid(self):
        """(rows, columns) of the frame's 16x16 blocks; block id = row * columns + column."""
        return (self.height + 15) // 16, (self.width + 15) // 16

    def adaptive_begin(self, current_sample: int = None):
        """PTAdaptiveBegin: every block holds `current_sample` samples (default: what OnRenderImage has accumulated); all active."""
        n = self._currentSample if current_sample is None else current_sample
        p = self.params(seed=0)
        plugin.check(self.lib.PTAdaptiveBegin(self.ctx, C.byref(p), n))

    def adaptive_end(self):
        plugin.check(self.lib.PTAdaptiveEnd(self.ctx))

    def set_active_blocks(self, ids=None) -> int:
        """PTSetActiveBlocks: strictly ascending block ids (None = every block, an empty sequence = none).  Returns how many
        this context keeps (its own blocks with a covered pixel)."""
        kept = C.c_uint32()
        if ids is None:
            plugin.check(self.lib.PTSetActiveBlocks(self.ctx, None, 0, C.byref(kept)))
        else:
            a = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            buf = (C.c_uint32 * max(1, a.size))(*a.tolist())
            plugin.check(self.lib.PTSetActiveBlocks(self.ctx, buf, a.size, C.byref(kept)))
        return kept.value

    def select_active_blocks(self, threshold: float, max_samples: int, add_samples: int, dilate: bool = True) -> int:
        """PTSelectActiveBlocks after noise(): the blocks whose mean error exceeds `threshold` and that may still take
        `add_samples` within `max_samples` (with dilate: and their neighbours).  Returns how many are active."""
        kept = C.c_uint32()
        sel = abi.adaptive_select(threshold, max_samples, add_samples, dilate)
        plugin.check(self.lib.PTSelectActiveBlocks(self.ctx, C.byref(sel), C.byref(kept)))
        return kept.value

    def active_blocks(self) -> np.ndarray:
        """The block ids the next render_active renders, ascending (uint32)."""
        n = C.c_uint32()
        plugin.check(self.lib.PTGetActiveBlocks(self.ctx, None, 0, C.byref(n)))
        buf = (C.c_uint32 * max(1, n.value))()
        plugin.check(self.lib.PTGetActiveBlocks(self.ctx, buf, n.value, C.byref(n)))
        return np.array(buf[:n.value], dtype=np.uint32)

    def block_samples(self) -> np.ndarray:
        """PTGetBlockSamples: the sample count of every block, (ceil(H/16), ceil(W/16)) uint32."""
        rows, cols = self.block_grid()
        out = np.empty((rows, cols), np.uint32)
        plugin.check(self.lib.PTGetBlockSamples(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out

    def _active_params(self, seeds):
        ps = []
        for s in seeds:
            p = self.params(seed=s)
            p.CurrentSample = 0          # not read: every block renders with its own count
            ps.append(p)
        return (abi.PTFrameParams * len(ps))(*ps)

    def render_active(self, seeds, d_output: int = 0, d_accumulated: int = 0):
        """PTRenderPassActive: len(seeds) passes (1..8, RngSeedRoot = seeds[j]) over the active blocks, into the internal
        ping-pong frames, or into caller-owned device frames when d_output is given (PTRenderPassActiveTo)."""
        arr = self._active_params(seeds)
        if d_output:
            plugin.check(self.lib.PTRenderPassActiveTo(self.ctx, arr, len(arr), C.c_void_p(d_output), C.c_void_p(d_accumulated or None)))
        else:
            plugin.check(self.lib.PTRenderPassActive(self.ctx, arr, len(arr)))

    def accumulate_moments_active(self, count: int, d_output: int = 0, d_accumulated: int = 0):
        """PTAccumulateMomentsActive: one observation for the blocks of the render_active call just enqueued (count = its
        number of passes); call it before flip()."""
        p = self._active_params([0])[0]
        if d_output:
            plugin.check(self.lib.PTAccumulateMomentsActiveTo(self.ctx, C.byref(p), count, C.c_void_p(d_output), C.c_void_p(d_accumulated or None)))
        else:
            plugin.check(self.lib.PTAccumulateMomentsActive(self.ctx, C.byref(p), count))

    def render_adaptive(self, noise: float, min_samples: int, max_samples: int, seed0: int = 0, passes_per_round: int = 4,
                        dilate: bool = True, history: list = None):
        """Reset(); tracked OnRenderImage(seed0 + k) until at least 4 observations and `min_samples`; then rounds of: noise(),
        select the blocks whose mean error exceeds `noise` (and that stay within `max_samples`), one render_active batch of
        `passes_per_round` passes with the next seeds, accumulate_moments_active, flip -- until nothing is selected.
        Afterwards readback() returns the frame (the last output, already flipped) and denoise(variance="moments") works on it.
        history (optional list) receives ("uniform", seed) and ("active", ids, seeds) records in order.
        Returns (block_samples, the last PTNoiseStats)."""
        spp = max(1, self.samplesPerPass)
        was, self.track_noise = self.track_noise, True
        try:
            self.adaptive_end()
            self.Reset()
            k = 0
            while k < 4 or self._currentSample < min_samples:
                self.OnRenderImage(seed0 + k)
                if history is not None:
                    history.append(("uniform", seed0 + k))
                k += 1
        finally:
            self.track_noise = was
        self.adaptive_begin()
        add = spp * passes_per_round
        while True:
            st = self.noise(threshold=noise)
            if self.select_active_blocks(noise, max_samples, add, dilate) == 0:
                break
            seeds = [seed0 + k + j for j in range(passes_per_round)]
            k += passes_per_round
            if history is not None:
                history.append(("active", self.active_blocks(), seeds))
            self.render_active(seeds)
            self.accumulate_moments_active(passes_per_round)
            self.flip()
            self._flipped = True
        return self.block_samples(), st

    # ---- scene updates (include/ptmi_plugin.h Part 5)
    def set_instance_transforms(self, local_to_world) -> bool:
        """Move the instances (one 4x4 localToWorld each): BVHScene.UpdateTLAS, then Reset() when anything changed, as the
        reference's frame loop does (PathTracer.cs:169-183).  Returns whether anything changed."""
        changed = self._bvhScene.UpdateTLAS(self.ctx, local_to_world)
        if changed:
            self.Reset()
        return changed

    def update_instances_device(self, records):
        """PTUpdateInstancesDevice from a torch tensor on this context's device holding instanceCount PTBlasInstance records
        (192 bytes each, e.g. uint8 (n, 192) or float32 (n, 48)).  Ordered after torch's current stream; torch's later work
        is ordered after the update.  Does not reset accumulation."""
        import torch
        assert records.is_contiguous() and records.numel() * records.element_size() % 192 == 0
        n = records.numel() * records.element_size() // 192
        dev = records.device
        with self._ordered(dev):
            plugin.check(self.lib.PTUpdateInstancesDevice(self.ctx, records.data_ptr(), n))

    def update_lights(self, lights: np.ndarray):
        """PTUpdateLights: (k, 16) float32 PTLight records, 1 <= k <= the scene's light count."""
        L = np.ascontiguousarray(lights, dtype=np.float32).reshape(-1, 16)
        plugin.check(self.lib.PTUpdateLights(self.ctx, L.ctypes.data, L.shape[0]))

    def update_materials(self, materials: np.ndarray):
        """PTUpdateMaterials: (materialCount, 32) float32 PTMaterialData records."""
        M = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 32)
        plugin.check(self.lib.PTUpdateMaterials(self.ctx, M.ctypes.data, M.shape[0]))

    def read_tlas(self):
        """PTReadTLAS: the current TLAS as plugin.build_tlas returns it -> (node bytes uint8[], indices uint32[])."""
        n = self._bvhScene.gpu_instances.shape[0]
        nodes = np.empty((2 * n - 1) * 64, np.uint8)
        idx = np.empty(n, np.uint32)
        count = C.c_uint32()
        plugin.check(self.lib.PTReadTLAS(self.ctx, nodes.ctypes.data, nodes.nbytes, idx.ctypes.data, n, C.byref(count)))
        return nodes[:count.value * 64].copy(), idx

    # ---- geometry updates (include/ptmi_plugin.h Part 9)
    def _blas_offsets(self, mesh):
        bvh = self._bvhScene
        if bvh.gpu_instances is None:
            return (0, 0, 0)
        assert mesh is not None, "a HAS_TLAS scene needs the mesh index"
        users = [i for i, inst in enumerate(self.scene.instances) if inst[0] == mesh]
        if not users:
            raise ValueError(f"mesh {mesh} has no instance in the scene: its BLAS cannot be named")
        return tuple(int(bvh.gpu_instances[users[0]][f]) for f in ("bvhOffset", "triOffset", "triAttributeOffset"))

    def _built_cost(self, mesh):
        """sahCost after the BLAS's last build or rebuild; the tree as built is measured on the host from the arrays PTSetScene was given"""
        if mesh not in self._builtCost:
            bvh = self._bvhScene
            n0, cap, t0, nt = bvh.blas_spans[0 if mesh is None else mesh]
            self._builtCost[mesh] = plugin.measure_cwbvh((bvh.bvh_nodes[n0 * 80:(n0 + cap) * 80], bvh.bvh_tris[t0 * 16:t0 * 16 + nt * 48]), nt)["sahCost"]
        return self._builtCost[mesh]

    def rebuild_geometry(self, vertices, mesh: int = None, tri_attrs=None):
        """PTRebuildGeometry / PTRebuildGeometryDevice: update_geometry's contract, but the BLAS gets a new tree (the device
        builder's, built in place on the GPU) instead of a refit.  The tree must fit the BLAS's node span (node_capacity)."""
        self.update_geometry(vertices, mesh=mesh, tri_attrs=tri_attrs, _rebuild=True)
        self._builtCost[mesh] = self.geometry_quality(mesh)["sahCost"]

    def geometry_quality(self, mesh: int = None) -> dict:
        """PTMeasureGeometry: nodeCapacity, nodeCount, triangleCount, levels, rootHalfArea and sahCost of the BLAS's current tree.
        Synchronising."""
        q = abi.geometry_quality()
        plugin.check(self.lib.PTMeasureGeometry(self.ctx, *self._blas_offsets(mesh), C.byref(q)))
        return q.as_dict()

    def update_geometry(self, vertices, mesh: int = None, tri_attrs=None, rebuild_above: float = None, _rebuild: bool = False):
        """PTUpdateGeometry: new positions for one BLAS, refitted in place on the GPU.  vertices: (3 * triangles, 4) float32 in
        the BLAS's primitive order (numpy), or a torch tensor on this context's device (PTUpdateGeometryDevice, ordered after
        torch's current stream; tri_attrs then is a device tensor too).  tri_attrs (optional): the BLAS's abi.TRI_ATTR records.
        Flat scene: mesh stays None.  HAS_TLAS scene: mesh indexes scene.mesh_ranges; the vertices are in the mesh's local space,
        and the world bounds of the mesh's instances are recomputed (scenes.instance_world_bounds) and sent through
        PTUpdateInstances -- the library does not touch the TLAS (with device tensors that is left to the caller).  Does not
        reset accumulation.
        rebuild_above (a ratio, no default): the refit is followed by PTMeasureGeometry; if sahCost exceeds rebuild_above x the cost
        recorded after the BLAS's last build or rebuild, the same vertices go through PTRebuildGeometry.  Returns "refit" or
        "rebuild" then, None otherwise."""
        bvh = self._bvhScene
        off = self._blas_offsets(mesh)
        if rebuild_above is not None:
            self.update_geometry(vertices, mesh=mesh, tri_attrs=tri_attrs)
            if self.geometry_quality(mesh)["sahCost"] <= rebuild_above * self._built_cost(mesh):
                return "refit"
            self.rebuild_geometry(vertices, mesh=mesh)         # the attributes were replaced by the refit above
            return "rebuild"
        fn_host, fn_device = (self.lib.PTRebuildGeometry, self.lib.PTRebuildGeometryDevice) if _rebuild else (self.lib.PTUpdateGeometry, self.lib.PTUpdateGeometryDevice)
        if isinstance(vertices, np.ndarray):
            v = np.ascontiguousarray(vertices, dtype=np.float32)
            assert v.ndim == 2 and v.shape[1] == 4 and v.shape[0] % 3 == 0
            a = None if tri_attrs is None else np.ascontiguousarray(tri_attrs)
            assert a is None or a.nbytes == v.shape[0] // 3 * 128
            plugin.check(fn_host(self.ctx, *off, v.ctypes.data, v.shape[0] // 3, None if a is None else a.ctypes.data))
        else:
            import torch
            assert vertices.is_contiguous() and vertices.dtype == torch.float32 and vertices.numel() % 12 == 0
            assert tri_attrs is None or (tri_attrs.is_contiguous() and tri_attrs.numel() * tri_attrs.element_size() == vertices.numel() // 12 * 128)
            with self._ordered(vertices.device):
                plugin.check(fn_device(self.ctx, *off, vertices.data_ptr(), vertices.numel() // 12, None if tri_attrs is None else tri_attrs.data_ptr()))
            if bvh.gpu_instances is not None:
                import warnings
                warnings.warn("update_geometry with device tensors on a HAS_TLAS scene: resend the instances' world bounds "
                              "(PTUpdateInstances / update_instances_device), the vertices are not read back for them")
            v = None
        if v is None:
            return
        # later transform updates take the mesh's bounds from the scene's vertices: kept current in a copy of our own, made once
        if not getattr(self, "_ownVertices", False):
            from dataclasses import replace
            self.scene = bvh.scene = replace(self.scene, vertices=self.scene.vertices.copy())
            self._ownVertices = True
        t0 = 0 if mesh is None else self.scene.mesh_ranges[mesh][0]
        self.scene.vertices[t0 * 3:t0 * 3 + v.shape[0]] = v
        if bvh.gpu_instances is not None:
            from .scenes import instance_world_bounds
            for k, (m, _, _) in enumerate(self.scene.instances):
                if m != mesh:
                    continue
                l2w = bvh.gpu_instances[k]["localToWorld"].reshape(4, 4).T.astype(np.float64)
                bvh.blas_instances[k]["aabbMin"], bvh.blas_instances[k]["aabbMax"] = instance_world_bounds(v, l2w)
            plugin.check(self.lib.PTUpdateInstances(self.ctx, bvh.blas_instances.ctypes.data, bvh.blas_instances.shape[0]))

    # ---- skinned geometry (include/ptmi_plugin.h Part 11)
    def set_skin(self, rest_vertices, joints, weights, mesh: int = None, rest_attrs=None, joint_count: int = None):
        """PTSetSkin: the skin of one BLAS, uploaded once.  rest_vertices (3T, 4) float32 in the BLAS's primitive order
        (update_geometry's layout), joints (3T, 4) uint16, weights (3T, 4) float32, rest_attrs (optional) the BLAS's abi.TRI_ATTR
        records of the rest pose -- with them every skin_geometry also writes the skinned normals and tangents.  joint_count: the
        palette's length (default: the largest joint index + 1).  rest_vertices = None removes the BLAS's skin."""
        off = self._blas_offsets(mesh)
        nt = self._bvhScene.blas_spans[0 if mesh is None else mesh][3]
        if rest_vertices is None:
            plugin.check(self.lib.PTSetSkin(self.ctx, *off, nt, None))
            return
        if joint_count is None:
            joint_count = int(np.asarray(joints).max()) + 1
        d, ntri, keep = plugin.skin_desc(rest_vertices, joints, weights, joint_count, rest_attrs)
        plugin.check(self.lib.PTSetSkin(self.ctx, *off, ntri, C.byref(d)))

    def skin_geometry(self, joint_matrices, mesh: int = None, rebuild: bool = False, rebuild_above: float = None):
        """PTSkinGeometry: one joint palette in, the BLAS's vertices skinned on the GPU and refitted (rebuild=True: rebuilt, Part
        10's rules) in place -- no vertex is uploaded or read back.  joint_matrices: numpy (J, 3, 4) or (J, 12) (rest space to the
        mesh's local space: joint world x inverse bind), or a float32 torch tensor of that shape on this context's device
        (PTSkinGeometryDevice, ordered after torch's current stream).  Returns the skinned vertices' bounds, (2, 3) float32: min, max.
        HAS_TLAS scene: the world bounds of the mesh's instances are recomputed from those two corners
        (scenes.instance_world_bounds) and sent through PTUpdateInstances.  Does not reset accumulation.
        rebuild_above: update_geometry's policy -- refit, measure, and rebuild from the same palette if sahCost exceeds
        rebuild_above x the cost after the BLAS's last build or rebuild; returns (bounds, "refit" or "rebuild") then."""
        off = self._blas_offsets(mesh)
        if rebuild_above is not None:
            bounds = self.skin_geometry(joint_matrices, mesh=mesh)
            if self.geometry_quality(mesh)["sahCost"] <= rebuild_above * self._built_cost(mesh):
                return bounds, "refit"
            return self.skin_geometry(joint_matrices, mesh=mesh, rebuild=True), "rebuild"
        flags = abi.PT_SKIN_REBUILD if rebuild else 0
        out = (C.c_float * 6)()
        if isinstance(joint_matrices, np.ndarray):
            m = plugin.joint_palette(joint_matrices)
            plugin.check(self.lib.PTSkinGeometry(self.ctx, *off, m.ctypes.data, m.shape[0], flags, out))
        else:
            import torch
            m = joint_matrices
            assert m.is_contiguous() and m.dtype == torch.float32 and m.numel() % 12 == 0 and tuple(m.shape[1:]) in ((3, 4), (12,))
            with self._ordered(m.device):
                plugin.check(self.lib.PTSkinGeometryDevice(self.ctx, *off, m.data_ptr(), m.numel() // 12, flags, out))
        bounds = np.array(out, np.float32).reshape(2, 3)
        if rebuild:
            self._builtCost[mesh] = self.geometry_quality(mesh)["sahCost"]
        self._send_instance_bounds(mesh, bounds)
        return bounds

    # ---- morph targets (include/ptmi_plugin.h Part 12)
    def set_morph(self, rest_vertices, position_deltas, normal_deltas=None, tangent_deltas=None, mesh: int = None, rest_attrs=None,
                  target_count: int = None):
        """PTSetMorph: the morph targets of one BLAS, uploaded once.  rest_vertices (3T, 4) float32 in the BLAS's primitive order
        (update_geometry's layout).  Each deltas argument is a dense (K, 3T, 3) float32 array (converted by plugin.morph_csr: a corner
        lists a target unless its delta is exactly +0, +0, +0) or an (offsets, entries) CSR tuple; normal_deltas and tangent_deltas
        need rest_attrs, the BLAS's abi.TRI_ATTR records of the rest pose -- with rest_attrs every morph_geometry also writes the
        records.  target_count: default the dense array's K, or for a CSR position stream its largest target + 1.
        rest_vertices = None removes the BLAS's morph."""
        off = self._blas_offsets(mesh)
        nt = self._bvhScene.blas_spans[0 if mesh is None else mesh][3]
        if rest_vertices is None:
            plugin.check(self.lib.PTSetMorph(self.ctx, *off, nt, None))
            return
        if target_count is None:
            if isinstance(position_deltas, tuple):
                target_count = int(np.asarray(position_deltas[1])["target"].max()) + 1 if len(position_deltas[1]) else 1
            else:
                target_count = len(position_deltas)
        d, ntri, keep = plugin.morph_desc(rest_vertices, target_count, position_deltas, normal_deltas, tangent_deltas, rest_attrs)
        plugin.check(self.lib.PTSetMorph(self.ctx, *off, ntri, C.byref(d)))

    def morph_geometry(self, weights, joint_matrices=None, mesh: int = None, rebuild: bool = False, rebuild_above: float = None):
        """PTMorphGeometry: one weight per target in (and optionally skin_geometry's joint palette: morph first, then the skin), the
        BLAS's vertices made on the GPU and refitted (rebuild=True: rebuilt, Part 10's rules) in place -- no vertex is uploaded or
        read back.  weights: numpy (K,), joint_matrices numpy (J, 3, 4) or (J, 12) or None; or float32 torch tensors on this
        context's device (PTMorphGeometryDevice, ordered after torch's current stream; both on the device then).  Returns the
        vertices' bounds, (2, 3) float32: min, max.  HAS_TLAS scene: the world bounds of the mesh's instances are recomputed from
        those two corners and sent through PTUpdateInstances.  Does not reset accumulation.
        rebuild_above: update_geometry's policy; returns (bounds, "refit" or "rebuild") then."""
        off = self._blas_offsets(mesh)
        if rebuild_above is not None:
            bounds = self.morph_geometry(weights, joint_matrices, mesh=mesh)
            if self.geometry_quality(mesh)["sahCost"] <= rebuild_above * self._built_cost(mesh):
                return bounds, "refit"
            return self.morph_geometry(weights, joint_matrices, mesh=mesh, rebuild=True), "rebuild"
        flags = abi.PT_SKIN_REBUILD if rebuild else 0
        out = (C.c_float * 6)()
        if isinstance(weights, np.ndarray):
            w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
            m = None if joint_matrices is None else plugin.joint_palette(joint_matrices)
            plugin.check(self.lib.PTMorphGeometry(self.ctx, *off, w.ctypes.data, len(w), None if m is None else m.ctypes.data,
                                                  0 if m is None else m.shape[0], flags, out))
        else:
            import torch
            w, m = weights, joint_matrices
            assert w.is_contiguous() and w.dtype == torch.float32 and w.dim() == 1
            assert m is None or (m.is_contiguous() and m.dtype == torch.float32 and m.numel() % 12 == 0 and tuple(m.shape[1:]) in ((3, 4), (12,)))
            with self._ordered(w.device):
                plugin.check(self.lib.PTMorphGeometryDevice(self.ctx, *off, w.data_ptr(), w.numel(), None if m is None else m.data_ptr(),
                                                            0 if m is None else m.numel() // 12, flags, out))
        bounds = np.array(out, np.float32).reshape(2, 3)
        if rebuild:
            self._builtCost[mesh] = self.geometry_quality(mesh)["sahCost"]
        self._send_instance_bounds(mesh, bounds)
        return bounds

    def _send_instance_bounds(self, mesh, bounds):
        """HAS_TLAS: the world bounds of the mesh's instances from its local box, through PTUpdateInstances"""
        bvh = self._bvhScene
        if bvh.gpu_instances is None:
            return
        from .scenes import instance_world_bounds
        for k, (m_, _, _) in enumerate(self.scene.instances):
            if m_ != mesh:
                continue
            l2w = bvh.gpu_instances[k]["localToWorld"].reshape(4, 4).T.astype(np.float64)
            bvh.blas_instances[k]["aabbMin"], bvh.blas_instances[k]["aabbMax"] = instance_world_bounds(bounds, l2w)
        plugin.check(self.lib.PTUpdateInstances(self.ctx, bvh.blas_instances.ctypes.data, bvh.blas_instances.shape[0]))

    def read_geometry(self):
        """PTReadGeometry: the current (nodes uint8[], tris uint8[], tri_attrs abi.TRI_ATTR[]) of the whole scene.  Synchronising."""
        bvh = self._bvhScene
        nodes, tris = np.empty(bvh.bvh_nodes.nbytes, np.uint8), np.empty(bvh.bvh_tris.nbytes, np.uint8)
        attrs = np.empty(bvh.tri_attrs.shape, bvh.tri_attrs.dtype)
        plugin.check(self.lib.PTReadGeometry(self.ctx, nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes, attrs.ctypes.data, attrs.nbytes))
        return nodes, tris, attrs

    def close(self):
        if self.ctx:
            self.lib.PTDestroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProbeVolume:
    """A baked probe grid on the device (PathTracer.bake_probe_volume; include/ptmi_plugin.h Part 16): the grid, the SH
    coefficients (n, 9, 3), their luminance moments (n,) and the depth records (n, 64, 2), x fastest.  placement: None, or the
    (n, 4) float32 PTProbePlacement rows of bake_probe_volume(relocate=...) (Part 18) -- offset xyz and state bits; sh and depth were
    then baked at position + offset, and irradiance() leaves out the probes marked PT_PROBE_INSIDE."""

    def __init__(self, tracer: "PathTracer", grid: abi.PTProbeGrid, sh, m2, depth, max_distance: float, placement=None):
        import torch
        self.tracer, self.grid, self.sh, self.m2, self.depth, self.max_distance = tracer, grid, sh, m2, depth, float(max_distance)
        self.placement = None if placement is None else placement.contiguous()
        assert placement is None or placement.shape == (sh.shape[0], 4), placement.shape
        n = sh.shape[0]
        assert n == grid.counts[0] * grid.counts[1] * grid.counts[2] and depth.shape == (n, 64, 2), (sh.shape, depth.shape)
        self._rows = torch.zeros((n, 28), dtype=torch.float32, device=sh.device)          # PTProbeCoeffs rows
        self._rows[:, :27] = sh.reshape(n, 27)
        self._rows[:, 27] = m2
        self._depth = depth.contiguous()

    @property
    def counts(self):
        return tuple(int(c) for c in self.grid.counts)

    def positions(self) -> np.ndarray:
        return plugin.probe_grid_positions(self.grid)

    def default_normal_bias(self) -> float:
        """a fifth of the smallest spacing along an axis that has more than one probe (0 for a single probe)"""
        s = [self.grid.spacing[a] for a in range(3) if self.grid.counts[a] > 1]
        return 0.2 * min(s) if s else 0.0

    def irradiance(self, positions=None, normals=None, receivers=None, wrap: bool = True, visibility: bool = True, normal_bias: float = None):
        """PTProbeGridIrradiancePlaced (PTProbeGridIrradiance for a volume without a placement): the irradiance the volume gives at
        points with unit normals, blended from the up to eight probes around each point.  wrap: weigh a probe by the side of the
        surface it is on; visibility: weigh it by the Chebyshev bound of its depth record, which keeps a lit room's probes out of
        the dark room next door.  normal_bias: how far the point is moved along its normal before the distance to a probe is taken
        (None: default_normal_bias()).

        positions, normals: (q, 3) float32, or receivers: (q, 8) float32 PTReceiver rows as chart_receivers returns them.  numpy in,
        numpy out; device tensors in, a device tensor out.  Returns (q, 4) float32: irradiance rgb and the support sumW."""
        import torch
        pt = self.tracer
        dev = self._rows.device
        if receivers is not None:
            assert positions is None and normals is None, "receivers come instead of positions and normals"
            as_numpy = isinstance(receivers, np.ndarray)
            recv = torch.from_numpy(np.ascontiguousarray(receivers, dtype=np.float32)).to(dev) if as_numpy else receivers.contiguous()
        else:
            as_numpy = isinstance(positions, np.ndarray) or not hasattr(positions, "device")
            if as_numpy:
                recv = torch.from_numpy(plugin.receiver_rows(positions, normals)).to(dev)
            else:
                recv = pt._receivers(positions, normals, None)
        assert recv.dtype == torch.float32 and recv.ndim == 2 and recv.shape[1] == 8, (recv.dtype, recv.shape)
        g = abi.PTProbeGrid.from_buffer_copy(self.grid)
        g.flags = (abi.PT_GRID_WRAP if wrap else 0) | (abi.PT_GRID_VISIBILITY if visibility else 0)
        g.normalBias = self.default_normal_bias() if normal_bias is None else float(normal_bias)
        q = recv.shape[0]
        out = torch.empty((q, 4), dtype=torch.float32, device=dev)
        if q:
            with pt._ordered(dev):
                plugin.check(pt.lib.PTProbeGridIrradiancePlaced(pt.ctx, C.byref(g), self._rows.data_ptr(), self._depth.data_ptr(),
                                                                None if self.placement is None else self.placement.data_ptr(), recv.data_ptr(), q, out.data_ptr()))
        return out.cpu().numpy() if as_numpy else out


class ReflectionProbes:
    """Captured and prefiltered reflection probes on the device (PathTracer.capture_reflection_probes; include/ptmi_plugin.h Part
    20): maps (n, plugin.reflection_texel_count(res, levels), 4) float32, the PTProbe rows (n, 4) and, with box projection, the
    PTReflectionBox rows (n, 8)."""

    def __init__(self, tracer: "PathTracer", res: int, levels: int, maps, probe_rows, box_rows=None):
        self.tracer, self.res, self.levels = tracer, int(res), int(levels)
        self.maps, self.probe_rows, self.box_rows = maps.contiguous(), probe_rows.contiguous(), None if box_rows is None else box_rows.contiguous()
        n = self.probe_rows.shape[0]
        assert self.maps.shape == (n, plugin.reflection_texel_count(res, levels), 4), self.maps.shape
        assert self.box_rows is None or self.box_rows.shape == (n, 8), self.box_rows.shape

    @property
    def positions(self):
        return self.probe_rows[:, 0:3]

    def level(self, k: int):
        """level k of every map as images: (n, res >> k, res >> k, 4), row v, column u; a view of the device maps"""
        assert 0 <= k < self.levels, k
        rk, first = self.res >> k, plugin.reflection_texel_count(self.res, k)
        return self.maps[:, first:first + rk * rk].reshape(-1, rk, rk, 4)

    def lookup(self, directions, roughness, probes, positions=None):
        """PTReflectionLookup: the prefiltered radiance a surface of `roughness` (0 ... 1) reflects from `directions` (the reflection
        vector, (q, 3) float32), read from probe `probes` ((q,) indices, or one): trilinear between the four nearest texels of the
        two nearest levels.  positions: the surface points (q, 3); with boxes given at the capture, a direction from a point inside
        its probe's box is first projected onto the box and re-aimed from the probe's position.  numpy in, numpy out; device
        tensors in, a device tensor out.  Returns (q, 4) float32: rgb and 1 (zeros for a probe index out of range)."""
        import torch
        pt, dev = self.tracer, self.maps.device
        as_numpy = isinstance(directions, np.ndarray) or not hasattr(directions, "device")
        if as_numpy:
            rows = torch.from_numpy(plugin.reflection_query_rows(directions, roughness, probes, positions)).to(dev)
        else:
            d = directions.reshape(-1, 3)
            q = d.shape[0]
            assert d.dtype == torch.float32, d.dtype
            rows = torch.zeros((q, 8), dtype=torch.float32, device=dev)
            if positions is not None:
                rows[:, 0:3] = positions.reshape(q, 3)
            rows[:, 3] = torch.as_tensor(roughness, dtype=torch.float32, device=dev).expand(q)
            rows[:, 4:7] = d
            idx = torch.as_tensor(probes, device=dev)
            rows.view(torch.int32)[:, 7] = pt._seed_bits(idx.expand(q) if idx.dim() == 0 else idx, q, dev)
        q = rows.shape[0]
        use_boxes = self.box_rows is not None and positions is not None
        out = torch.empty((q, 4), dtype=torch.float32, device=dev)
        if q:
            with pt._ordered(dev):
                plugin.check(pt.lib.PTReflectionLookup(pt.ctx, self.maps.data_ptr() or None, self.maps.shape[0], self.res, self.levels,
                                                       self.probe_rows.data_ptr() or None, self.box_rows.data_ptr() if use_boxes else None,
                                                       rows.data_ptr(), q, out.data_ptr()))
        return out.cpu().numpy() if as_numpy else out


def select_blocks(tiles, samples, threshold: float, max_samples: int, add_samples: int, dilate: bool) -> np.ndarray:
    """PTSelectActiveBlocks restated: tiles / samples are the (rows, columns) tile map and block sample counts.  A block is
    selected when its tile value > threshold and samples + add_samples <= max_samples; with dilate also the up to eight
    neighbours of such a block that meet the sample limit.  Returns the ascending block ids (uint32)."""
    tiles = np.asarray(tiles, np.float32)
    samples = np.asarray(samples, np.uint64)
    within = samples + np.uint64(add_samples) <= np.uint64(max_samples)
    core = (tiles > np.float32(threshold)) & within
    pick = core.copy()
    if dilate:
        rows, cols = core.shape
        for by, bx in zip(*np.nonzero(core)):
            y0, y1, x0, x1 = max(by - 1, 0), min(by + 2, rows), max(bx - 1, 0), min(bx + 2, cols)
            pick[y0:y1, x0:x1] |= within[y0:y1, x0:x1]
    return np.flatnonzero(pick.reshape(-1)).astype(np.uint32)


def list_slot_to_pixel(width: int, height: int, ids, cover=None):
    """The slot -> pixel mapping of a pass over a block list (pt_launch.h PTListMap), restated: slot e * 256 + tid of entry e =
    block ids[e], four 8x8 waves per block.  Returns (px, py, valid) arrays of len(ids) * 256 entries."""
    cw, ch = cover or (width, height)
    cols = (width + 15) // 16
    ids = np.asarray(ids, np.int64)
    tid = np.arange(256)
    wave, lane = tid >> 6, tid & 63
    px = ((ids % cols) * 16)[:, None] + ((wave & 1) * 8 + (lane & 7))[None, :]
    py = ((ids // cols) * 16)[:, None] + ((wave >> 1) * 8 + (lane >> 3))[None, :]
    return px.reshape(-1), py.reshape(-1), ((px < cw) & (py < ch)).reshape(-1)


def _device_to_numpy(ptr: int, shape) -> np.ndarray:
    """Copy float32 device memory at `ptr` into a new numpy array of `shape` (the HIP runtime's hipMemcpy, synchronous)."""
    out = np.empty(shape, dtype=np.float32)
    plugin.hip_memcpy(out.ctypes.data, ptr, out.nbytes, plugin.HIP_MEMCPY_D2H)
    return out
