"""PathTracer's bakes (include/ptmi_plugin.h Parts 13 to 23): irradiance gathers, lightmap charts and their filter, SH probes,
probe volumes and placement, reflection probes, and first hits shaded from all of them -- with `ProbeVolume` and
`ReflectionProbes`, the bakes that stay on the device."""
import ctypes as C

import numpy as np

from . import abi, plugin
from ._hostcalls import HostCalls, address, is_numpy, torch


def probe_grid(lo, hi, counts) -> np.ndarray:
    """Probe positions on a regular grid: counts = (nx, ny, nz) points from corner lo to corner hi inclusive (a count of 1 sits in
    the middle of its axis).  Returns (nx * ny * nz, 3) float32, x fastest, as probe_sh() takes them."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    counts = [int(c) for c in counts]
    assert len(counts) == 3 and min(counts) >= 1, counts
    axes = [np.linspace(lo[a], hi[a], counts[a]) if counts[a] > 1 else np.array([0.5 * (lo[a] + hi[a])]) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.float32)


class Bakes(HostCalls):
    def _sample_rays(self, fn, rows, p, first_sample, spp):
        """PTGatherRays / PTProbeRays (`fn`) over receiver / probe rows: the (n * spp, 8) ray rows, numpy for numpy rows (uploaded
        and read back), else a device tensor"""
        d_rows, as_numpy = self._as_rows(rows)
        n = rows.shape[0]
        return self._device_call(fn, [C.byref(p), d_rows, n, first_sample & 0xFFFFFFFF, spp], [((n * max(spp, 0), 8), "float32")], as_numpy)

    # ---- irradiance gathers (include/ptmi_plugin.h Part 13)
    def _receivers(self, positions, normals, seeds):
        """(n, 8) float32 PTReceiver rows -- position xyz, seed bits, normal xyz, 0 -- of the kind the positions are (numpy or a
        device tensor); seeds None = the entry index."""
        if is_numpy(positions):
            pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
            nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            assert pos.shape == nrm.shape, (pos.shape, nrm.shape)
            n = pos.shape[0]
            recv = np.zeros((n, 8), np.float32)
            recv[:, 0:3], recv[:, 4:7] = pos, nrm
            sd = np.arange(n, dtype=np.uint32) if seeds is None else np.ascontiguousarray(np.asarray(seeds).astype(np.uint32)).reshape(n)
            recv[:, 3] = sd.view(np.float32)
            return recv
        assert positions.dtype == torch.float32 and normals.dtype == torch.float32 and positions.shape == normals.shape, (positions.shape, normals.shape)
        n = positions.reshape(-1, 3).shape[0]
        recv = torch.zeros((n, 8), dtype=torch.float32, device=positions.device)
        recv[:, 0:3], recv[:, 4:7] = positions.reshape(-1, 3), normals.reshape(-1, 3).to(positions.device)
        recv.view(torch.int32)[:, 3] = self._seed_bits(seeds, n, positions.device)
        return recv

    def _gather_rows(self, positions, normals, seeds, receivers):
        """The (n, 8) PTReceiver rows of a gather, numpy or a device tensor: _receivers(positions, normals, seeds), or the ready-made
        `receivers` that come instead of the three"""
        if receivers is None:
            return self._receivers(positions, normals, seeds)
        assert positions is None and normals is None and seeds is None, "receivers come instead of positions, normals and seeds"
        assert receivers.dtype == np.float32 or str(receivers.dtype) == "torch.float32", receivers.dtype
        return self._as_rows(receivers, 8, stage=False)[0]

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
        recv = self._gather_rows(positions, normals, seeds, receivers)
        return self._twin_call(self.lib.PTGatherIrradiance, self.lib.PTGatherIrradianceHost, recv, [((recv.shape[0], 4), "float32")],
                               head=(C.byref(p),), tail=(first_sample & 0xFFFFFFFF, spp))

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
        recv = self._gather_rows(positions, normals, seeds, receivers)
        n = recv.shape[0]
        if dark_floor is None:
            first = self.irradiance(receivers=recv, spp=min_samples, first_sample=first_sample, params=p) if n else np.zeros((0, 4), np.float32)
            first = first if isinstance(first, np.ndarray) else self._result([first], as_numpy=True)     # read back for the mean
            rgb = first[np.isfinite(first).all(axis=1), :3].astype(np.float64)
            dark_floor = 0.01 * float((rgb @ np.array([0.299, 0.587, 0.114])).mean()) if len(rgb) else 0.0
            dark_floor = dark_floor if np.isfinite(dark_floor) and dark_floor > 0.0 else 0.0
        a = abi.adaptive_gather(threshold, min_samples, add_samples, max_samples, dark_floor, first_sample)
        st = abi.PTAdaptiveGatherStats()
        out, counts = self._twin_call(self.lib.PTGatherIrradianceAdaptive, self.lib.PTGatherIrradianceAdaptiveHost, recv, [((n, 4), "float32"), ((n,), "uint32")],
                                      head=(C.byref(p), C.byref(a)), after=(C.byref(st),))
        return out, counts, dict(st.as_dict(), darkFloor=float(a.darkFloor))

    def equalise_irradiance(self, irradiance, counts, samples_eq: int):
        """PTEqualiseIrradiance: rewrites m2 of an irradiance_adaptive() list (device tensors: (n, 4) float32 and (n,) int32 counts) so
        that denoise_lightmap(..., samples=samples_eq) recovers every entry's own variance of the mean.  Returns a new (n, 4) tensor."""
        n = irradiance.shape[0]
        assert irradiance.dtype == torch.float32 and irradiance.is_contiguous() and irradiance.shape == (n, 4), irradiance.shape
        assert counts.element_size() == 4 and counts.is_contiguous() and counts.shape == (n,), counts.shape
        return self._device_call(self.lib.PTEqualiseIrradiance, [irradiance, counts, n, int(samples_eq)], [((n, 4), "float32")], empty="null")

    def gather_rays(self, positions, normals, spp: int = 64, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None):
        """PTGatherRays: the gather ray and RNG state each sample of irradiance() leaves the receiver with, as radiance() takes
        them: (n * spp, 8) float32 rows, entry-major (row i * spp + j = sample first_sample + j of entry i); a sample that ended at
        the receiver has a NaN direction.  numpy in, numpy out; device tensors in, a device tensor out."""
        return self._sample_rays(self.lib.PTGatherRays, self._receivers(positions, normals, seeds), self._radiance_params(params), first_sample, spp)

    # ---- SH light probes (include/ptmi_plugin.h Part 15)
    def _probes(self, positions, seeds):
        """(n, 4) float32 PTProbe rows -- position xyz, seed bits -- of the kind the positions are; seeds None = the probe index."""
        if is_numpy(positions):
            return plugin.probe_rows(positions, seeds)
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
        out = self._twin_call(self.lib.PTProbeSH, self.lib.PTProbeSHHost, rows, [((n, 28), "float32")], head=(C.byref(p),),
                              tail=(first_sample & 0xFFFFFFFF, spp, flags))
        sh, m2 = out[:, :27].reshape(n, 9, 3), out[:, 27]
        return (sh.copy(), m2.copy()) if isinstance(out, np.ndarray) else (sh, m2)

    def probe_rays(self, positions, spp: int = 256, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None):
        """PTProbeRays: the ray and RNG state each sample of probe_sh() starts with, as radiance() takes them: (n * spp, 8) float32
        rows, entry-major (row i * spp + j = sample first_sample + j of probe i).  numpy in, numpy out; a device tensor in, a
        device tensor out."""
        return self._sample_rays(self.lib.PTProbeRays, self._probes(positions, seeds), self._radiance_params(params), first_sample, spp)

    def probe_irradiance(self, sh, normals, probes):
        """PTProbeIrradiance: the irradiance the coefficients of probe_sh() give for unit normals.  sh (n, 9, 3), normals (q, 3),
        probes (q,) indices into sh (an index >= n gives zeros).  Returns (q, 4) float32 PTIrradiance rows, m2 = 0.  numpy in, numpy
        out; device tensors in, a device tensor out."""
        dev = self._device
        as_numpy = is_numpy(sh)
        if as_numpy:
            d_sh, d_q = self._as_rows(plugin.probe_coeff_rows(sh))[0], self._as_rows(plugin.probe_query_rows(normals, probes))[0]
        else:
            assert sh.dtype == torch.float32 and normals.dtype == torch.float32, (sh.dtype, normals.dtype)
            d_sh = torch.zeros((sh.reshape(-1, 27).shape[0], 28), dtype=torch.float32, device=dev)
            d_sh[:, :27] = sh.reshape(-1, 27)
            nrm = normals.reshape(-1, 3)
            d_q = torch.empty((nrm.shape[0], 4), dtype=torch.float32, device=dev)
            d_q[:, 0:3] = nrm
            d_q.view(torch.int32)[:, 3] = self._seed_bits(probes, -1, dev)
        q = d_q.shape[0]
        return self._device_call(self.lib.PTProbeIrradiance, [address(d_sh, "null"), d_sh.shape[0], d_q, q], [((q, 4), "float32")], as_numpy, empty="skip")

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
        return self._twin_call(self.lib.PTProbeDepth, self.lib.PTProbeDepthHost, rows, [((rows.shape[0], 64, 2), "float32")],
                               tail=(first_sample & 0xFFFFFFFF, spp, max_distance))

    # ---- reflection probes (include/ptmi_plugin.h Part 20)
    def reflection_rays(self, positions, res: int = 64, spp: int = 16, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None):
        """PTReflectionRays: the ray and RNG state each sample of capture_reflection_probes() starts with, as radiance() takes them:
        (n * res * res * spp, 8) float32 rows, slot-major (row (i * res * res + t) * spp + j = sample first_sample + j of texel t of
        probe i).  numpy in, numpy out; a device tensor in, a device tensor out."""
        p = self._radiance_params(params)
        d_rows, as_numpy = self._as_rows(self._probes(positions, seeds))
        n = d_rows.shape[0]
        ok = abi.PT_REFLECTION_MIN_RES <= res <= abi.PT_REFLECTION_MAX_RES and 0 <= spp <= 65536     # (the call refuses the rest itself)
        return self._device_call(self.lib.PTReflectionRays, [C.byref(p), d_rows, n, res, first_sample & 0xFFFFFFFF, spp],
                                 [((n * res * res * spp if ok else 0, 8), "float32")], as_numpy, empty="dummy")

    def capture_reflection_base(self, positions, res: int = 64, spp: int = 16, first_sample: int = 0, seeds=None, params: abi.PTFrameParams = None):
        """PTReflectionCapture: the base maps alone, (n, res * res, 4) float32 -- mean radiance rgb and the sum of the samples' squared
        luminances per texel v * res + u of the octahedral map.  numpy positions -> PTReflectionCaptureHost, returns numpy; a device
        tensor -> PTReflectionCapture zero-copy, ordered against torch's current stream both ways, returns a device tensor."""
        p = self._radiance_params(params)
        rows = self._probes(positions, seeds)
        ok = abi.PT_REFLECTION_MIN_RES <= res <= abi.PT_REFLECTION_MAX_RES
        return self._twin_call(self.lib.PTReflectionCapture, self.lib.PTReflectionCaptureHost, rows, [((rows.shape[0], res * res if ok else 1, 4), "float32")],
                               head=(C.byref(p),), tail=(res, first_sample & 0xFFFFFFFF, spp), empty="dummy")

    def prefilter_reflection(self, base, res: int, levels: int):
        """PTReflectionPrefilter: base maps (n, res * res, 4) float32 -> whole maps (n, plugin.reflection_texel_count(res, levels), 4),
        level k filtered with the GGX lobe of roughness k / (levels - 1).  numpy in, numpy out; a device tensor in, a device tensor
        out."""
        d_base, as_numpy = self._as_rows(base)
        assert d_base.dim() == 3 and d_base.shape[2] == 4, (d_base.dtype, d_base.shape)
        n = d_base.shape[0]
        ok = abi.PT_REFLECTION_MIN_RES <= res <= abi.PT_REFLECTION_MAX_RES and 1 <= levels <= 8
        return self._device_call(self.lib.PTReflectionPrefilter, [d_base, n, res, levels],
                                 [((n, plugin.reflection_texel_count(res, levels) if ok else 1, 4), "float32")], as_numpy, empty="dummy")

    def capture_reflection_probes(self, positions, res: int = 64, spp: int = 16, levels: int = 5, first_sample: int = 0, seeds=None, boxes=None,
                                  params: abi.PTFrameParams = None):
        """Reflection probes on the GPU: what a glossy object that moves through a baked scene reads.  Every probe is an octahedral
        radiance map of res x res texels around a point, `spp` paths of the render's own per texel (jittered inside the texel;
        bounces, roulette, firefly filter from `params`, default this tracer's), prefiltered into `levels` levels of roughness
        0 ... 1 with the GGX lobe.  boxes: None, or (bmin, bmax), each (n, 3) or (3,): the box each probe's surroundings stand for,
        which lookup() projects directions onto (parallax correction).

        positions: (n, 3) float32, numpy or a tensor on this context's device; seeds: (n,) uint32, None = the probe index.  Returns a
        ReflectionProbes, whose maps stay on the device."""
        d_rows, _ = self._as_rows(self._probes(positions, seeds))
        base = self.capture_reflection_base(d_rows[:, 0:3].contiguous(), res, spp, first_sample, d_rows.view(torch.int32)[:, 3], params)
        maps = self.prefilter_reflection(base, res, levels)
        d_boxes = None
        if boxes is not None:
            n = d_rows.shape[0]
            lo, hi = (np.broadcast_to(np.asarray(b, np.float32), (n, 3)) for b in boxes)
            d_boxes, _ = self._as_rows(plugin.reflection_box_rows(lo, hi))
        return ReflectionProbes(self, res, levels, maps, d_rows, d_boxes)

    # ---- shading from the bakes (include/ptmi_plugin.h Part 21)
    def bake_dfg(self, res: int = 32):
        """PTBakeDFG: the split-sum table of the specular BRDF on the GPU, a (res, res, 2) float32 device tensor -- row j =
        perceptual roughness (j + 0.5) / res, column i = N.V (i + 0.5) / res, {scale, bias} of F0; plugin.bake_dfg is its twin."""
        ok = int(res) in abi.PT_SHADE_DFG_RES                                 # (the call refuses another res itself)
        return self._device_call(self.lib.PTBakeDFG, [int(res)], [((res, res, 2) if ok else (1, 1, 2), "float32")])

    def _first_hits(self, rays, hits, surfaces):
        """(rays (n, 8), hits (n, 4), surfaces (n, 12) on the device, n, were numpy): what trace_rays(rays, surface=True) took and
        returned, as the shading calls take it"""
        r, as_numpy = self._as_rows(rays, 8)
        h, _ = self._as_rows(hits, 4)
        s, _ = self._as_rows(surfaces, 12)
        n = r.shape[0]
        assert h.shape[0] == n and s.shape[0] == n, (r.shape, h.shape, s.shape)
        return r, h, s, n, as_numpy

    def shade_surfaces(self, rays, hits, surfaces, probes=None, boxes=None):
        """PTShadeSurfaces: from what trace_rays(rays, surface=True) took and returned to what the bakes are asked -- the material
        record the render's own fetch gives for every hit (n, 12), the shading terms (n, 12), the PTReceiver rows (n, 8) a probe
        volume takes and the PTReflectionQuery rows (n, 8) reflection probes take.  probes: (k, 4) PTProbe rows or (k, 3)
        positions, or None; boxes: (k, 8) PTReflectionBox rows or None.  numpy in, numpy out; device tensors in, device tensors
        out."""
        r, h, s, n, as_numpy = self._first_hits(rays, hits, surfaces)
        pr = None
        if probes is not None:
            pr = self._as_rows(probes if probes.shape[1] == 4 else self._probes(probes, None), 4)[0]
        bx = None if boxes is None else self._as_rows(boxes, 8)[0]
        k = 0 if pr is None else pr.shape[0]
        return self._device_call(self.lib.PTShadeSurfaces, [r, h, s, n, None if pr is None else address(pr, "null"), bx, k],
                                 [((n, c), "float32") for c in (12, 12, 8, 8)], as_numpy, empty="skip")

    def shade_compose(self, terms, irradiance, reflection, dfg):
        """PTShadeCompose: emission + occlusion * (diffuse * E / pi + spec * (f0 * A + B)) per entry, (A, B) bilinear in the DFG
        table at (N.V, roughness).  terms (n, 12), irradiance (n, 4), reflection (n, 4), dfg (res, res, 2).  Returns (n, 4): rgb and
        1, zeros for a miss.  numpy in, numpy out; device tensors in, a device tensor out."""
        t, as_numpy = self._as_rows(terms, 12)
        e, _ = self._as_rows(irradiance, 4)
        s, _ = self._as_rows(reflection, 4)
        d, _ = self._as_rows(dfg)
        n = t.shape[0]
        assert e.shape[0] == n and s.shape[0] == n and d.dim() == 3 and d.shape[0] == d.shape[1] and d.shape[2] == 2, (t.shape, e.shape, s.shape, d.shape)
        return self._device_call(self.lib.PTShadeCompose, [t, e, s, n, d, d.shape[0]], [((n, 4), "float32")], as_numpy, empty="skip")

    def _shade_inputs(self, volume, reflections, dfg, wrap=True, visibility=True, normal_bias=None, placement=True, boxes=True):
        """(PTShadeInputs, the tensors it points into) from a ProbeVolume, a ReflectionProbes or None (no probes: the specular term
        reads zeros) and a DFG table or None (a 32 x 32 table, baked once per context)"""
        if dfg is None:
            if getattr(self, "_dfg", None) is None:
                self._dfg = self.bake_dfg(32)
            dfg = self._dfg
        d, _ = self._as_rows(dfg)
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

    def _shade_list(self, fn, rays, hits, surfaces, volume, reflections, dfg, options):
        """shade_baked's and shade_lightmapped's body: `fn` is PTShadeBaked or PTShadeLightmapped"""
        r, h, sf, n, as_numpy = self._first_hits(rays, hits, surfaces)
        s, keep = self._shade_inputs(volume, reflections, dfg, **options)           # keep: alive until the call is enqueued
        return self._device_call(fn, [C.byref(s), r, h, sf, n], [((n, 4), "float32")], as_numpy, empty="skip")

    def _shade_frame(self, fn, params, volume, reflections, dfg, return_rays, options):
        """render_baked's and render_lightmapped's body: `fn` is PTShadeBakedFrame or PTShadeLightmappedFrame"""
        p = params or self.params(seed=0)
        s, keep = self._shade_inputs(volume, reflections, dfg, **options)           # keep: alive until the call is enqueued
        w, h = int(p.OutputWidth), int(p.OutputHeight)
        out, rays = self._device_call(fn, [C.byref(p), C.byref(s)], [((h, w, 4), "float32"), ((h * w, 8), "float32") if return_rays else None])
        return (out, rays) if return_rays else out

    def shade_baked(self, rays, hits, surfaces, volume, reflections=None, dfg=None, **options):
        """PTShadeBaked: the first hits of trace_rays(rays, surface=True) shaded from a ProbeVolume and a ReflectionProbes in one
        kernel -- the material fetch, the terms, the volume's lookup (the placed one for a volume with a placement), the nearest
        reflection probe's lookup (the nearest whose box holds the point, with boxes) and the compose step, bit for bit what
        shade_surfaces, volume.irradiance, reflections.lookup and shade_compose give one after the other.  options: wrap,
        visibility, normal_bias as ProbeVolume.irradiance takes them; placement=False, boxes=False leave those out.  Returns
        (n, 4) float32: rgb and 1, zeros for a miss.  numpy in, numpy out; device tensors in, a device tensor out."""
        return self._shade_list(self.lib.PTShadeBaked, rays, hits, surfaces, volume, reflections, dfg, options)

    def render_baked(self, params: abi.PTFrameParams, volume, reflections=None, dfg=None, return_rays: bool = False, **options):
        """PTShadeBakedFrame: the frame `params` describes (None: this tracer's), every pixel's centre ray traced to its first hit
        and shaded from the bakes: a view of the scene lit by a ProbeVolume and a ReflectionProbes, as they are returned by
        bake_probe_volume and capture_reflection_probes.  dfg: a DFG table, None = a 32 x 32 one baked once per context.  Returns
        the (height, width, 4) float32 device tensor, and with return_rays the (height * width, 8) PTRay rows it traced."""
        return self._shade_frame(self.lib.PTShadeBakedFrame, params, volume, reflections, dfg, return_rays, options)

    # ---- first hits shaded from baked lightmaps (include/ptmi_plugin.h Part 22)
    def lightmap_binding(self, image, mesh: int = None, instance: int = None, uvs=None, two_sided: bool = False):
        """One entry for bind_lightmaps: `image`, an (height, width, 4) float32 lightmap as bake_lightmap / resolve_lightmap return it
        (numpy, or a tensor on this context's device; w > 0 marks a filled texel), bound to the primitives of one mesh.  mesh names
        the BLAS as chart_receivers does (None on a flat scene: the whole scene).  instance: None = whichever instance was hit (the
        only choice on a flat scene), else only hits of that instance read this image.  uvs: the (T, 6) float32 lightmap UVs the
        image was baked with, None = the attribute records' uv0 .. uv2.  two_sided: hits seen from behind read it too.  The entry
        keeps its tensors alive."""
        dev = self._device
        img, _ = self._as_rows(image)
        assert img.dim() == 3 and img.shape[2] == 4 and img.device == dev, (img.shape, img.dtype, img.device)
        bvh = self._bvhScene
        assert bvh.gpu_instances is not None or instance is None, "a flat scene has no instances"
        first, count = self._blas_offsets(mesh)[2], bvh.blas_spans[0 if mesh is None else mesh][3]
        d_uvs = None
        if uvs is not None:
            d_uvs, _ = self._as_rows(uvs)
            assert d_uvs.numel() == count * 6 and d_uvs.device == dev, (d_uvs.shape, d_uvs.dtype)
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
        bindings = list(bindings or [])
        table = (abi.PTLightmapBinding * max(len(bindings), 1))(*[b["record"] for b in bindings])
        self._device_call(self.lib.PTBindLightmaps, [table if bindings else None, len(bindings)], [])
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
        r, h, s, n, as_numpy = self._first_hits(rays, hits, surfaces)
        out, which = self._device_call(self.lib.PTLightmapLookup, [r, h, s, n], [((n, 4), "float32"), ((n,), "int32")], as_numpy, empty="skip")
        return (out, which.view(np.uint32)) if as_numpy else (out, which)

    def shade_lightmapped(self, rays, hits, surfaces, volume, reflections=None, dfg=None, **options):
        """PTShadeLightmapped: shade_baked, but a hit inside a bound lightmap's span reads its irradiance from the lightmap (four
        texels) instead of the probe volume; every other hit falls back to the volume.  Arguments, options and result as
        shade_baked's; with nothing bound the two are equal bit for bit."""
        return self._shade_list(self.lib.PTShadeLightmapped, rays, hits, surfaces, volume, reflections, dfg, options)

    def render_lightmapped(self, params: abi.PTFrameParams, volume, reflections=None, dfg=None, return_rays: bool = False, **options):
        """PTShadeLightmappedFrame: render_baked with the bound lightmaps as the diffuse source of the surfaces they cover: static
        surfaces read their lightmap, everything else the probe volume.  Arguments and result as render_baked's."""
        return self._shade_frame(self.lib.PTShadeLightmappedFrame, params, volume, reflections, dfg, return_rays, options)

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
        as_numpy = isinstance(rows, np.ndarray)
        if as_numpy:
            out = plugin.probe_placement_rows(start, None, n)
            assert out.shape[0] == n, (out.shape, n)
        else:
            out = torch.zeros((n, 4), dtype=torch.float32, device=rows.device)
            if start is not None:
                out[:, 0:3] = torch.as_tensor(start, dtype=torch.float32, device=rows.device).reshape(n, 3)
        out, st = self._twin_call(self.lib.PTProbePlace, self.lib.PTProbePlaceHost, rows, [out, ((n, 8), "int32", 0) if stats else None],
                                  tail=(first_sample & 0xFFFFFFFF, spp, C.byref(q), flags))
        res = (out[:, 0:3].copy(), out[:, 3].copy().view(np.uint32)) if as_numpy else (out[:, 0:3], out.view(torch.int32)[:, 3])
        if not stats:
            return res
        st = st if as_numpy else self._result([st], as_numpy=True)           # the records are numpy in either form
        return res + (st.view(abi.PLACE_STATS_DTYPE).reshape(n),)

    def bake_probe_volume(self, lo, hi, counts, spp: int = 256, depth_spp: int = 256, max_distance: float = None, first_sample: int = 0, seeds=None,
                          delta_lights: bool = True, params: abi.PTFrameParams = None, relocate=None) -> "ProbeVolume":
        """A probe volume over the box lo ... hi: counts = (nx, ny, nz) probes, the outer ones on the box's faces (a count of 1 sits
        in the middle of its axis).  Bakes probe_sh(spp) and probe_depth(depth_spp) at plugin.probe_grid_positions of the grid; both
        stay on the device.  max_distance: where a depth ray ends, default 1.5 x the diagonal of a cell.
        relocate: None or False -- the probes stay on the grid; True, or a dict of place_probes() arguments -- place_probes() runs
        first (the grid's spacing, first_sample and seeds), both bakes are made at position + offset (one float32 add per component,
        on the host), and the placement stays on the device for the lookup (ProbeVolume.placement).  Returns a ProbeVolume."""
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        counts = [int(c) for c in counts]
        assert len(counts) == 3 and min(counts) >= 1 and (hi >= lo).all(), (counts, lo, hi)
        origin = [lo[a] if counts[a] > 1 else 0.5 * (lo[a] + hi[a]) for a in range(3)]
        spacing = [(hi[a] - lo[a]) / (counts[a] - 1) if counts[a] > 1 else (hi[a] - lo[a] if hi[a] > lo[a] else 1.0) for a in range(3)]
        grid = plugin.probe_grid_desc(origin, spacing, counts)
        if max_distance is None:
            max_distance = 1.5 * float(np.linalg.norm([grid.spacing[a] for a in range(3)]))
        h_pos = plugin.probe_grid_positions(grid)
        pos, _ = self._as_rows(h_pos)
        d_seeds = None if seeds is None else self._as_rows(np.asarray(seeds).astype(np.int64), dtype=np.int64)[0]
        placement = None
        if relocate is not None and relocate is not False:
            args = dict(first_sample=first_sample)
            args.update({} if relocate is True else dict(relocate))
            offsets, states = self.place_probes(pos, [grid.spacing[a] for a in range(3)], seeds=d_seeds, **args)[:2]
            placement = torch.zeros((pos.shape[0], 4), dtype=torch.float32, device=pos.device)
            placement[:, 0:3] = offsets
            placement.view(torch.int32)[:, 3] = states
            pos, _ = self._as_rows((h_pos + self._result([offsets], as_numpy=True)).astype(np.float32))
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
        dev = self._device
        d = self._chart_desc(width, height, mesh, instance, seed)
        d_uvs = None
        if uvs is not None:
            d_uvs, _ = self._as_rows(uvs, strict=True)
            assert d_uvs.numel() == d.triangleCount * 6 and d_uvs.device == dev, (d_uvs.shape, d_uvs.dtype)
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
        assert texels.element_size() == 4 and texels.dim() == 1 and texels.is_contiguous(), (texels.dtype, texels.shape)
        assert irradiance.dtype == torch.float32 and irradiance.is_contiguous() and irradiance.shape == (texels.shape[0], 4), irradiance.shape
        return self._device_call(self.lib.PTResolveLightmap, [texels, irradiance, texels.shape[0], int(width), int(height), int(dilate)],
                                 [((max(int(height), 1), max(int(width), 1), 4), "float32")], empty="null")

    def denoise_lightmap(self, texels, receivers, irradiance, width: int, height: int, samples: int, iterations: int = 5, params=None):
        """PTDenoiseLightmap: a chart-aware a-trous filter over a gathered list, in texel space, on the GPU (Part 17 has the rule).
        texels: (n,) int32 / uint32 device tensor of unique texel indices and receivers: (n, 8) float32 PTReceiver rows
        (chart_receivers'), irradiance: (n, 4) float32 (irradiance()'s, of `samples` samples per texel, 2 or more).  iterations:
        0 ... 8 levels; params: a dict of abi.lightmap_denoise_params' keywords (sigma_luminance, sigma_position, sigma_plane,
        normal_power, iterations) or a PTLightmapDenoiseParams.  Returns an (n, 4) float32 device tensor that resolve_lightmap
        takes: the filtered rgb, and in m2's place the variance estimate of the filtered luminance.  Texels that touch in the atlas
        but not in the world do not mix.  Ordered against torch's current stream both ways."""
        assert texels.element_size() == 4 and texels.dim() == 1 and texels.is_contiguous(), (texels.dtype, texels.shape)
        n = texels.shape[0]
        assert receivers.dtype == torch.float32 and receivers.is_contiguous() and receivers.shape == (n, 8), receivers.shape
        assert irradiance.dtype == torch.float32 and irradiance.is_contiguous() and irradiance.shape == (n, 4), irradiance.shape
        p = plugin.lightmap_denoise_params(samples, iterations, params)
        return self._device_call(self.lib.PTDenoiseLightmap, [C.byref(p), texels, receivers, irradiance, n, int(width), int(height)], [((n, 4), "float32")],
                                 empty="null")

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
        image = self._result([self.resolve_lightmap(texels, irr, width, height, dilate=dilate)], as_numpy=not as_tensor)
        if not return_counts:
            return image
        count_image = torch.zeros((max(int(height), 1) * max(int(width), 1),), dtype=torch.int32, device=texels.device)
        if recv.shape[0]:
            count_image[texels.long()] = counts.to(torch.int32) if counts is not None else torch.full_like(texels, spp, dtype=torch.int32)
        count_image = count_image.reshape(max(int(height), 1), max(int(width), 1))
        return image, self._result([count_image], as_numpy=not as_tensor)

    # ---- lightmap UVs (include/ptmi_plugin.h Part 23)
    def unwrap_lightmap(self, width: int, height: int, mesh: int = None, texels_per_unit: float = None, padding: int = 2, vertices=None) -> "LightmapUnwrap":
        """Lightmap UVs of one mesh, made on the GPU from the scene's CURRENT geometry: PTUnwrapCharts cuts the mesh into charts by
        facing (connected triangles whose normals share their dominant axis and its sign), plugin.pack_charts places the chart
        rectangles on shelves on the host, PTEmitChartUVs writes the UVs.  No vertex and no UV leaves the device; the chart records
        (32 bytes per chart) do.

        mesh names the BLAS as update_geometry does (None on a flat scene).  texels_per_unit: the density in the mesh's local units;
        None = the largest one plugin.fit_chart_density finds for this atlas.  padding: empty texels around every chart (0 ... 16).
        vertices: a (3T, 4) float32 tensor on this context's device in the BLAS's primitive order -- what update_geometry takes --,
        None = the corners the triangle records hold, which weld a little less (a few more charts).
        Returns a LightmapUnwrap; its uvs go unchanged into chart_receivers(uvs=), bake_lightmap(uvs=) and lightmap_binding(uvs=).
        Raises ValueError when the charts do not fit the atlas at texels_per_unit.  Synchronises."""
        dev = self._device
        count = self._bvhScene.blas_spans[0 if mesh is None else mesh][3]
        d = abi.unwrap_desc(count, self._blas_offsets(mesh))
        d_verts = None
        if vertices is not None:
            d_verts, _ = self._as_rows(vertices, cols=4, strict=True)
            assert d_verts.shape[0] == 3 * count and d_verts.device == dev, (d_verts.shape, d_verts.device)
        v_ptr = None if d_verts is None else d_verts.data_ptr()
        n, st = C.c_uint32(), abi.PTUnwrapStats()
        chart_of_prim = torch.empty((count,), dtype=torch.int32, device=dev)
        with self._ordered(dev):
            # a mesh of a few charts: one call with room for 4096; more: the count first
            cap = 4096
            d_charts = torch.empty((cap, 8), dtype=torch.float32, device=dev)
            rc = self.lib.PTUnwrapCharts(self.ctx, C.byref(d), v_ptr, chart_of_prim.data_ptr(), d_charts.data_ptr(), cap, C.byref(n), C.byref(st))
            if rc != abi.PT_OK and n.value > cap:
                cap = n.value
                d_charts = torch.empty((cap, 8), dtype=torch.float32, device=dev)
                rc = self.lib.PTUnwrapCharts(self.ctx, C.byref(d), v_ptr, chart_of_prim.data_ptr(), d_charts.data_ptr(), cap, C.byref(n), C.byref(st))
            plugin.check(rc)
        d_charts = d_charts[:n.value]
        charts = d_charts.cpu().numpy().view(abi.UNWRAP_CHART_DTYPE).reshape(-1)
        if texels_per_unit is None:
            texels_per_unit, _ = plugin.fit_chart_density(charts, width, height, padding)
        origins, rows = plugin.pack_charts(charts, width, height, texels_per_unit, padding)
        if origins is None:
            raise ValueError(f"the charts do not fit {width} x {height} at {texels_per_unit} texels per unit (rows needed: {rows}, 0 = a chart is too wide)")
        d_origins = torch.from_numpy(origins).to(dev)
        uvs = torch.empty((count, 6), dtype=torch.float32, device=dev)
        with self._ordered(dev):
            plugin.check(self.lib.PTEmitChartUVs(self.ctx, C.byref(d), v_ptr, chart_of_prim.data_ptr(), address(d_charts, "dummy"), address(d_origins, "dummy", 1),
                                                 n.value, int(width), int(height), int(padding), float(texels_per_unit), uvs.data_ptr()))
        return LightmapUnwrap(uvs, chart_of_prim, charts, origins, float(texels_per_unit), int(rows), st.as_dict())


class LightmapUnwrap:
    """What PathTracer.unwrap_lightmap returns (include/ptmi_plugin.h Part 23): uvs, the (T, 6) float32 device tensor that
    chart_receivers, bake_lightmap and lightmap_binding take; chart_of_prim, (T,) int32 on the device (-1: an excluded triangle);
    charts, the numpy records of abi.UNWRAP_CHART_DTYPE; origins, (n, 2) int32 numpy; texels_per_unit; rows_used; stats."""

    def __init__(self, uvs, chart_of_prim, charts, origins, texels_per_unit, rows_used, stats):
        self.uvs, self.chart_of_prim, self.charts, self.origins = uvs, chart_of_prim, charts, origins
        self.texels_per_unit, self.rows_used, self.stats = texels_per_unit, rows_used, stats


class ProbeVolume:
    """A baked probe grid on the device (PathTracer.bake_probe_volume; include/ptmi_plugin.h Part 16): the grid, the SH
    coefficients (n, 9, 3), their luminance moments (n,) and the depth records (n, 64, 2), x fastest.  placement: None, or the
    (n, 4) float32 PTProbePlacement rows of bake_probe_volume(relocate=...) (Part 18) -- offset xyz and state bits; sh and depth were
    then baked at position + offset, and irradiance() leaves out the probes marked PT_PROBE_INSIDE."""

    def __init__(self, tracer: "PathTracer", grid: abi.PTProbeGrid, sh, m2, depth, max_distance: float, placement=None):
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
        pt = self.tracer
        if receivers is not None:
            assert positions is None and normals is None, "receivers come instead of positions and normals"
            recv, as_numpy = pt._as_rows(receivers, 8)
        else:
            as_numpy = is_numpy(positions)
            recv = pt._as_rows(plugin.receiver_rows(positions, normals), 8)[0] if as_numpy else pt._as_rows(pt._receivers(positions, normals, None), 8)[0]
        g = abi.PTProbeGrid.from_buffer_copy(self.grid)
        g.flags = (abi.PT_GRID_WRAP if wrap else 0) | (abi.PT_GRID_VISIBILITY if visibility else 0)
        g.normalBias = self.default_normal_bias() if normal_bias is None else float(normal_bias)
        q = recv.shape[0]
        return pt._device_call(pt.lib.PTProbeGridIrradiancePlaced, [C.byref(g), self._rows, self._depth, self.placement, recv, q], [((q, 4), "float32")],
                               as_numpy, empty="skip")


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
        pt, dev = self.tracer, self.maps.device
        as_numpy = is_numpy(directions)
        if as_numpy:
            rows, _ = pt._as_rows(plugin.reflection_query_rows(directions, roughness, probes, positions))
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
        return pt._device_call(pt.lib.PTReflectionLookup, [self.maps, self.maps.shape[0], self.res, self.levels, self.probe_rows,
                                                           self.box_rows if use_boxes else None, rows, q], [((q, 4), "float32")], as_numpy, empty="skip")
