"""PathTracer's direct light at first hits (include/ptmi_plugin.h Part 24): the analytic lights evaluated with shadow rays over
the bakes -- the pairs' rays, the sum, the fused call, the mixed list call and frame -- and `muted_lights`, which makes the bakes
fit that pass; and the light grid of Part 25 with the `culled=True` forms of the three fused calls."""
import contextlib
import ctypes as C

import numpy as np

from . import abi, plugin
from ._hostcalls import HostCalls, address


class Direct(HostCalls):
    @staticmethod
    def _direct_params(strata, seed, centered, min_alpha, params=None) -> abi.PTDirectParams:
        return params if params is not None else abi.direct_params(strata, seed, centered, min_alpha)

    def light_records(self) -> np.ndarray:
        """The scene's current PTLight records, (k, 16) float32: what update_lights sent last, else the scene's own.  This is the
        host layer's own copy -- the C API has no call that reads lights back --, so it follows update_lights only: after a
        PTUpdateLights made directly through `lib`, it (and what muted_lights() restores) is stale."""
        cur = getattr(self, "_lightRecords", None)
        return (self._bvhScene.lights.reshape(-1, 16) if cur is None else cur).copy()

    def direct_pair_count(self, strata: int = 1) -> int:
        """PTDirectPairCount: the pairs one entry has with the current lights -- 1 per point or spot light, strata * strata per
        rectangle light; 0 for a scene without lights."""
        n = C.c_uint32()
        plugin.check(self.lib.PTDirectPairCount(self.ctx, int(strata), C.byref(n)))
        return n.value

    def direct_rays(self, rays, terms, receivers, strata: int = 1, seed: int = 0, centered: bool = False, min_alpha: float = 0.0, params=None):
        """PTDirectRays: for every entry and every pair (light, stratum) the shadow ray and the contribution it carries when it
        arrives.  rays (n, 8) PTRay rows, terms (n, 12) and receivers (n, 8) as shade_surfaces returns them.  Returns (pair rays
        (n * pairs, 8), contributions (n * pairs, 4)); a pair that does not count has tmax = 0 and zero contribution.
        plugin.direct_rays is its twin.  numpy in, numpy out; device tensors in, device tensors out."""
        r, as_numpy = self._as_rows(rays, 8)
        t, _ = self._as_rows(terms, 12)
        rc, _ = self._as_rows(receivers, 8)
        n = r.shape[0]
        assert t.shape[0] == n and rc.shape[0] == n, (r.shape, t.shape, rc.shape)
        p = self._direct_params(strata, seed, centered, min_alpha, params)
        pairs = self.direct_pair_count(p.strata)
        return self._device_call(self.lib.PTDirectRays, [C.byref(p), r, t, rc, n], [((n * pairs, 8), "float32"), ((n * pairs, 4), "float32")],
                                 as_numpy, empty="skip")

    def direct_accumulate(self, terms, contrib, pair_hits, pairs_per_entry: int):
        """PTDirectAccumulate: per entry the sum, in pair order, of the contributions whose shadow ray hit nothing.  terms (n, 12),
        contrib (n * pairs, 4) as direct_rays returns it, pair_hits (n * pairs, 4): trace_rays(pair rays, any_hit=True).  Returns
        (n, 4): the direct light and 1, zeros for a miss.  numpy in, numpy out; device tensors in, a device tensor out."""
        t, as_numpy = self._as_rows(terms, 12)
        c, _ = self._as_rows(contrib, 4)
        h, _ = self._as_rows(pair_hits, 4)
        n = t.shape[0]
        assert c.shape[0] == n * pairs_per_entry and h.shape[0] == n * pairs_per_entry, (t.shape, c.shape, h.shape, pairs_per_entry)
        return self._device_call(self.lib.PTDirectAccumulate, [t, address(c, "null"), address(h, "null"), n, int(pairs_per_entry)], [((n, 4), "float32")],
                                 as_numpy, empty="skip")

    # ---- the light grid (include/ptmi_plugin.h Part 25)
    def build_light_grid(self, origin, cell_size: float, dims):
        """PTBuildLightGrid: a grid of dims[0] x dims[1] x dims[2] cubes of cell_size from origin over the scene's CURRENT lights,
        built on the GPU; every cell lists the lights that can reach it.  direct_light, shade_mixed and render_mixed take it with
        culled=True.  update_lights makes it stale: build it again before the next culled call.  plugin.build_light_grid is its
        twin.  Returns light_grid_info()."""
        p = abi.light_grid_params(origin, cell_size, dims)
        plugin.check(self.lib.PTBuildLightGrid(self.ctx, C.byref(p)))
        return self.light_grid_info()

    def _scene_bounds(self):
        """(min, max) of the scene's geometry in world space, float32: the instances' world boxes for a HAS_TLAS scene"""
        bvh = self._bvhScene
        if bvh.gpu_instances is not None:
            return bvh.blas_instances["aabbMin"].min(axis=0).astype(np.float32), bvh.blas_instances["aabbMax"].max(axis=0).astype(np.float32)
        v = np.asarray(self.scene.vertices)[:, :3]
        return v.min(axis=0).astype(np.float32), v.max(axis=0).astype(np.float32)

    def fit_light_grid(self, cell_size=None):
        """build_light_grid over the scene's bounds: cubes of cell_size -- None: the largest extent / 32, at least what keeps every
        axis within PT_LIGHT_GRID_MAX_DIM cells and the grid within PT_LIGHT_GRID_MAX_CELLS.  A good cell is about the range of a
        local light.  Returns light_grid_info()."""
        lo, hi = self._scene_bounds()
        extent = np.maximum((hi - lo).astype(np.float64), 1e-6)
        size = float(extent.max() / 32 if cell_size is None else cell_size)
        while True:
            dims = np.maximum(np.ceil(extent / size * (1 + 1e-6)).astype(np.int64), 1)
            if dims.max() <= abi.PT_LIGHT_GRID_MAX_DIM and int(dims.prod()) <= abi.PT_LIGHT_GRID_MAX_CELLS:
                break
            assert cell_size is None, f"cell_size {cell_size} gives {tuple(dims)} cells"
            size *= 1.25
        return self.build_light_grid(lo, size, dims)

    def light_grid_info(self) -> dict:
        """PTLightGridInfo: built, cells, lightCount, longest (list of a cell), stale, entries, generation"""
        s = abi.PTLightGridStats()
        s.structSize = C.sizeof(s)
        plugin.check(self.lib.PTLightGridInfo(self.ctx, C.byref(s)))
        return s.as_dict()

    def light_grid(self):
        """PTReadLightGrid: (offsets (cells + 2,), indices (total,), rect_before (L + 1,)), uint32 numpy arrays, as
        plugin.build_light_grid returns them"""
        info = self.light_grid_info()
        assert info["built"], "no light grid: build_light_grid first"
        offsets, indices = np.zeros(info["cells"] + 2, np.uint32), np.zeros(info["entries"], np.uint32)
        rect_before = np.zeros(info["lightCount"] + 1, np.uint32)
        plugin.check(self.lib.PTReadLightGrid(self.ctx, offsets.ctypes.data, indices.ctypes.data if indices.size else None, indices.size,
                                              rect_before.ctypes.data))
        return offsets, indices, rect_before

    def direct_light(self, rays, hits, surfaces, strata: int = 1, seed: int = 0, centered: bool = False, min_alpha: float = 0.0, params=None,
                     culled: bool = False):
        """PTDirectLight: the light of the scene's point, spot and rectangle lights at the first hits of trace_rays(rays,
        surface=True), shadow rays walked inside the kernel -- bit for bit what shade_surfaces, direct_rays, trace_rays(any_hit=True)
        and direct_accumulate give one after the other.  strata: a rectangle light is sampled on a strata x strata grid; centered:
        at the strata's centres, else jittered from `seed`; min_alpha: a floor under the specular lobe's alpha.  Returns (n, 4)
        float32: rgb and 1, zeros for a miss.  numpy in, numpy out; device tensors in, a device tensor out.
        culled: PTDirectLightCulled -- every wave walks only the lights the light grid lists for its entries' cells; the same bits.
        It needs a grid built for the current lights (build_light_grid, fit_light_grid): a stale or absent one is refused, also for
        an empty list.  DESIGN.md 5.30 has what it was measured to save, and to cost with two lights."""
        r, h, s, n, as_numpy = self._first_hits(rays, hits, surfaces)
        p = self._direct_params(strata, seed, centered, min_alpha, params)
        fn = self.lib.PTDirectLightCulled if culled else self.lib.PTDirectLight
        # an empty list: the unculled call is not made; the culled one is, with made-up addresses, for the grid's refusal
        return self._device_call(fn, [C.byref(p), r, h, s, n], [((n, 4), "float32")], as_numpy, empty="dummy" if culled else "skip")

    def shade_mixed(self, rays, hits, surfaces, volume, reflections=None, dfg=None, strata: int = 1, seed: int = 0, centered: bool = False,
                    min_alpha: float = 0.0, culled: bool = False, **options):
        """PTShadeMixed: shade_lightmapped plus direct_light, one add per channel -- sky, emissive surfaces and bounces from the
        bakes, the analytic lights with shadow rays.  Arguments as shade_lightmapped's and direct_light's; culled:
        PTShadeMixedCulled."""
        r, h, sf, n, as_numpy = self._first_hits(rays, hits, surfaces)
        s, keep = self._shade_inputs(volume, reflections, dfg, **options)           # keep: alive until the call is enqueued
        p = self._direct_params(strata, seed, centered, min_alpha)
        fn = self.lib.PTShadeMixedCulled if culled else self.lib.PTShadeMixed
        return self._device_call(fn, [C.byref(s), C.byref(p), r, h, sf, n], [((n, 4), "float32")], as_numpy, empty="dummy" if culled else "skip")

    def render_mixed(self, params: abi.PTFrameParams, volume, reflections=None, dfg=None, strata: int = 1, seed: int = 0, centered: bool = False,
                     min_alpha: float = 0.0, return_rays: bool = False, culled: bool = False, **options):
        """PTShadeMixedFrame: render_lightmapped with the direct light of the analytic lights added at every first hit: a light
        moved with update_lights, a deformed mesh's shadow and a point light's highlight show in the next frame without a new
        bake.  Bake inside muted_lights() so that the lights are not counted twice.  Arguments and result as render_lightmapped's;
        culled: PTShadeMixedFrameCulled, through the light grid (direct_light has the conditions)."""
        p = params or self.params(seed=0)
        s, keep = self._shade_inputs(volume, reflections, dfg, **options)           # keep: alive until the call is enqueued
        d = self._direct_params(strata, seed, centered, min_alpha)
        w, h = int(p.OutputWidth), int(p.OutputHeight)
        out, rays = self._device_call(self.lib.PTShadeMixedFrameCulled if culled else self.lib.PTShadeMixedFrame, [C.byref(p), C.byref(s), C.byref(d)],
                                      [((h, w, 4), "float32"), ((h * w, 8), "float32") if return_rays else None])
        return (out, rays) if return_rays else out

    @contextlib.contextmanager
    def muted_lights(self):
        """Inside the block the scene's analytic lights have zero emission (update_lights); on exit the records are restored.
        bake_lightmap, bake_probe_volume and capture_reflection_probes inside it bake sky, emissive surfaces and their bounces
        only: what render_mixed adds the lights to.  The records restored are light_records()'s: lights changed behind this
        layer's back (PTUpdateLights through `lib`) are not known here and come back as they were last sent through update_lights."""
        records = self.light_records()
        if records.shape[0] == 0:
            yield
            return
        muted = records.copy()
        muted[:, 4:7] = 0.0
        self.update_lights(muted)
        try:
            yield
        finally:
            self.update_lights(records)
