"""PathTracer's guides and denoiser, variance across passes and adaptive sampling (include/ptmi_plugin.h Parts 4, 6 and 7)."""
import ctypes as C

import numpy as np

from . import abi, plugin
from ._hostcalls import HostCalls, torch


def _device_to_numpy(ptr: int, shape) -> np.ndarray:
    """Copy float32 device memory at `ptr` into a new numpy array of `shape` (the HIP runtime's hipMemcpy, synchronous)."""
    out = np.empty(shape, dtype=np.float32)
    plugin.hip_memcpy(out.ctypes.data, ptr, out.nbytes, plugin.HIP_MEMCPY_D2H)
    return out


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


class Denoise(HostCalls):
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
        dst = torch.empty((h, w, 4), dtype=torch.float32, device=self._device)
        torch.cuda.synchronize(dst.device)
        plugin.check(fn(self.ctx, C.byref(dp), C.c_void_p(d_src), C.c_void_p(dst.data_ptr())))
        self.synchronize()
        return self._result([dst], as_numpy=True)

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
