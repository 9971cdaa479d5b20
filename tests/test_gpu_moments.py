"""Per-pixel variance across passes (PTAccumulateMoments / PTMeasureNoise / PTDenoiseMoments, include/ptmi_plugin.h Part 6) on the
MI355X.

The moment planes equal the numpy float32 restatement of tests/test_moments.py in every bit; the noise statistics equal its
integer restatement exactly and its float64 sums to the rounding of the kernel's summation layout; the variance-led filter
equals the float64 restatement; and none of it changes what the render computes."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
from test_denoise import random_guides
from test_gpu_denoise import _bits, _check, _converged, _upload_guides
from test_moments import denoise_ref, moments_update, moments_variance, noise_ref

pytestmark = pytest.mark.gpu

SIZES = [(67, 45), (257, 131)]          # neither a multiple of 16 nor of 64
EPS = 2.0 ** -24


def _upload(ptr, a):
    a = np.ascontiguousarray(a, np.float32)
    plugin.hip_memcpy(ptr, a.ctypes.data, a.nbytes, plugin.HIP_MEMCPY_H2D)


def _rel_close(got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):             # inf - inf where both are +inf: those compare equal
        return bool(((got == ref) | (fin & (np.abs(got - ref) <= tol * np.abs(ref)))).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 1: bits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_moments_equal_the_restatement_in_every_bit(size):
    import torch
    W, H = size
    pt = PathTracer(scenes.material_zoo(), width=W, height=H, samplesPerPass=2)
    try:
        assert pt.moments_pointer(0) == 0 and pt.moments_pointer(1) == 0        # nothing allocated before first use
        assert pt.moments_info() == (0, 0, 0, 0)
        frames, planes = [], []
        p0 = p1 = prev = None
        n = 0
        for k in range(6):
            pt._currentSample = n
            p = pt.params(0xA110 + k)
            pt.render_pass(p)
            pt.accumulate_moments(p)
            out = pt.readback(last_output=False)
            p0, p1 = moments_update(p0, p1, out, prev, n, 2)
            g0, g1 = pt.moments()
            assert (_bits(g0) == _bits(p0)).all(), k
            assert (_bits(g1) == _bits(p1)).all(), k
            assert (_bits(g1[..., 3]) == 0).all()
            assert pt.moments_info() == (k + 1, n + 2, W, H)
            assert (_bits(pt.readback(last_output=False)) == _bits(out)).all()  # the Output frame is not modified
            frames.append(out)
            planes.append((p0, p1))
            pt.flip()
            prev, n = out, n + 2
        assert (p0[..., 3] > 0).any() and (p1[..., :3] != 0).any()

        # caller-owned frames: the same passes give the same bits; CurrentSample = 0 resets
        buf = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        n = 0
        for k in range(6):
            pt._currentSample = n
            p = pt.params(0xA110 + k)
            o, a = buf[k % 2], buf[1 - k % 2]
            pt.render_pass_to(p, o.data_ptr(), a.data_ptr() if n else 0)
            pt.accumulate_moments(p, d_output=o.data_ptr(), d_accumulated=a.data_ptr() if n else 0)
            g0, g1 = pt.moments()
            assert (_bits(o.cpu().numpy()) == _bits(frames[k])).all(), k
            assert (_bits(g0) == _bits(planes[k][0])).all() and (_bits(g1) == _bits(planes[k][1])).all(), k
            assert pt.moments_info()[:2] == (k + 1, n + 2)
            n += 2

        # one batch of 3 passes is ONE observation with m = 6
        plugin.check(pt.lib.PTResetFrames(pt.ctx))
        pt._currentSample = 0
        p = pt.params(0xBA7C)
        pt.render_pass(p)
        pt.accumulate_moments(p)
        assert pt.moments_info()[:2] == (1, 2)
        g0, g1 = pt.moments()
        assert (_bits(g0) == 0).all() and (_bits(g1) == 0).all()               # reset
        first = pt.readback(last_output=False)
        pt.flip()
        batch = []
        for j in range(3):
            pt._currentSample = 2 + 2 * j
            batch.append(pt.params(0xBA7D + j))
        arr = (abi.PTFrameParams * 3)(*batch)
        plugin.check(pt.lib.PTRenderPassBatch(pt.ctx, arr, 3))
        pt.accumulate_moments(arr[0], count=3)
        out = pt.readback(last_output=False)
        r0, r1 = moments_update(np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), out, first, 2, 6)
        g0, g1 = pt.moments()
        assert (_bits(g0) == _bits(r0)).all() and (_bits(g1) == _bits(r1)).all()
        assert pt.moments_info()[:2] == (2, 8)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2: continuity and errors
# ---------------------------------------------------------------------------------------------------------------------------
def test_continuity_and_errors():
    W, H = 67, 45
    pt = PathTracer(scenes.cornell_box(), width=W, height=H, samplesPerPass=2)
    lib, err = pt.lib, lambda: pt.lib.PTGetLastError().decode()
    try:
        assert lib.PTGetMomentsPointer(pt.ctx, 0) is None and lib.PTGetMomentsPointer(pt.ctx, 1) is None
        assert lib.PTGetNoiseTilePointer(pt.ctx) is None
        p = pt.params(1)
        pt.render_pass(p)
        for count in (0, 9, -1):
            assert lib.PTAccumulateMoments(pt.ctx, p, count) == abi.PT_ERR_INVALID_ARG and "count" in err()
        pt.accumulate_moments(p)
        assert lib.PTGetMomentsPointer(pt.ctx, 2) is None and lib.PTGetMomentsPointer(pt.ctx, 0) is not None
        # one observation: neither measuring nor denoising
        st, q = abi.noise_stats(), abi.noise_params()
        assert lib.PTMeasureNoise(pt.ctx, q, None, st) == abi.PT_ERR_INVALID_ARG and "2 observations" in err()
        pt.render_guides(1)
        out = np.empty((H, W, 4), np.float32)
        assert lib.PTDenoiseMomentsToHost(pt.ctx, abi.denoise_params(), out.ctypes.data, out.size) == abi.PT_ERR_INVALID_ARG
        assert "2 observations" in err()
        assert lib.PTDenoiseMoments(pt.ctx, abi.denoise_params(), None, pt.frame_pointer(0)) == abi.PT_ERR_INVALID_ARG
        pt.flip()
        # a pass that does not continue the stored sample count: the message names both numbers
        pt._currentSample = 6
        bad = pt.params(2)
        assert lib.PTAccumulateMoments(pt.ctx, bad, 1) == abi.PT_ERR_INVALID_ARG
        assert "6" in err() and " 2 " in err(), err()
        assert pt.moments_info()[:2] == (1, 2)
        # another size
        other = scenes.frame_params(pt.scene, W + 1, H, spp=2, current_sample=2, seed=3)
        buf = np.zeros(16, np.float32)
        assert lib.PTAccumulateMomentsTo(pt.ctx, other, 1, buf.ctypes.data, buf.ctypes.data) == abi.PT_ERR_INVALID_ARG
        assert f"{W}x{H}" in err() and f"{W + 1}x{H}" in err(), err()
        assert lib.PTAccumulateMoments(pt.ctx, other, 1) == abi.PT_ERR_INVALID_ARG
        # the second observation, then the argument checks of PTMeasureNoise
        pt._currentSample = 2
        p = pt.params(4)
        pt.render_pass(p)
        pt.accumulate_moments(p)
        before = pt.readback(last_output=False)
        assert lib.PTMeasureNoise(pt.ctx, q, None, st) == abi.PT_OK and st.observations == 2 and st.samples == 4
        for bad in (abi.noise_params(rel_floor=0.0), abi.noise_params(threshold=-1.0), abi.noise_params(threshold=float("nan")),
                    abi.noise_params(percentile=0.0), abi.noise_params(percentile=1.5), abi.noise_params(percentile=float("nan"))):
            assert lib.PTMeasureNoise(pt.ctx, bad, None, st) == abi.PT_ERR_INVALID_ARG
        short = abi.noise_params()
        short.structSize = 12
        assert lib.PTMeasureNoise(pt.ctx, short, None, st) == abi.PT_ERR_INVALID_ARG and "structSize" in err()
        st_short = abi.noise_stats()
        st_short.structSize = 64
        assert lib.PTMeasureNoise(pt.ctx, q, None, st_short) == abi.PT_ERR_INVALID_ARG and "structSize" in err()
        assert lib.PTMeasureNoise(pt.ctx, None, None, st) == abi.PT_ERR_INVALID_ARG
        assert lib.PTMeasureNoise(pt.ctx, q, None, None) == abi.PT_ERR_INVALID_ARG
        assert lib.PTMeasureNoise(pt.ctx, abi.noise_params(percentile=1.0), None, st) == abi.PT_OK
        # guides of another size than the moments
        pt.render_guides(1, scenes.frame_params(pt.scene, W + 1, H, seed=0))
        wide = np.empty((H, W + 1, 4), np.float32)
        assert lib.PTDenoiseMomentsToHost(pt.ctx, abi.denoise_params(), wide.ctypes.data, wide.size) == abi.PT_ERR_INVALID_ARG
        assert "guides" in err()
        pt.render_guides(1)
        pt.denoise(variance="moments")
        flags = abi.denoise_params()
        flags.flags = 2
        assert lib.PTDenoiseMoments(pt.ctx, flags, None, pt.frame_pointer(0)) == abi.PT_ERR_INVALID_ARG
        assert (_bits(pt.readback(last_output=False)) == _bits(before)).all()      # measuring and denoising write no frame
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3: noise statistics
# ---------------------------------------------------------------------------------------------------------------------------
def _check_stats(st, tiles, r, what):
    assert (np.array(st.histogram[:], np.uint32) == r["histogram"]).all(), what
    assert st.pixels == r["pixels"] and st.pixelsBelow == r["pixelsBelow"], (what, st.pixels, st.pixelsBelow, r["pixels"], r["pixelsBelow"])
    assert int(_bits(np.array([st.maxError]))[0]) == r["maxBits"], what
    assert _bits(np.array([st.percentileError]))[0] == _bits(np.array([r["percentileError"]]))[0], (what, st.percentileError, r["percentileError"])
    # the layout's longest chain of additions: 256 inside a block, then one per block
    assert _rel_close(tiles, r["tiles"], 256 * EPS), what
    assert _rel_close(st.meanError, r["mean"], (256 + tiles.size) * EPS), (what, st.meanError, r["mean"])


@pytest.mark.parametrize("size", SIZES)
def test_noise_statistics(size):
    import torch
    W, H = size
    pt = PathTracer(scenes.material_zoo(), width=W, height=H, samplesPerPass=2, track_noise=True)
    try:
        for k in range(6):
            pt.OnRenderImage(0x5EED + k)
        frame = pt.readback()
        p0, _ = pt.moments()
        st = pt.noise()
        assert (st.structSize, st.observations, st.samples, st.pixels) == (1072, 6, 12, W * H)
        r = noise_ref(frame, p0[..., 3], 6, 12)
        _check_stats(st, pt.noise_tiles(), r, "rendered")
        assert 0 < st.pixelsBelow < st.pixels or st.percentileError > 0
        print(f"[noise] zoo {W}x{H}, 6 x 2 spp: mean {st.meanError:.4f}, p95 <= {st.percentileError:.4f}, max {st.maxError:.4f}, "
              f"{st.pixelsBelow}/{st.pixels} below 2 %")
        st2 = pt.noise()
        assert bytes(st) == bytes(st2)                                   # integer atomics and ordered sums: reproducible
        # other parameters
        st3 = pt.noise(threshold=0.1, percentile=0.5, rel_floor=0.05)
        _check_stats(st3, pt.noise_tiles(), noise_ref(frame, p0[..., 3], 6, 12, 0.05, 0.1, 0.5), "parameters")

        # a synthetic case through the device pointers
        rng = np.random.RandomState(W)
        syn = rng.uniform(0.05, 2.0, (H, W, 4)).astype(np.float32)
        s0 = np.zeros((H, W, 4), np.float32)
        s0[..., 3] = (rng.uniform(0, 1, (H, W)) ** 4 * 10.0).astype(np.float32)
        s0[0, 0, 3] = 0.0                                                # zero variance
        s0[1, 2, 3] = 1e30                                               # a huge variance
        syn[2, 3, :3] = np.nan                                           # a NaN pixel
        syn[H - 1, W - 1, :3] = 0.0                                      # a black pixel (in the partial corner block)
        _upload(pt.moments_pointer(0), s0)
        d_frame = torch.from_numpy(syn).to("cuda:0")
        torch.cuda.synchronize()
        st = pt.noise(d_frame=d_frame.data_ptr())
        r = noise_ref(syn, s0[..., 3], 6, 12)
        assert r["bins"][0, 0] == 0 and r["bins"][1, 2] == 255 and r["bins"][2, 3] == 255
        black = float(np.sqrt(s0[H - 1, W - 1, 3] * np.float32(1.0 / 60.0)) / np.float32(0.01))
        assert 0 < r["bins"][H - 1, W - 1] < 255 and 2.0 ** -24 < black < 240.0
        _check_stats(st, pt.noise_tiles(), r, "synthetic")
        assert np.isinf(st.maxError) and np.isinf(st.meanError) and st.histogram[255] >= 2 and st.histogram[0] >= 1
    finally:
        pt.close()


def test_ownership_adds_up():
    W, H = 67, 45
    s = scenes.material_zoo()
    stats, tiles = [], []
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        pt = PathTracer(s, width=W, height=H, samplesPerPass=2, rank=rank, world_size=world, track_noise=True)
        try:
            for k in range(6):
                pt.OnRenderImage(0x0DD + k)
            stats.append(pt.noise())
            tiles.append(pt.noise_tiles())
        finally:
            pt.close()
    one, r0, r1 = stats
    assert (np.array(r0.histogram[:], np.int64) + np.array(r1.histogram[:], np.int64) == np.array(one.histogram[:], np.int64)).all()
    assert r0.pixels + r1.pixels == one.pixels == W * H and r0.pixels > 0 and r1.pixels > 0
    assert r0.pixelsBelow + r1.pixelsBelow == one.pixelsBelow
    assert max(_bits(np.array([r0.maxError]))[0], _bits(np.array([r1.maxError]))[0]) == _bits(np.array([one.maxError]))[0]
    by, bx = np.mgrid[0:tiles[0].shape[0], 0:tiles[0].shape[1]]
    even = (bx + by) % 2 == 0
    assert (tiles[1][~even] == 0).all() and (tiles[2][even] == 0).all()
    assert (_bits(tiles[1][even]) == _bits(tiles[0][even])).all() and (_bits(tiles[2][~even]) == _bits(tiles[0][~even])).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the filter
# ---------------------------------------------------------------------------------------------------------------------------
def _two_observations(pt, W, H):
    """Allocates the moments at W x H with 2 observations of 1 sample each (invDof = 1 / 2), over throw-away frames."""
    import torch
    a = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    b = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for n in (0, 1):
        p = scenes.frame_params(pt.scene, W, H, spp=1, current_sample=n, seed=0)
        pt.accumulate_moments(p, d_output=a.data_ptr(), d_accumulated=b.data_ptr())
    assert pt.moments_info() == (2, 2, W, H)
    return a, b


@pytest.mark.parametrize("size", SIZES)
def test_filter_matches_restatement(size):
    import torch
    W, H = size
    rng = np.random.RandomState(H)
    pt = PathTracer(scenes.cornell_box(), width=W, height=H)
    try:
        keep = _two_observations(pt, W, H)
        pt.render_guides(1)
        albedo, nd = random_guides(H, W, rng)
        _upload_guides(pt, albedo, nd)
        p0 = (rng.uniform(0, 1, (H, W, 4)) ** 2 * 0.02).astype(np.float32)
        p1 = (rng.uniform(0, 1, (H, W, 4)) ** 2 * 0.01).astype(np.float32)
        p1[..., 3] = 0
        _upload(pt.moments_pointer(0), p0)
        _upload(pt.moments_pointer(1), p1)
        color = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
        d_src = torch.from_numpy(color).to("cuda:0")
        torch.cuda.synchronize()
        for demod in (True, False):
            var = moments_variance(p0, p1, albedo, 2, 2, demod)
            for it in (1, 3, 5):
                dp = abi.denoise_params(iterations=it, demodulate=demod)
                got = pt.denoise(dp, d_src=d_src.data_ptr(), variance="moments")
                _check(got, denoise_ref(color, albedo, nd, it, demodulate=demod, variance=var), (size, demod, it))
                bg = albedo[..., 3] == 0
                assert (_bits(got[bg]) == _bits(color[bg])).all()
                assert (_bits(got[..., 3]) == _bits(color[..., 3])).all()
        assert (_bits(d_src.cpu().numpy()) == _bits(color)).all()
        got = pt.denoise(abi.denoise_params(iterations=0), d_src=d_src.data_ptr(), variance="moments")
        assert (_bits(got) == _bits(color)).all()
        # "auto": fewer than 4 observations -> the spatial estimate
        a = pt.denoise(d_src=d_src.data_ptr(), variance="auto")
        b = pt.denoise(d_src=d_src.data_ptr())
        assert (_bits(a) == _bits(b)).all()
        del keep
    finally:
        pt.close()


def test_a_converged_frame_is_left_alone():
    """All moments zero and neighbouring filter luminances at least 1e-3 apart: every foreign tap weighs exp(-1000) = 0, so the
    output is the input up to the roundings of demodulate, (w e) / w per level and remodulate (at most 12 x 2^-24 < 1e-6); the
    spatial estimate blurs the same input."""
    import torch
    W, H = 67, 45
    rng = np.random.RandomState(11)
    pt = PathTracer(scenes.cornell_box(), width=W, height=H)
    try:
        keep = _two_observations(pt, W, H)
        pt.render_guides(1)
        albedo, nd = random_guides(H, W, rng)
        _upload_guides(pt, albedo, nd)
        lum = (0.5 + 2e-3 * rng.permutation(W * H).reshape(H, W)).astype(np.float32)       # demodulated luminances, all distinct
        color = np.ones((H, W, 4), np.float32)
        color[..., :3] = lum[..., None] * np.maximum(albedo[..., :3], np.float32(1e-3))
        d_src = torch.from_numpy(color).to("cuda:0")
        torch.cuda.synchronize()
        assert (_bits(pt.moments()[0]) == 0).all()
        got = pt.denoise(d_src=d_src.data_ptr(), variance="moments")
        rel = np.abs(got.astype(np.float64) - color) / np.abs(color)
        assert rel.max() <= 1e-6, float(rel.max())
        spatial = pt.denoise(d_src=d_src.data_ptr())
        assert np.abs(spatial - color).max() > 1e-2
        del keep
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5: quality against a converged render
# ---------------------------------------------------------------------------------------------------------------------------
def test_quality_against_a_converged_render():
    """Cornell box and material zoo, 128x128, 16 tracked passes of 4 spp against 2048 spp, MSE after x / (1 + x).  Asserted: the
    moments-led result is no worse than the noisy frame; the three figures are printed.  Whether the
    moments-led result beats the spatial estimate at this sample count is not asserted."""
    for name, make in (("cornell", scenes.cornell_box), ("zoo", scenes.material_zoo)):
        s = make()
        ref = _converged(s, 1000)
        pt = PathTracer(s, width=128, height=128, samplesPerPass=4, track_noise=True)
        try:
            for k in range(16):
                pt.OnRenderImage(77 + k)
            noisy = pt.readback()
            pt.render_guides(4)
            # OnRenderImage flipped: the frame last accumulated (what PTDenoiseMoments reads by default) is the other one
            plugin.check(pt.lib.PTFlipFrames(pt.ctx))
            frame = pt.frame_pointer(-1)
            plugin.check(pt.lib.PTFlipFrames(pt.ctx))
            spatial = pt.denoise(d_src=frame)
            moments = pt.denoise(variance="moments")
            assert (_bits(pt.denoise(d_src=frame, variance="moments")) == _bits(moments)).all()
            assert pt.moments_info()[:2] == (16, 64)
        finally:
            pt.close()

        def mse(a):
            t = lambda x: np.maximum(x[..., :3].astype(np.float64), 0) / (1 + np.maximum(x[..., :3].astype(np.float64), 0))
            return float(np.mean((t(a) - t(ref)) ** 2))
        m_noisy, m_spatial, m_moments = mse(noisy), mse(spatial), mse(moments)
        print(f"[quality] {name} 16 x 4 spp: MSE noisy {m_noisy:.3e}, PTDenoise {m_spatial:.3e} ({m_spatial / m_noisy:.3f}x), "
              f"PTDenoiseMoments {m_moments:.3e} ({m_moments / m_noisy:.3f}x)")
        assert m_moments <= m_noisy, (name, m_moments, m_noisy)


# ---------------------------------------------------------------------------------------------------------------------------
# 6: no effect on rendering; render_until
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_no_effect_on_rendering(name):
    s = scenes.cornell_box() if name == "cornell" else scenes.material_zoo()
    W, H = 64, 48
    frames, stats = [], []
    for interleave in (True, False):
        pt = PathTracer(s, width=W, height=H, samplesPerPass=2, track_noise=interleave)
        pt.set_stats_level(1)
        try:
            if interleave:
                pt.render_guides(1)
            for k in range(4):
                pt.OnRenderImage(0xBEEF + k)
                if interleave and k >= 1:
                    pt.noise()
                    pt.denoise(variance="moments")
            pt.synchronize()
            frames.append(pt.readback())
            stats.append(bytes(pt.stats()))
        finally:
            pt.close()
    assert (_bits(frames[0]) == _bits(frames[1])).all()
    assert stats[0] == stats[1]


def test_render_until_stops_at_the_first_check_below_the_target():
    """The material zoo, 2 spp a pass, a check every 2 passes.  The edges of a plain tracked 16-pass run give the targets: for the
    95th percentile (the issue's criterion) and for the median.  The 95th percentile of a path-traced frame is held up by the
    pixels whose light arrives in rare samples (their relative error stays near 1 until a second such sample arrives), so it need
    not fall from one check to the next; whatever it does, the target is set just above the first minimum of the sequence, which
    by construction is the first check below it.  The median falls as 1/sqrt(samples): from 4 to 32 samples that is a factor
    2.8, twelve eighth-octave bins, so some later check is below every check before it and the stop is not at the first check."""
    W, H = 67, 45
    s = scenes.material_zoo()
    QS = (0.95, 0.5)
    pt = PathTracer(s, width=W, height=H, samplesPerPass=2, track_noise=True)
    try:
        edges = {q: [] for q in QS}
        for k in range(16):
            pt.OnRenderImage(40 + k)
            if k % 2 == 1:
                for q in QS:
                    edges[q].append(float(pt.noise(percentile=q).percentileError))
        print(f"[render_until] edges at every check: {edges}")
        got = {}
        for q in QS:
            E = edges[q]
            j = next((i for i in range(1, len(E)) if E[i] < min(E[:i])), 0)     # the first check that improves on all before it
            if q == 0.5:
                assert j >= 1, E
            target = E[j] * 1.0001                                              # edges are an eighth of an octave apart
            assert all(e >= target for e in E[:j]) and E[j] < target
            passes, st = pt.render_until(target, percentile=q, seed0=40, check_every=2, max_samples=64)
            assert passes == 2 * (j + 1), (q, passes, j, E)
            assert st.percentileError == E[j] and st.observations == passes and st.samples == 2 * passes
            got[passes] = pt.readback()
        # a target nothing reaches: stops at max_samples
        passes_all, _ = pt.render_until(1e-9, seed0=40, check_every=4, max_samples=16)
        assert passes_all == 8
    finally:
        pt.close()
    plain = PathTracer(s, width=W, height=H, samplesPerPass=2)
    try:
        for k in range(max(got)):
            plain.OnRenderImage(40 + k)
            if k + 1 in got:
                assert (_bits(plain.readback()) == _bits(got[k + 1])).all(), k + 1
    finally:
        plain.close()
