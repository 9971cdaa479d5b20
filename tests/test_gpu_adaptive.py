"""Adaptive sampling (PTAdaptiveBegin / PTSetActiveBlocks / PTRenderPassActive / PTAccumulateMomentsActive, include/ptmi_plugin.h
Part 7) on the MI355X.

The contract is bit-exact and the tests hold it without tolerances: with every block active and equal counts the frame is
PTRenderPassBatch's; in general it is a per-block composite of oracle frames, one per distinct sample count; pixels that are not
rendered equal Accumulated in every bit; the moment planes equal the float32 restatement with one factor per block."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer, select_blocks
from test_gpu_denoise import _bits
from test_gpu_moments import _check_stats
from test_moments import bin_edge, lum32, moments_update

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 40, 24, 2, 3           # 3 x 2 blocks, the last column 8 px wide, the last row 8 px high
COLS, ROWS = 3, 2
SCENES = {"cornell": scenes.cornell_box, "instanced": scenes.instanced_scene}        # flat, HAS_TLAS
SEED = 0xADA0


def _tracer(name="cornell", schedule=1, w=W, h=H, **kw):
    return PathTracer(SCENES[name](), width=w, height=h, samplesPerPass=SPP, maxRayBounces=BOUNCES, schedule=schedule, **kw)


def _block_mask(ids, w=W, h=H):
    """(h, w) bool: the pixels of the listed 16x16 blocks."""
    cols = (w + 15) // 16
    m = np.zeros((h, w), bool)
    for b in ids:
        by, bx = divmod(int(b), cols)
        m[by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = True
    return m


class Composite:
    """The contract restated through the oracle: the frame and the per-block counts after uniform and adaptive steps."""

    def __init__(self, oracle, pt, cover=None):
        self.oracle, self.pt = oracle, pt
        self.b = oracle.buffers_from_bvhscene(pt._bvhScene)
        self.rows, self.cols = pt.block_grid()
        self.n = np.zeros((self.rows, self.cols), np.uint32)
        self.frame = None
        self.cover = cover

    def _params(self, seed, n):
        was, self.pt._currentSample = self.pt._currentSample, int(n)
        try:
            return self.pt.params(seed)
        finally:
            self.pt._currentSample = was

    def uniform(self, seed):
        n = int(self.n.flat[0])
        self.frame, _ = self.oracle.render(self.b, self._params(seed, n), accumulated=self.frame)
        self.n += SPP
        return self.frame

    def active(self, ids, seeds):
        """One adaptive call: one oracle chain per distinct count among the listed blocks, composited per block."""
        new = self.frame.copy()
        flat = self.n.reshape(-1)
        for n in sorted({int(flat[b]) for b in ids}):
            f = self.frame
            for j, s in enumerate(seeds):
                f, _ = self.oracle.render(self.b, self._params(s, n + j * SPP), accumulated=f)
            m = _block_mask([b for b in ids if int(flat[b]) == n], self.pt.width, self.pt.height)
            if self.cover:
                m[:, self.cover[0]:] = False
                m[self.cover[1]:, :] = False
            new[m] = f[m]
        for b in ids:
            flat[b] += SPP * len(seeds)
        self.frame = new
        return new


def _step(pt, ids, seeds, moments=False):
    """set the list, render, (record the observation,) read Output and Accumulated back, flip"""
    kept = pt.set_active_blocks(ids)
    pt.render_active(seeds)
    if moments:
        pt.accumulate_moments_active(len(seeds))
    out = pt.readback(last_output=False)
    pt.flip()
    acc = pt.readback(last_output=False)
    pt.flip()
    pt.flip()
    return kept, out, acc


# the sequence of consequence (b): two uniform passes, {1, 4} twice, {0, 1, 5} -- the last call mixes the counts of blocks rendered
# before and not, and includes block 5, partial both ways -- and one more call with four different counts in one launch
SEQUENCE = [([1, 4], 1), ([1, 4], 2), ([0, 1, 5], 1), ([0, 1, 2, 4], 2)]


# ---------------------------------------------------------------------------------------------------------------------------
# (a): every block active, equal counts -> PTRenderPassBatch, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [1, 2, 3])
@pytest.mark.parametrize("name", list(SCENES))
def test_all_blocks_active_is_the_batch(name, schedule):
    seeds = [SEED + 10, SEED + 11, SEED + 12]
    frames, stats = [], []
    for adaptive in (True, False):
        pt = _tracer(name, schedule)
        try:
            pt.OnRenderImage(SEED)
            pt.OnRenderImage(SEED + 1)
            pt.synchronize()
            pt.reset_stats()
            if adaptive:
                pt.adaptive_begin()
                assert pt.active_blocks().tolist() == list(range(6))
                assert (pt.block_samples() == 4).all() and pt.block_samples().shape == (ROWS, COLS)
                pt.render_active(seeds)
                assert (pt.block_samples() == 10).all()
            else:
                batch = []
                for j, s in enumerate(seeds):
                    pt._currentSample = 4 + j * SPP
                    batch.append(pt.params(s))
                plugin.check(pt.lib.PTRenderPassBatch(pt.ctx, (abi.PTFrameParams * 3)(*batch), 3))
            frames.append(pt.readback(last_output=False))
            st = pt.stats()
            stats.append((st.paths, st.rays, st.pixelsWritten, st.pixelsRead))
        finally:
            pt.close()
    assert (_bits(frames[0]) == _bits(frames[1])).all(), (name, schedule)
    assert stats[0] == stats[1], (stats, name, schedule)
    assert stats[0][0] == W * H * SPP * 3


# ---------------------------------------------------------------------------------------------------------------------------
# (b): the per-block composite of oracle frames; inactive pixels; PTGetBlockSamples; PTStats.paths
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [1, 2, 3])
@pytest.mark.parametrize("name", list(SCENES))
def test_block_lists_give_the_oracle_composite(oracle, name, schedule):
    pt = _tracer(name, schedule)
    try:
        ref = Composite(oracle, pt)
        for k in range(2):
            pt.OnRenderImage(SEED + k)
            ref.uniform(SEED + k)
        assert (_bits(pt.readback()) == _bits(ref.frame)).all()
        pt.adaptive_begin()
        seed = SEED + 100
        for ids, count in SEQUENCE:
            seeds = [seed + j for j in range(count)]
            seed += count
            before = ref.frame
            paths0 = pt.stats().paths
            kept, out, acc = _step(pt, ids, seeds)
            want = ref.active(ids, seeds)
            assert kept == len(ids)
            assert (_bits(acc) == _bits(before)).all()
            assert (_bits(out) == _bits(want)).all(), (name, schedule, ids, int((_bits(out) != _bits(want)).any(axis=-1).sum()))
            inactive = ~_block_mask(ids)
            assert (_bits(out[inactive]) == _bits(acc[inactive])).all()
            assert (_bits(out[~inactive]) != _bits(acc[~inactive])).any()
            assert (pt.block_samples() == ref.n).all(), (pt.block_samples(), ref.n)
            assert pt.stats().paths - paths0 == int(_block_mask(ids).sum()) * SPP * count
        assert len(set(ref.n.reshape(-1).tolist())) >= 4
    finally:
        pt.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_single_blocks_and_the_empty_list(oracle, name):
    pt = _tracer(name, 1)
    try:
        ref = Composite(oracle, pt)
        pt.OnRenderImage(SEED)
        ref.uniform(SEED)
        pt.adaptive_begin()
        for k, b in enumerate((0, 5)):                      # a full block, and the one that is partial both ways
            kept, out, acc = _step(pt, [b], [SEED + 20 + k])
            want = ref.active([b], [SEED + 20 + k])
            assert kept == 1 and (_bits(out) == _bits(want)).all(), b
            assert (_bits(out[~_block_mask([b])]) == _bits(acc[~_block_mask([b])])).all()
        paths0 = pt.stats().paths
        kept, out, acc = _step(pt, [], [SEED + 30])
        assert kept == 0 and pt.active_blocks().size == 0
        assert (_bits(out) == _bits(acc)).all() and (_bits(out) == _bits(ref.frame)).all()
        assert pt.stats().paths == paths0
        assert (pt.block_samples() == ref.n).all()
        # None = every block again
        assert pt.set_active_blocks(None) == 6 and pt.active_blocks().tolist() == list(range(6))
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# passes in flight
# ---------------------------------------------------------------------------------------------------------------------------
def test_calls_in_flight_give_the_bytes_of_synchronised_calls():
    def run(sync):
        pt = _tracer("instanced", 1)
        try:
            pt.OnRenderImage(SEED)
            pt.adaptive_begin()
            for k, ids in enumerate(([0, 1, 4], [1, 2, 4, 5], [0, 5])):
                pt.set_active_blocks(ids)
                pt.render_active([SEED + 40 + 2 * k, SEED + 41 + 2 * k])
                if sync:
                    pt.synchronize()
                pt.flip()
            pt.flip()
            return pt.readback(last_output=False).tobytes(), pt.block_samples().tobytes()
        finally:
            pt.close()
    a, b, c = run(False), run(True), run(False)
    assert a == b and a == c


# ---------------------------------------------------------------------------------------------------------------------------
# ownership and dispatch coverage
# ---------------------------------------------------------------------------------------------------------------------------
def test_ownership_adds_up():
    frames, kept = [], []
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        pt = _tracer("cornell", 1, rank=rank, world_size=world)
        try:
            pt.OnRenderImage(SEED)
            pt.adaptive_begin()
            kept.append(pt.set_active_blocks([0, 1, 2, 4]))
            own = [b for b in (0, 1, 2, 4) if (b % COLS + b // COLS) % world == rank]
            assert pt.active_blocks().tolist() == own
            pt.render_active([SEED + 50, SEED + 51])
            frames.append(pt.readback(last_output=False))
            want = np.full(6, 2, np.uint32)
            want[own] = 6
            assert (pt.block_samples().reshape(-1) == want).all()
        finally:
            pt.close()
    assert kept == [4, 3, 1]                                 # blocks 0, 2 and 4 are rank 0's, block 1 rank 1's
    assert (_bits(frames[1] + frames[2]) == _bits(frames[0])).all()
    even = _block_mask([0, 2, 4])
    assert (frames[1][~even] == 0).all() and (frames[2][even] == 0).all()


def test_dispatch_coverage_leaves_the_edge_pixels(oracle):
    import torch
    w, h = 44, 28                                           # reference dispatch: 5 x 3 groups of 8 cover 40 x 24
    pt = _tracer("cornell", 1, w=w, h=h, reference_dispatch=True)
    try:
        rng = np.random.RandomState(5)
        pattern = rng.uniform(0.1, 1.0, (h, w, 4)).astype(np.float32)
        acc = torch.from_numpy(pattern).to("cuda:0")
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        pt._currentSample = 2
        pt.adaptive_begin()
        assert pt.set_active_blocks(None) == 6
        pt.render_active([SEED + 60], d_output=out.data_ptr(), d_accumulated=acc.data_ptr())
        pt.synchronize()
        got = out.cpu().numpy()
        ref = Composite(oracle, pt, cover=(40, 24))
        ref.frame, ref.n[:] = pattern, 2
        want = ref.active(list(range(6)), [SEED + 60])
        assert (_bits(got) == _bits(want)).all()
        assert (_bits(got[:, 40:]) == _bits(pattern[:, 40:])).all() and (_bits(got[24:]) == _bits(pattern[24:])).all()
        assert (_bits(got[:24, :40, :3]) != _bits(pattern[:24, :40, :3])).any()
        assert pt.stats().paths == 40 * 24 * SPP
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# moments, noise and the variance-led filter with per-block counts
# ---------------------------------------------------------------------------------------------------------------------------
def _noise_ref_blocks(frame, sll, k, wsum, rel_floor=0.01, threshold=0.02, percentile=0.95):
    """tests/test_moments.py noise_ref with invDof_b = (float)(1.0 / ((k_b - 1) W_b)) per block."""
    import math
    f32 = np.float32
    h, w = frame.shape[:2]
    inv_b = np.array([[f32(1.0 / (float(k[y, x] - 1) * float(wsum[y, x]))) for x in range(k.shape[1])] for y in range(k.shape[0])], f32)
    inv = np.repeat(np.repeat(inv_b, 16, 0), 16, 1)[:h, :w]
    with np.errstate(all="ignore"):
        eps = np.sqrt(np.asarray(sll, f32) * inv) / (lum32(frame) + f32(rel_floor))
    eps = np.where(eps >= 0, eps, f32(np.inf)).astype(f32)
    bits = eps.view(np.uint32) & np.uint32(0x7FFFFFFF)
    eps = bits.view(f32)
    bins = np.clip((bits >> 20).astype(np.int64) - ((127 - 24) << 3), 0, 255)
    hist = np.bincount(bins.reshape(-1), minlength=256).astype(np.uint32)
    tiles = np.array([[eps[y * 16:y * 16 + 16, x * 16:x * 16 + 16].astype(np.float64).mean() for x in range(k.shape[1])] for y in range(k.shape[0])])
    target = math.ceil(float(f32(percentile)) * eps.size)
    edge = bin_edge(int(np.argmax(np.cumsum(hist.astype(np.int64)) >= target)))
    return {"histogram": hist, "pixels": eps.size, "pixelsBelow": int((eps <= f32(threshold)).sum()), "maxBits": int(bits.max()),
            "mean": float(eps.astype(np.float64).mean()), "tiles": tiles, "percentileError": edge}


@pytest.mark.parametrize("name", list(SCENES))
def test_moments_per_block_equal_the_restatement(name):
    pt = _tracer(name, 1, track_noise=True)
    try:
        p0 = p1 = prev = None
        for k in range(2):
            pt.OnRenderImage(SEED + k)
            out = pt.readback()
            p0, p1 = moments_update(p0, p1, out, prev, k * SPP, SPP)
            prev = out
        pt.adaptive_begin()
        n = np.full(6, 4, np.int64)
        obs, wsum = np.full(6, 2, np.int64), np.full(6, 4, np.int64)
        seed = SEED + 100
        for ids, count in SEQUENCE:
            seeds = [seed + j for j in range(count)]
            seed += count
            _, out, acc = _step(pt, ids, seeds, moments=True)
            m = SPP * count
            q0, q1 = p0.copy(), p1.copy()
            for b in ids:                                   # one factor f_b per block, from its count before the call
                r0, r1 = moments_update(p0, p1, out, acc, int(n[b]), m)
                mask = _block_mask([b])
                q0[mask], q1[mask] = r0[mask], r1[mask]
            g0, g1 = pt.moments()
            assert (_bits(g0) == _bits(q0)).all() and (_bits(g1) == _bits(q1)).all(), (ids, count)
            off = ~_block_mask(ids)
            assert (_bits(g0[off]) == _bits(p0[off])).all() and (_bits(g1[off]) == _bits(p1[off])).all()
            p0, p1 = q0, q1
            n[ids] += m
            obs[ids] += 1
            wsum[ids] += m
            assert pt.moments_info()[:2] == (int(obs.min()), int(wsum.min()))
        assert len(set(obs.tolist())) >= 3
        frame = out
        st = pt.noise()
        assert (st.observations, st.samples, st.pixels) == (int(obs.min()), int(wsum.min()), W * H)
        r = _noise_ref_blocks(frame, p0[..., 3], obs.reshape(ROWS, COLS), wsum.reshape(ROWS, COLS))
        _check_stats(st, pt.noise_tiles(), r, name)
        # the host-side selection reads this tile map
        tiles = pt.noise_tiles()
        thr = float(np.sort(tiles.reshape(-1))[2])
        for dilate in (False, True):
            want = select_blocks(tiles, n.reshape(ROWS, COLS), thr, 16, 4, dilate)
            assert pt.select_active_blocks(thr, 16, 4, dilate) == want.size
            assert pt.active_blocks().tolist() == want.tolist()
        # the global call is refused while the state is live; after PTAdaptiveEnd it is the adaptive calls that are
        p = pt.params(1)
        assert pt.lib.PTAccumulateMoments(pt.ctx, p, 1) == abi.PT_ERR_INVALID_ARG
        assert "adaptive" in pt.lib.PTGetLastError().decode()
    finally:
        pt.close()


def test_filter_with_equal_counts_is_the_scalar_path():
    """All n_b equal: the per-block table holds one value, the scalar's -- PTDenoiseMoments gives the bits of a context whose
    moments were built by uniform passes."""
    results = []
    for adaptive in (True, False):
        pt = _tracer("cornell", 1, track_noise=True)
        try:
            for k in range(2):
                pt.OnRenderImage(SEED + k)
            if adaptive:
                pt.adaptive_begin()
                for k in range(2, 4):
                    pt.render_active([SEED + k])
                    pt.accumulate_moments_active(1)
                    pt.flip()
                pt._flipped = True
            else:
                for k in range(2, 4):
                    pt.OnRenderImage(SEED + k)
            assert pt.moments_info() == (4, 8, W, H)
            pt.render_guides(1)
            st = pt.noise()
            results.append((pt.readback(), pt.moments(), pt.denoise(variance="moments"), bytes(st), pt.noise_tiles()))
        finally:
            pt.close()
    a, b = results
    assert (_bits(a[0]) == _bits(b[0])).all()
    assert (_bits(a[1][0]) == _bits(b[1][0])).all() and (_bits(a[1][1]) == _bits(b[1][1])).all()
    assert (_bits(a[2]) == _bits(b[2])).all()
    assert a[3] == b[3] and (_bits(a[4]) == _bits(b[4])).all()
    assert (_bits(a[2]) != _bits(a[0])).any()              # the filter did something


# ---------------------------------------------------------------------------------------------------------------------------
# render_adaptive
# ---------------------------------------------------------------------------------------------------------------------------
def test_render_adaptive_stops_block_by_block(oracle):
    w = h = 64
    MIN, MAX, ROUND = 8, 24, 2
    pt = _tracer("cornell", 1, w=w, h=h, track_noise=True)
    try:
        # the target: the median of the tile map after the uniform phase, so the first round selects some blocks and not all
        for k in range(4):
            pt.OnRenderImage(SEED + k)
        pt.noise()
        tiles0 = pt.noise_tiles()
        target = float(np.median(tiles0))
        assert tiles0.min() < target < tiles0.max()
        history = []
        samples, st = pt.render_adaptive(target, MIN, MAX, seed0=SEED, passes_per_round=ROUND, dilate=False, history=history)
        assert samples.shape == (4, 4) and samples.min() >= MIN and samples.max() <= MAX
        assert len(set(samples.reshape(-1).tolist())) > 1, samples
        assert select_blocks(pt.noise_tiles(), samples, target, MAX, SPP * ROUND, False).size == 0
        assert st.observations >= 4
        got = pt.readback()
        ref = Composite(oracle, pt)
        for rec in history:
            if rec[0] == "uniform":
                ref.uniform(rec[1])
            else:
                ref.active(rec[1].tolist(), rec[2])
        assert [r[0] for r in history[:4]] == ["uniform"] * 4 and history[4][0] == "active"
        assert (ref.n == samples).all()
        assert (_bits(got) == _bits(ref.frame)).all()
        print(f"[render_adaptive] cornell 64x64, target {target:.4f}: samples per block\n{samples}")
        pt.render_guides(1)
        assert pt.denoise(variance="auto").shape == (h, w, 4)           # the filter keeps working afterwards
    finally:
        pt.close()


def test_equal_budget_quality_is_printed(oracle):
    """Cornell 48x48 against the 2048-spp oracle frame of tests/test_moments.py (32 passes of 64 spp, seeds 1000...), MSE after
    x / (1 + x): an adaptive run and a uniform run of the same number of paths.  Printed, not asserted: stopping on an estimated
    variance is biased by construction, and nobody has measured by how much here."""
    s = scenes.cornell_box()
    w = h = 48
    pt = PathTracer(s, width=w, height=h, samplesPerPass=4, schedule=1)
    try:
        b = oracle.buffers_from_bvhscene(pt._bvhScene)
        ref, n = None, 0
        for k in range(32):
            ref, _ = oracle.render(b, scenes.frame_params(s, w, h, spp=64, current_sample=n, seed=1000 + k), accumulated=ref)
            n += 64
        pt.render_adaptive(0.03, 16, 128, seed0=77, passes_per_round=2)
        samples = pt.block_samples()
        adaptive = pt.readback()
        budget = int((samples.astype(np.int64) * 256).sum())
        passes = max(1, round(budget / (w * h * 4)))
        pt.adaptive_end()
        pt.Reset()
        for k in range(passes):
            pt.OnRenderImage(77 + k)
        uniform = pt.readback()
    finally:
        pt.close()

    def mse(a):
        t = lambda x: np.maximum(x[..., :3].astype(np.float64), 0) / (1 + np.maximum(x[..., :3].astype(np.float64), 0))
        return float(np.mean((t(a) - t(ref)) ** 2))
    print(f"[adaptive quality] cornell 48x48: adaptive {budget} paths (blocks {samples.min()}..{samples.max()} spp) MSE {mse(adaptive):.3e}; "
          f"uniform {passes} x 4 spp = {passes * 4 * w * h} paths MSE {mse(uniform):.3e}")
    assert np.isfinite(adaptive).all() and np.isfinite(uniform).all()


# ---------------------------------------------------------------------------------------------------------------------------
# errors: refused on the host, before any launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_error_behaviour():
    pt = _tracer("cornell", 1)
    lib, err = pt.lib, lambda: pt.lib.PTGetLastError().decode()
    INV, UNS = abi.PT_ERR_INVALID_ARG, abi.PT_ERR_UNSUPPORTED
    try:
        p = pt.params(1)
        arr = (abi.PTFrameParams * 1)(p)
        n = C.c_uint32()
        ids = (C.c_uint32 * 8)()
        # no PTAdaptiveBegin
        for rc in (lib.PTRenderPassActive(pt.ctx, arr, 1), lib.PTSetActiveBlocks(pt.ctx, None, 0, C.byref(n)),
                   lib.PTGetActiveBlocks(pt.ctx, ids, 8, C.byref(n)), lib.PTGetBlockSamples(pt.ctx, ids, 8),
                   lib.PTAccumulateMomentsActive(pt.ctx, p, 1),
                   lib.PTSelectActiveBlocks(pt.ctx, abi.adaptive_select(0.1, 8, 2), C.byref(n))):
            assert rc == INV and "PTAdaptiveBegin" in err(), err()
        pt.OnRenderImage(SEED)
        pt.adaptive_begin()
        paths0 = pt.stats().paths
        # another frame size: both sizes named
        other = scenes.frame_params(pt.scene, W + 1, H, spp=SPP, seed=3)
        assert lib.PTRenderPassActive(pt.ctx, (abi.PTFrameParams * 1)(other), 1) == INV
        assert f"{W}x{H}" in err() and f"{W + 1}x{H}" in err(), err()
        # ids not strictly ascending, out of range
        for bad, words in (([0, 2, 2], ("2", "index 2")), ([3, 1], ("3", "1")), ([0, 6], ("6", "6 blocks"))):
            a = (C.c_uint32 * len(bad))(*bad)
            assert lib.PTSetActiveBlocks(pt.ctx, a, len(bad), C.byref(n)) == INV
            assert all(x in err() for x in words), err()
        assert pt.active_blocks().tolist() == list(range(6))            # a refused list changes nothing
        # count outside 1..8
        for count in (0, 9, -1):
            big = (abi.PTFrameParams * 9)(*[p] * 9)
            assert lib.PTRenderPassActive(pt.ctx, big, count) == INV and "count" in err() and str(count) in err(), err()
        # dOutput == dAccumulated; NULL accumulated with samples present
        f0 = pt.frame_pointer(0)
        assert lib.PTRenderPassActiveTo(pt.ctx, arr, 1, f0, f0) == INV and "dAccumulated" in err()
        assert lib.PTRenderPassActiveTo(pt.ctx, arr, 1, f0, None) == INV and "NULL" in err()
        # passes that differ in more than the seed
        two = (abi.PTFrameParams * 2)(p, scenes.frame_params(pt.scene, W, H, spp=SPP, seed=1, max_bounces=2))
        assert lib.PTRenderPassActive(pt.ctx, two, 2) == INV
        # n_b + m past 2^32
        pt.adaptive_begin(current_sample=0xFFFFFFFF - 3)
        four = (abi.PTFrameParams * 4)(*[p] * 4)
        assert lib.PTRenderPassActive(pt.ctx, four, 4) == INV
        assert str(0xFFFFFFFF - 3) in err() and " 8 " in err(), err()
        pt.adaptive_begin(current_sample=2)
        # moments: none tracked at PTAdaptiveBegin
        pt.render_active([5])
        assert lib.PTAccumulateMomentsActive(pt.ctx, p, 1) == INV and "moments" in err()
        # a short structSize
        sel = abi.adaptive_select(0.1, 8, 2)
        sel.structSize = 16
        assert lib.PTSelectActiveBlocks(pt.ctx, sel, C.byref(n)) == INV and "structSize" in err() and "16" in err() and "20" in err()
        assert lib.PTSelectActiveBlocks(pt.ctx, abi.adaptive_select(0.1, 8, 2), C.byref(n)) == INV and "PTMeasureNoise" in err()
        # capacity
        assert lib.PTGetBlockSamples(pt.ctx, ids, 5) == INV and "5" in err() and "6" in err()
        assert lib.PTGetActiveBlocks(pt.ctx, ids, 2, C.byref(n)) == INV and n.value == 6
        # schedules 0 and 4
        for schedule in (0, 4):
            pt.set_schedule(schedule)
            assert lib.PTRenderPassActive(pt.ctx, arr, 1) == UNS and str(schedule) in err(), err()
        pt.set_schedule(1)
        pt.synchronize()
        assert pt.stats().paths - paths0 == W * H * SPP                 # only the one accepted call rendered
        # the global moments call while adaptive state is live
        assert lib.PTAccumulateMoments(pt.ctx, p, 1) == INV and "adaptive" in err()
        pt.adaptive_end()
        assert lib.PTRenderPassActive(pt.ctx, arr, 1) == INV and "PTAdaptiveBegin" in err()
        assert lib.PTAdaptiveEnd(pt.ctx) == abi.PT_OK                   # idempotent
    finally:
        pt.close()


def test_moments_call_must_describe_the_call_just_enqueued():
    pt = _tracer("cornell", 1, track_noise=True)
    lib, err = pt.lib, lambda: pt.lib.PTGetLastError().decode()
    try:
        pt.OnRenderImage(SEED)
        pt.OnRenderImage(SEED + 1)
        pt.adaptive_begin()
        p = pt.params(1)
        assert lib.PTAccumulateMomentsActive(pt.ctx, p, 1) == abi.PT_ERR_INVALID_ARG and " 0" in err()       # nothing enqueued yet
        pt.render_active([7, 8])
        assert lib.PTAccumulateMomentsActive(pt.ctx, p, 1) == abi.PT_ERR_INVALID_ARG and "2" in err() and "4" in err(), err()
        assert lib.PTAccumulateMomentsActive(pt.ctx, p, 2) == abi.PT_OK
        assert lib.PTAccumulateMomentsActive(pt.ctx, p, 2) == abi.PT_ERR_INVALID_ARG                          # one observation per call
        assert pt.moments_info()[:2] == (3, 8)
    finally:
        pt.close()
