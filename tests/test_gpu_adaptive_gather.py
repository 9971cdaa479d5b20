"""Adaptive gathers (PTGatherIrradianceAdaptive and its steps / PathTracer.irradiance_adaptive / bake_lightmap(adaptive=...),
include/ptmi_plugin.h Part 19) on the MI355X.

The step kernels are held to the host twins byte for byte (the twins to the numpy restatement by tests/test_adaptive_gather.py) on
the lists of adaptive_gather_cases.py.  The loop is held to its contract: (out[i], counts[i]) is what the numpy select and fold make
of plain irradiance() results of the same receivers over the same sample ranges, bit for bit -- which catches a wrong compaction
order, a wrong sample range and a fold with a fused multiply-add.  Only the last statement compares against something else: a
4,096-sample gather of the same receivers."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import adaptive_gather_cases as cases
import adaptive_gather_ref as ref
import chart_cases

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL_F, SENTINEL_U = 7.25, 0xABCDEF01
PARAMS = dict(threshold=cases.THRESHOLD, min_samples=cases.N, add_samples=cases.ADD, max_samples=cases.MAX, dark_floor=cases.DARK_FLOOR)
W = H = 48
MIN, ADD, MAX = 8, 8, 40


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return
    diff = np.nonzero((_bits(got) != _bits(want)).reshape(len(got), -1).any(axis=1))[0]
    assert len(diff) == 0, (what, len(diff), len(want), diff[:3], got[diff[:3]], want[diff[:3]])


@pytest.fixture(scope="module")
def box():
    scene = chart_cases.lit_box()
    pt = PathTracer(scene, width=32, height=32, samplesPerPass=1, maxRayBounces=3, schedule=1)
    yield pt, chart_cases.floor_only_uvs(len(scene.tri_attrs))
    pt.close()


def _dev(pt):
    import torch
    return torch.device(f"cuda:{pt.device}")


def _up(pt, a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(_dev(pt))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the steps against the twins
# ---------------------------------------------------------------------------------------------------------------------------
def _device_select(pt, acc, recv, n, params, active=None, pad=64):
    """PTSelectReceivers into arrays `pad` entries longer than the list, filled with sentinels -> (indices, receivers, stopped)"""
    import torch
    lib = plugin.load_library()
    count = len(acc) if active is None else len(active)
    d_acc, d_recv = _up(pt, acc), _up(pt, recv)
    d_act = None if active is None else _up(pt, np.asarray(active, np.uint32))
    out_a = torch.full((count + pad,), SENTINEL_U - (1 << 32), dtype=torch.int32, device=_dev(pt))
    out_r = torch.full((count + pad, 8), SENTINEL_F, dtype=torch.float32, device=_dev(pt))
    torch.cuda.synchronize(_dev(pt))
    survivors, stopped = C.c_uint64(), (C.c_uint64 * 3)()
    a = plugin.adaptive_gather_params(params)
    plugin.check(lib.PTSelectReceivers(pt.ctx, C.byref(a), n, None if d_act is None else d_act.data_ptr(), count, d_acc.data_ptr(), d_recv.data_ptr(), len(acc),
                                       out_a.data_ptr(), out_r.data_ptr(), C.byref(survivors), stopped))
    s = survivors.value
    got_a, got_r = out_a.cpu().numpy().view(np.uint32), out_r.cpu().numpy()
    assert (got_a[s:] == SENTINEL_U).all() and (got_r[s:] == SENTINEL_F).all(), "something past the survivor count was written"
    return got_a[:s], got_r[:s], np.array(list(stopped), np.uint64)


@pytest.mark.parametrize("count", cases.SIZES + [262144])
def test_select_equals_twin(box, count):
    """262,144 and 262,145 entries are 1,024 and 1,025 blocks: the last list of which each of the scan's 1,024 threads owns one
    block count, and the first of which it owns two (csrc/pt_compact.h)"""
    pt, _ = box
    for pattern in cases.PATTERNS:
        acc, recv, keep = cases.generated_list(count, pattern, seed=count)
        want = plugin.select_receivers(acc, recv, cases.N, PARAMS)
        assert len(want[0]) == keep.sum()
        got = _device_select(pt, acc, recv, cases.N, PARAMS)                      # the NULL "every entry" list
        assert (got[0] == want[0]).all() and (got[2] == want[2]).all(), (count, pattern, got[2], want[2])
        _same(got[1], want[1], (count, pattern))


@pytest.mark.parametrize("count", [257, 1000, 262144, 262145])
def test_select_through_a_list_equals_twin(box, count):
    pt, _ = box
    acc, recv, keep = cases.generated_list(count, "random30", seed=count + 1)
    active = np.nonzero(np.random.RandomState(count).uniform(size=count) < 0.33)[0].astype(np.uint32)
    for lst in (active, active[::-1].copy()):
        want = plugin.select_receivers(acc, recv, cases.N, PARAMS, active=lst)
        got = _device_select(pt, acc, recv, cases.N, PARAMS, active=lst)
        assert 0 < len(want[0]) < len(lst) and (got[0] == want[0]).all() and (got[2] == want[2]).all()
        _same(got[1], want[1], count)
    # an index the arrays do not hold is left out and counted nowhere (the twin refuses it)
    lst = np.concatenate([active[:100], np.array([count, 0xFFFFFFFF], np.uint32), active[100:]])
    want = plugin.select_receivers(acc, recv, cases.N, PARAMS, active=active)
    got = _device_select(pt, acc, recv, cases.N, PARAMS, active=lst)
    assert (got[0] == want[0]).all() and (got[2] == want[2]).all()


def test_select_special_entries_equal_twin(box):
    pt, _ = box
    acc, want_reason, _ = cases.special_entries()
    recv = cases.receivers(len(acc))
    want = plugin.select_receivers(acc, recv, cases.N, PARAMS)
    got = _device_select(pt, acc, recv, cases.N, PARAMS)
    assert (got[0] == want[0]).all() and (got[0] == np.nonzero(want_reason == ref.ACTIVE)[0]).all() and (got[2] == want[2]).all()
    _same(got[1], want[1], "special entries")
    acc, n, threshold, floor, reasons = cases.bound_entries()
    kw = dict(threshold=threshold, min_samples=2, add_samples=2, max_samples=8, dark_floor=floor)
    got = _device_select(pt, acc, cases.receivers(2), n, kw)
    assert list(got[0]) == [1] and list(got[2]) == [1, 0, 0], "v exactly at the bound stops: the comparison is >"
    acc, recv, keep = cases.generated_list(300, "alternating", seed=3, n=24)
    for max_samples, kept, by_max in ((32, 150, 0), (31, 0, 150)):
        got = _device_select(pt, acc, recv, 24, dict(PARAMS, max_samples=max_samples))
        assert len(got[0]) == kept and list(got[2]) == [150, by_max, 0], max_samples


@pytest.mark.parametrize("count", [1, 257, 1000, 262144, 262145])
def test_fold_and_equalise_equal_twins(box, count):
    import torch
    pt, _ = box
    lib = plugin.load_library()
    dev = _dev(pt)
    pad = 64
    first, second = cases.fresh_rows(count, seed=count, m=cases.N), cases.fresh_rows(count, seed=count + 1)
    if count > 1:
        second[count // 2, 1] = np.nan
    active = np.nonzero(cases.pattern_mask(count, "random30", seed=count) | (np.arange(count) == 0))[0].astype(np.uint32)
    third = cases.fresh_rows(len(active), seed=count + 2)
    acc = torch.full((count + pad, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    counts = torch.full((count + pad,), SENTINEL_U - (1 << 32), dtype=torch.int32, device=dev)
    d1, d2, d3, d_act = _up(pt, first), _up(pt, second), _up(pt, third), _up(pt, active)
    torch.cuda.synchronize(dev)
    # round 0 writes, a fold of every entry (NULL list), a fold through a list
    plugin.check(lib.PTFoldIrradiance(pt.ctx, None, count, d1.data_ptr(), cases.N, 0, count, acc.data_ptr(), counts.data_ptr()))
    plugin.check(lib.PTFoldIrradiance(pt.ctx, None, count, d2.data_ptr(), cases.ADD, cases.N, count, acc.data_ptr(), counts.data_ptr()))
    plugin.check(lib.PTFoldIrradiance(pt.ctx, d_act.data_ptr(), len(active), d3.data_ptr(), cases.ADD, cases.N + cases.ADD, count, acc.data_ptr(), counts.data_ptr()))
    pt.synchronize()
    want, want_counts = plugin.fold_irradiance(np.zeros((count, 4), F), 0, first, cases.N, counts=np.zeros(count, np.uint32))
    want, want_counts = plugin.fold_irradiance(want, cases.N, second, cases.ADD, counts=want_counts)
    want, want_counts = plugin.fold_irradiance(want, cases.N + cases.ADD, third, cases.ADD, active=active, counts=want_counts)
    got, got_counts = acc.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
    _same(got[:count], want, ("fold", count))
    assert (got_counts[:count] == want_counts).all() and (got[count:] == SENTINEL_F).all() and (got_counts[count:] == SENTINEL_U).all()
    # equalise out of place, then in place
    out = torch.full((count + pad, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    plugin.check(lib.PTEqualiseIrradiance(pt.ctx, acc.data_ptr(), counts.data_ptr(), count, cases.MAX, out.data_ptr()))
    plugin.check(lib.PTEqualiseIrradiance(pt.ctx, acc.data_ptr(), counts.data_ptr(), count, cases.MAX, acc.data_ptr()))
    pt.synchronize()
    want_eq = plugin.equalise_irradiance(want, want_counts, cases.MAX)
    for name, t in (("out of place", out), ("in place", acc)):
        g = t.cpu().numpy()
        _same(g[:count], want_eq, ("equalise", name, count))
        assert (g[count:] == SENTINEL_F).all(), name + ": something past count was written"
    if count > 1:
        assert (_bits(want_eq[count // 2]) == _bits(want[count // 2])).all(), "the NaN entry passes through"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the contract
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floor(box):
    """the box's floor at 48 x 48: its receivers, and irradiance() of ALL of them over each of the five ranges of 8 / 8 / 40, from
    sample 0 and from sample 2^20"""
    pt, uvs = box
    p = pt.params(seed=0)
    texels, recv = pt.chart_receivers(W, H, uvs=uvs, seed=77)
    assert texels.shape[0] == W * H
    rounds = {first: [pt.irradiance(receivers=recv, spp=MIN if r == 0 else ADD, first_sample=first + (0 if r == 0 else MIN + (r - 1) * ADD), params=p).cpu().numpy()
                      for r in range(1 + (MAX - MIN) // ADD)] for first in (0, 1 << 20)}
    # the threshold from the data: the square root of the median of v / d^2 of the 8-sample gather, so about half the entries stop there
    r0 = rounds[0][0]
    l = ref.luminance(r0[:, :3])
    floor_l = 0.01 * float(l.astype(np.float64).mean())
    v = ref.variance_of_mean(l, r0[:, 3], MIN).astype(np.float64)
    threshold = float(np.sqrt(np.median(v / np.maximum(l, F(floor_l)).astype(np.float64) ** 2)))
    return p, texels, recv, rounds, threshold, floor_l


def _expected(rounds, first, threshold, dark_floor, recv):
    sizes = [MIN] + [ADD] * (len(rounds[first]) - 1)
    starts = {(first + sum(sizes[:r])) & 0xFFFFFFFF: r for r in range(len(sizes))}
    return ref.adaptive(lambda a, m: rounds[first][starts[a]], len(recv), first, MIN, ADD, MAX, threshold, dark_floor, recv)


def _check_stats(stats, counts, count):
    counts = np.asarray(counts).astype(np.int64)
    assert stats["samples"] == counts.sum() and stats["maxCount"] == counts.max(), stats
    assert stats["rounds"] == 1 + (counts.max() - MIN) // ADD, stats
    assert stats["stoppedThreshold"] + stats["stoppedMaxSamples"] + stats["stoppedNonFinite"] == count, stats


def test_the_contract(box, floor):
    pt, _ = box
    p, _, recv, rounds, threshold, dark = floor
    want, want_counts, want_stats = _expected(rounds, 0, threshold, dark, recv.cpu().numpy())
    # not vacuous: about half stop after round 0, some go all the way, and there is something in between
    share = (want_counts == MIN).mean()
    print(f"[adaptive gather] box floor {W} x {H}, {MIN} / {ADD} / {MAX}, threshold {threshold:.4f}: {share * 100:.1f} % stop after round 0, "
          f"counts {dict(zip(*np.unique(want_counts, return_counts=True)))}")
    assert 0.25 <= share <= 0.75 and (want_counts == MAX).any() and len(np.unique(want_counts)) >= 3
    got, counts, stats = pt.irradiance_adaptive(receivers=recv, threshold=threshold, min_samples=MIN, add_samples=ADD, max_samples=MAX, dark_floor=dark, params=p)
    _same(got.cpu().numpy(), want, "the adaptive gather against the fold of plain gathers")
    assert (counts.cpu().numpy() == want_counts).all()
    _check_stats(stats, want_counts, len(want))
    assert {k: stats[k] for k in want_stats} == want_stats, (stats, want_stats)
    # PTStats counts the paths the rounds traced
    pt.synchronize()
    pt.reset_stats()
    pt.irradiance_adaptive(receivers=recv, threshold=threshold, min_samples=MIN, add_samples=ADD, max_samples=MAX, dark_floor=dark, params=p)
    assert pt.stats().as_dict()["paths"] == stats["samples"]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. invariants
# ---------------------------------------------------------------------------------------------------------------------------
def test_host_variant_permutation_and_offset(box, floor):
    import torch
    pt, _ = box
    p, _, recv, rounds, threshold, dark = floor
    kw = dict(threshold=threshold, min_samples=MIN, add_samples=ADD, max_samples=MAX, dark_floor=dark, params=p)
    want, want_counts, _ = _expected(rounds, 0, threshold, dark, recv.cpu().numpy())
    # numpy in: the Host variant
    got, counts, stats = pt.irradiance_adaptive(receivers=recv.cpu().numpy(), **kw)
    assert isinstance(got, np.ndarray) and counts.dtype == np.uint32
    _same(got, want, "the Host variant")
    assert (counts == want_counts).all()
    _check_stats(stats, counts, len(want))
    # a permuted list gives the permuted result
    perm = np.random.RandomState(5).permutation(len(want))
    got, counts, _ = pt.irradiance_adaptive(receivers=recv[torch.from_numpy(perm).to(recv.device)].contiguous(), **kw)
    _same(got.cpu().numpy(), want[perm], "a permuted list")
    assert (counts.cpu().numpy() == want_counts[perm]).all()
    # firstSample offset by 2^20: the expectation built from the offset ranges
    want_o, want_counts_o, _ = _expected(rounds, 1 << 20, threshold, dark, recv.cpu().numpy())
    got, counts, _ = pt.irradiance_adaptive(receivers=recv, first_sample=1 << 20, **kw)
    _same(got.cpu().numpy(), want_o, "firstSample = 2^20")
    assert (counts.cpu().numpy() == want_counts_o).all() and (want_counts_o != want_counts).any()


def test_schedules_agree(box, floor):
    pt, _ = box
    p, _, recv, rounds, threshold, dark = floor
    want, want_counts, _ = _expected(rounds, 0, threshold, dark, recv.cpu().numpy())
    try:
        for schedule in (2, 3, 1):
            pt.set_schedule(schedule)
            got, counts, _ = pt.irradiance_adaptive(receivers=recv, threshold=threshold, min_samples=MIN, add_samples=ADD, max_samples=MAX, dark_floor=dark, params=p)
            _same(got.cpu().numpy(), want, schedule)
            assert (counts.cpu().numpy() == want_counts).all(), schedule
    finally:
        pt.set_schedule(1)


def test_the_ends_of_the_threshold(box, floor):
    pt, _ = box
    p, _, recv, rounds, _, dark = floor
    n = len(rounds[0][0])
    # so large that everything stops after round 0: PTGatherIrradiance(minSamples), bit for bit
    got, counts, stats = pt.irradiance_adaptive(receivers=recv, threshold=1e30, min_samples=MIN, add_samples=ADD, max_samples=MAX, dark_floor=dark, params=p)
    _same(got.cpu().numpy(), rounds[0][0], "everything stops after round 0")
    assert (counts.cpu().numpy() == MIN).all() and stats["rounds"] == 1 and stats["stoppedThreshold"] == n and stats["samples"] == n * MIN
    # so small that nothing stops early (threshold^2 underflows to 0: only an entry whose samples so far are all equal -- v == 0 --
    # stops): the fold of all rounds; with maxSamples = 39 the largest count reachable is 32
    for max_samples, last in ((MAX, MAX), (MAX - 1, MAX - ADD)):
        full, k = rounds[0][0], MIN
        for r in rounds[0][1:1 + (last - MIN) // ADD]:
            full, k = ref.fold(full, k, r, ADD), k + ADD
        assert k == last
        sizes = {MIN * (r > 0) + ADD * max(r - 1, 0): r for r in range(len(rounds[0]))}
        want, want_counts, _ = ref.adaptive(lambda a, m: rounds[0][sizes[a]], n, 0, MIN, ADD, max_samples, 1e-30, dark, recv.cpu().numpy())
        whole = want_counts == last
        print(f"[adaptive gather] threshold 1e-30, maxSamples {max_samples}: {whole.mean() * 100:.1f} % of the entries reach {last}")
        assert whole.mean() > 0.5 and want_counts.max() == last
        _same(want[whole], full[whole], "the restatement: an entry that never stops is the fold of all rounds")
        got, counts, stats = pt.irradiance_adaptive(receivers=recv, threshold=1e-30, min_samples=MIN, add_samples=ADD, max_samples=max_samples, dark_floor=dark,
                                                    params=p)
        _same(got.cpu().numpy(), want, ("nothing stops early", max_samples))
        assert (counts.cpu().numpy() == want_counts).all() and stats["maxCount"] == last and stats["stoppedMaxSamples"] == whole.sum()


def test_two_chunks_in_round_zero(box):
    """minSamples = 1,024: a launch sequence holds floor(2^21 / 1024) = 2,048 entries, the list has 2,304, so round 0 takes two chunks;
    the threshold keeps a few hundred entries, so round 1's compacted list fits one"""
    pt, uvs = box
    p = pt.params(seed=0)
    _, recv = pt.chart_receivers(W, H, uvs=uvs, seed=78)
    n = recv.shape[0]
    assert (1 << 21) // 1024 < n
    r0 = pt.irradiance(receivers=recv, spp=1024, params=p).cpu().numpy()
    r1 = pt.irradiance(receivers=recv, spp=64, first_sample=1024, params=p).cpu().numpy()
    l = ref.luminance(r0[:, :3])
    dark = 0.01 * float(l.astype(np.float64).mean())
    v = ref.variance_of_mean(l, r0[:, 3], 1024).astype(np.float64)
    threshold = float(np.sqrt(np.quantile(v / np.maximum(l, F(dark)).astype(np.float64) ** 2, 0.9)))
    want, want_counts, _ = ref.adaptive(lambda a, m: r0 if a == 0 else r1, n, 0, 1024, 64, 1088, threshold, dark, recv.cpu().numpy())
    kept = (want_counts == 1088).sum()
    assert 0 < kept < 2048 and set(want_counts) == {1024, 1088}
    got, counts, stats = pt.irradiance_adaptive(receivers=recv, threshold=threshold, min_samples=1024, add_samples=64, max_samples=1088, dark_floor=dark, params=p)
    _same(got.cpu().numpy(), want, "two chunks, then one")
    assert (counts.cpu().numpy() == want_counts).all() and stats["rounds"] == 2 and stats["samples"] == n * 1024 + kept * 64


# ---------------------------------------------------------------------------------------------------------------------------
# 4. bake_lightmap
# ---------------------------------------------------------------------------------------------------------------------------
def test_bake_lightmap_adaptive(box, floor):
    pt, uvs = box
    p, texels, recv, rounds, threshold, dark = floor
    kw = dict(uvs=uvs, seed=77, params=p)
    t = texels.cpu().numpy()
    # None: today's bytes -- the resolve of the plain gather
    irr8 = pt.irradiance(receivers=recv, spp=MIN, params=p)
    plain = pt.bake_lightmap(W, H, spp=MIN, **kw)
    assert (_bits(plain) == _bits(pt.resolve_lightmap(texels, irr8, W, H).cpu().numpy())).all()
    assert (_bits(pt.bake_lightmap(W, H, spp=MIN, adaptive=None, **kw)) == _bits(plain)).all()
    image, count_image = pt.bake_lightmap(W, H, spp=MIN, return_counts=True, **kw)
    assert (_bits(image) == _bits(plain)).all() and count_image.dtype == np.int32 and (count_image == MIN).all()
    # a dict: the resolve of irradiance_adaptive's list, and the scatter of its counts
    ad = dict(threshold=threshold, min_samples=MIN, add_samples=ADD, max_samples=MAX, dark_floor=dark)
    irr, counts, _ = pt.irradiance_adaptive(receivers=recv, params=p, **ad)
    image, count_image = pt.bake_lightmap(W, H, adaptive=ad, return_counts=True, **kw)
    assert (_bits(image) == _bits(pt.resolve_lightmap(texels, irr, W, H).cpu().numpy())).all() and (_bits(image) != _bits(plain)).any()
    scatter = np.zeros(W * H, np.int32)
    scatter[t] = counts.cpu().numpy()
    assert (count_image == scatter.reshape(H, W)).all() and len(np.unique(count_image)) >= 3
    # spp is max_samples unless the dict says otherwise; a number is the threshold
    ad2 = {k: v for k, v in ad.items() if k != "max_samples"}
    assert (_bits(pt.bake_lightmap(W, H, spp=MAX, adaptive=ad2, **kw)) == _bits(image)).all()
    irr_n, _, _ = pt.irradiance_adaptive(receivers=recv, params=p, threshold=threshold, max_samples=48, dark_floor=dark)
    assert (_bits(pt.bake_lightmap(W, H, spp=48, adaptive=dict(threshold=threshold, dark_floor=dark), **kw)) ==
            _bits(pt.resolve_lightmap(texels, irr_n, W, H).cpu().numpy())).all()
    # with denoise: equalised to max_samples, the denoiser runs with samples = max_samples
    eq = pt.equalise_irradiance(irr, counts, MAX)
    _same(eq.cpu().numpy(), plugin.equalise_irradiance(irr.cpu().numpy(), counts.cpu().numpy(), MAX), "equalise on the device")
    want = pt.resolve_lightmap(texels, pt.denoise_lightmap(texels, recv, eq, W, H, MAX, iterations=5), W, H).cpu().numpy()
    got = pt.bake_lightmap(W, H, adaptive=ad, denoise=5, **kw)
    assert (_bits(got) == _bits(want)).all() and (_bits(got) != _bits(image)).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. it does what it is for
# ---------------------------------------------------------------------------------------------------------------------------
def test_adaptive_beats_uniform_at_equal_paths():
    """A floor half in plain view of a point light, half in the shadow of an occluder: the 95th percentile of the relative luminance
    error against a 4,096-sample gather over a disjoint range must be lower for the adaptive gather than for the uniform gather with
    at least as many paths.  Both figures and their ratio are printed (DESIGN.md 5.24 has the ones measured on the card)."""
    scene = cases.shadowed_box()
    pt = PathTracer(scene, width=32, height=32, samplesPerPass=1, maxRayBounces=3, schedule=1)
    try:
        p = pt.params(seed=0)
        _, recv = pt.chart_receivers(W, H, uvs=chart_cases.floor_only_uvs(len(scene.tri_attrs)), seed=77)
        n = recv.shape[0]
        assert n == W * H
        ref_irr = pt.irradiance(receivers=recv, spp=4096, first_sample=1 << 20, params=p).cpu().numpy()
        lum_ref = ref.luminance(ref_irr[:, :3]).astype(np.float64)
        r0 = pt.irradiance(receivers=recv, spp=16, params=p).cpu().numpy()
        l0 = ref.luminance(r0[:, :3])
        dark = 0.01 * float(l0.astype(np.float64).mean())
        v0 = ref.variance_of_mean(l0, r0[:, 3], 16).astype(np.float64)
        threshold = float(np.sqrt(np.median(v0 / np.maximum(l0, F(dark)).astype(np.float64) ** 2)))
        irr, counts, stats = pt.irradiance_adaptive(receivers=recv, threshold=threshold, min_samples=16, add_samples=16, max_samples=256, dark_floor=dark, params=p)
        counts = counts.cpu().numpy().astype(np.int64)
        x = recv.cpu().numpy()[:, 0]
        shadowed, lit = x < cases.SHADOW_X, x > -cases.SHADOW_X
        # the scene is heterogeneous: the shadowed half is darker and asks for more samples
        assert shadowed.sum() > n // 3 and lit.sum() > n // 3 and lum_ref[shadowed].mean() < 0.5 * lum_ref[lit].mean()
        print(f"[adaptive gather] shadowed box: mean count {counts[shadowed].mean():.1f} in the shadow, {counts[lit].mean():.1f} in the light; "
              f"{stats['rounds']} rounds, {stats['samples']} paths")
        assert counts[shadowed].mean() > counts[lit].mean()
        spp = -(-stats["samples"] // n)                             # rounded up: the uniform gather never gets fewer paths
        uni = pt.irradiance(receivers=recv, spp=spp, params=p).cpu().numpy()

        def p95(e):
            return float(np.percentile(np.abs(ref.luminance(e[:, :3]).astype(np.float64) - lum_ref) / np.maximum(lum_ref, dark), 95))
        e_ad, e_un = p95(irr.cpu().numpy()), p95(uni)
        print(f"[adaptive gather] shadowed box {W} x {H}, threshold {threshold:.4f}: p95 relative luminance error {e_ad:.4e} adaptive ({stats['samples']} paths), "
              f"{e_un:.4e} uniform at {spp} spp ({n * spp} paths), ratio {e_un / e_ad:.2f}")
        assert e_ad < e_un
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. errors that need a context
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors(box, floor):
    import torch
    pt, _ = box
    lib = plugin.load_library()
    p, _, recv, rounds, threshold, dark = floor
    n = 100
    d_recv = recv[:n].contiguous()
    out = torch.full((n, 4), SENTINEL_F, dtype=torch.float32, device=recv.device)
    counts = torch.full((n,), 7, dtype=torch.int32, device=recv.device)
    torch.cuda.synchronize(recv.device)
    good = abi.adaptive_gather(threshold, MIN, ADD, MAX, dark)

    def call(a=good, params=p, r=d_recv.data_ptr(), count=n, o=out.data_ptr(), c=counts.data_ptr()):
        return lib.PTGatherIrradianceAdaptive(pt.ctx, None if params is None else C.byref(params), None if a is None else C.byref(a), r, count, o, c, None)

    assert call(a=None) == abi.PT_ERR_INVALID_ARG and b"adaptive == NULL" in lib.PTGetLastError()
    assert call(params=None) == abi.PT_ERR_INVALID_ARG and b"params == NULL" in lib.PTGetLastError()
    for kw, word in ((dict(min_samples=1), b"minSamples = 1"), (dict(min_samples=65537, max_samples=70000), b"minSamples = 65537"),
                     (dict(add_samples=0), b"addSamples = 0"), (dict(add_samples=65537), b"addSamples = 65537"), (dict(max_samples=MIN - 1), b"maxSamples = 7"),
                     (dict(max_samples=(1 << 24) + 1), b"maxSamples = 16777217"), (dict(threshold=0.0), b"threshold"), (dict(threshold=float("nan")), b"threshold"),
                     (dict(dark_floor=-1.0), b"darkFloor"), (dict(dark_floor=float("inf")), b"darkFloor")):
        a = abi.adaptive_gather(**dict(dict(threshold=threshold, min_samples=MIN, add_samples=ADD, max_samples=MAX, dark_floor=dark), **kw))
        assert call(a=a) == abi.PT_ERR_INVALID_ARG and word in lib.PTGetLastError(), (kw, lib.PTGetLastError())
    a = abi.adaptive_gather(threshold, MIN, ADD, MAX, dark)
    a.reserved[0] = 1
    assert call(a=a) == abi.PT_ERR_INVALID_ARG and b"reserved" in lib.PTGetLastError()
    a = abi.adaptive_gather(threshold, MIN, ADD, MAX, dark)
    a.structSize = 40
    assert call(a=a) == abi.PT_ERR_INVALID_ARG and b"structSize" in lib.PTGetLastError()
    for name in ("r", "o"):
        assert call(**{name: None}) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError(), name
    for name, ptr in (("r", d_recv.data_ptr() + 4), ("o", out.data_ptr() + 4), ("c", counts.data_ptr() + 2)):
        assert call(**{name: ptr}) == abi.PT_ERR_INVALID_ARG and b"misaligned" in lib.PTGetLastError(), name
    assert call(count=(1 << 31) + 1) == abi.PT_ERR_INVALID_ARG and b"2^31" in lib.PTGetLastError()
    deep = pt.params(seed=0)
    deep.MaxRayBounces = 8192
    assert call(params=deep) == abi.PT_ERR_UNSUPPORTED and b"8191" in lib.PTGetLastError()
    try:
        for schedule in (0, 4):
            pt.set_schedule(schedule)
            assert call() == abi.PT_ERR_UNSUPPORTED and b"schedule" in lib.PTGetLastError(), schedule
    finally:
        pt.set_schedule(1)
    # the Host variant checks the receivers' reserved words
    host = recv[:n].cpu().numpy().copy()
    host.view(np.uint32)[3, 7] = 1
    h_out = np.full((n, 4), SENTINEL_F, F)
    assert lib.PTGatherIrradianceAdaptiveHost(pt.ctx, C.byref(p), C.byref(good), host.ctypes.data, n, h_out.ctypes.data, None, None) == abi.PT_ERR_INVALID_ARG
    assert b"receivers[3].reserved" in lib.PTGetLastError() and (h_out == SENTINEL_F).all()
    # the steps
    n64 = C.c_uint64(5)
    assert lib.PTSelectReceivers(pt.ctx, C.byref(good), 1, None, n, out.data_ptr(), d_recv.data_ptr(), n, counts.data_ptr(), out.data_ptr(), C.byref(n64),
                                 None) == abi.PT_ERR_INVALID_ARG and b"n = 1" in lib.PTGetLastError()
    assert lib.PTSelectReceivers(pt.ctx, C.byref(good), 8, None, n + 1, out.data_ptr(), d_recv.data_ptr(), n, counts.data_ptr(), out.data_ptr(), C.byref(n64),
                                 None) == abi.PT_ERR_INVALID_ARG and b"activeCount" in lib.PTGetLastError()
    assert lib.PTFoldIrradiance(pt.ctx, None, n, d_recv.data_ptr(), 0, 8, n, out.data_ptr(), None) == abi.PT_ERR_INVALID_ARG and b"m = 0" in lib.PTGetLastError()
    assert lib.PTFoldIrradiance(pt.ctx, None, n, None, 8, 8, n, out.data_ptr(), None) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    assert lib.PTEqualiseIrradiance(pt.ctx, out.data_ptr(), counts.data_ptr(), n, 1, out.data_ptr()) == abi.PT_ERR_INVALID_ARG and b"samplesEq = 1" in lib.PTGetLastError()
    assert lib.PTEqualiseIrradiance(pt.ctx, out.data_ptr(), counts.data_ptr() + 2, n, 16, out.data_ptr()) == abi.PT_ERR_INVALID_ARG
    # before a scene
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(pt.device, C.byref(ctx)))
    try:
        assert lib.PTGatherIrradianceAdaptive(ctx, C.byref(p), C.byref(good), d_recv.data_ptr(), n, out.data_ptr(), counts.data_ptr(), None) == abi.PT_ERR_NO_SCENE
    finally:
        lib.PTDestroy(ctx)
    # an empty list is fine and launches nothing; so far nothing was written
    st = abi.PTAdaptiveGatherStats()
    st.rounds = 9
    assert lib.PTGatherIrradianceAdaptive(pt.ctx, C.byref(p), C.byref(good), d_recv.data_ptr(), 0, out.data_ptr(), None, C.byref(st)) == abi.PT_OK and st.rounds == 0
    pt.synchronize()
    assert (out == SENTINEL_F).all().item() and (counts == 7).all().item(), "a refused call wrote something"
    # and the context still works
    assert call() == abi.PT_OK
    want, want_counts, _ = _expected(rounds, 0, threshold, dark, recv.cpu().numpy())
    _same(out.cpu().numpy(), want[:n], "after the refusals")
    assert (counts.cpu().numpy() == want_counts[:n]).all()
