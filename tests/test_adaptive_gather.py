"""Adaptive gathers without a GPU (include/ptmi_plugin.h Part 19): the ABI, the host twins of select, fold and equalise against the
numpy restatement of the rule bit for bit -- on lists of every size at which the compaction changes its path and in every survivor
pattern --, the special entries the rule has a sentence for, what equalising does to the denoiser's variance, the refusals, the
sanitizer program and the compile-time resources of the kernels.  tests/test_gpu_adaptive_gather.py holds the
kernels to the twins and the loop to its contract.

Every statement about a case's content is asserted on the case itself before anything is compared."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from kernel_resources import resources
import adaptive_gather_cases as cases
import adaptive_gather_ref as ref
import lmfilter_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SYMBOLS = ["PTGatherIrradianceAdaptive", "PTGatherIrradianceAdaptiveHost", "PTSelectReceivers", "PTFoldIrradiance", "PTEqualiseIrradiance",
           "PTSelectReceiversHost", "PTFoldIrradianceHost", "PTEqualiseIrradianceHost"]
PARAMS = dict(threshold=cases.THRESHOLD, min_samples=cases.N, add_samples=cases.ADD, max_samples=cases.MAX, dark_floor=cases.DARK_FLOOR)
RULE = (cases.ADD, cases.MAX, cases.THRESHOLD, cases.DARK_FLOOR)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape and (_bits(got) == _bits(want)).all(), what


# ---------------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in SYMBOLS:
        assert name in exported and name in plugin.EXPORTED_SYMBOLS and f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 19: adaptive gathers" in header


def test_structs_match_c_header():
    fields = {"PTAdaptiveGather": ["structSize", "firstSample", "minSamples", "addSamples", "maxSamples", "threshold", "darkFloor", "reserved"],
              "PTAdaptiveGatherStats": ["rounds", "maxCount", "samples", "stoppedThreshold", "stoppedMaxSamples", "stoppedNonFinite"]}
    lines = []
    for s, fs in fields.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ptmi_plugin.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = dict(l.split() for l in subprocess.check_output([os.path.join(d, "p")]).decode().splitlines())
    for s, fs in fields.items():
        cls = getattr(abi, s)
        assert int(got[s]) == C.sizeof(cls), s
        assert [f for f, _ in cls._fields_] == fs, s
        for f in fs:
            assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, (s, f)
    a = abi.adaptive_gather(0.1)
    assert a.structSize == 48 and (a.minSamples, a.addSamples, a.maxSamples) == (16, 16, 1024) and a.darkFloor == 0.0


def test_null_context_is_named():
    lib = plugin.load_library()
    a, p = abi.adaptive_gather(0.1), abi.PTFrameParams()
    buf = (C.c_float * 64)()
    n64 = C.c_uint64()
    assert lib.PTGatherIrradianceAdaptive(None, C.byref(p), C.byref(a), buf, 1, buf, None, None) == abi.PT_ERR_INVALID_ARG
    assert b"PTGatherIrradianceAdaptive: ctx == NULL" in lib.PTGetLastError()
    assert lib.PTGatherIrradianceAdaptiveHost(None, C.byref(p), C.byref(a), buf, 1, buf, None, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTSelectReceivers(None, C.byref(a), 16, None, 1, buf, buf, 1, buf, buf, C.byref(n64), None) == abi.PT_ERR_INVALID_ARG
    assert b"PTSelectReceivers: ctx == NULL" in lib.PTGetLastError()
    assert lib.PTFoldIrradiance(None, None, 1, buf, 8, 8, 1, buf, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTEqualiseIrradiance(None, buf, buf, 1, 16, buf) == abi.PT_ERR_INVALID_ARG and b"PTEqualiseIrradiance: ctx == NULL" in lib.PTGetLastError()


# ---------------------------------------------------------------------------------------------------------------------------
# select: the twin against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", cases.SIZES)
def test_select_twin_equals_numpy(count):
    for pattern in cases.PATTERNS:
        acc, recv, keep = cases.generated_list(count, pattern, seed=count)
        # the case is what it says: the restatement keeps exactly the entries made to go on
        assert (ref.reasons(acc, cases.N, *RULE) == np.where(keep, ref.ACTIVE, ref.BY_THRESHOLD)).all(), pattern
        want = ref.select(acc, recv, cases.N, *RULE)
        assert (want[0] == np.nonzero(keep)[0]).all()
        got = plugin.select_receivers(acc, recv, cases.N, PARAMS)
        assert (got[0] == want[0]).all() and got[0].dtype == np.uint32, (count, pattern)
        _same(got[1], want[1], (count, pattern, "receivers"))
        assert (got[2] == want[2]).all() and int(got[2].sum()) + len(got[0]) == count, (count, pattern, got[2], want[2])


@pytest.mark.parametrize("count", [257, 1000, 262145])
def test_select_through_a_list(count):
    """a round >= 1: the list names a third of the entries, in ascending order; the survivors keep the list's order"""
    acc, recv, keep = cases.generated_list(count, "random30", seed=count + 1)
    active = np.nonzero(np.random.RandomState(count).uniform(size=count) < 0.33)[0].astype(np.uint32)
    want = ref.select(acc, recv, cases.N, *RULE, active=active)
    assert 0 < len(want[0]) < len(active) and (want[0] == active[keep[active]]).all()
    got = plugin.select_receivers(acc, recv, cases.N, PARAMS, active=active)
    assert (got[0] == want[0]).all() and (got[2] == want[2]).all()
    _same(got[1], want[1], "receivers")
    # a list in another order: a stable compaction keeps it
    back = active[::-1].copy()
    got = plugin.select_receivers(acc, recv, cases.N, PARAMS, active=back)
    assert (got[0] == back[keep[back]]).all()
    _same(got[1], recv[got[0]], "receivers")


def test_special_entries():
    acc, want, words = cases.special_entries()
    recv = cases.receivers(len(acc))
    assert (ref.reasons(acc, cases.N, *RULE) == want).all(), [w for w, a, b in zip(words, ref.reasons(acc, cases.N, *RULE), want) if a != b]
    idx, rows, stopped = plugin.select_receivers(acc, recv, cases.N, PARAMS)
    assert (idx == np.nonzero(want == ref.ACTIVE)[0]).all(), idx
    assert list(stopped) == [(want == k).sum() for k in (ref.BY_THRESHOLD, ref.BY_MAX_SAMPLES, ref.NON_FINITE)]
    # the floor decided the last one: without a floor it goes on
    assert words[-1].startswith("l below darkFloor") and ref.reasons(acc[-1:], cases.N, cases.ADD, cases.MAX, cases.THRESHOLD, 0.0)[0] == ref.ACTIVE
    assert len(plugin.select_receivers(acc[-1:], recv[-1:], cases.N, dict(PARAMS, dark_floor=0.0))[0]) == 1


def test_v_exactly_at_the_bound_stops():
    acc, n, threshold, floor, want = cases.bound_entries()
    l = ref.luminance(acc[:, :3])
    v = ref.variance_of_mean(l, acc[:, 3], n)
    assert v[0] == F(threshold) * F(threshold) * (l[0] * l[0]) and v[1] > v[0], (v, l)
    kw = dict(threshold=threshold, min_samples=2, add_samples=2, max_samples=8, dark_floor=floor)
    assert list(ref.reasons(acc, n, 2, 8, threshold, floor)) == want
    idx, _, stopped = plugin.select_receivers(acc, cases.receivers(2), n, kw)
    assert list(idx) == [1] and list(stopped) == [1, 0, 0]


def test_max_samples_is_inclusive():
    """n + addSamples == maxSamples stays; one sample less room stops, and is counted as stopped by maxSamples"""
    acc, recv, keep = cases.generated_list(300, "alternating", seed=3, n=24)
    for max_samples, reason in ((32, ref.ACTIVE), (31, ref.BY_MAX_SAMPLES)):
        assert (ref.reasons(acc, 24, 8, max_samples, cases.THRESHOLD, cases.DARK_FLOOR) == np.where(keep, reason, ref.BY_THRESHOLD)).all()
        idx, _, stopped = plugin.select_receivers(acc, recv, 24, dict(PARAMS, max_samples=max_samples))
        assert len(idx) == (150 if reason == ref.ACTIVE else 0) and list(stopped) == [150, 0 if reason == ref.ACTIVE else 150, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# fold
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 257, 1000])
def test_fold_of_three_parts(count):
    parts = [cases.fresh_rows(count, seed=count + k, m=m) for k, m in enumerate((cases.N, cases.ADD, cases.ADD))]
    if count > 1:
        parts[1][count // 2, 1] = np.nan                            # a NaN folds like any number
    acc_t = plugin.fold_irradiance(np.full((count, 4), 9.0, F), 0, parts[0], cases.N)
    _same(acc_t, parts[0], "n == 0 writes")
    acc_r, n = ref.fold(np.zeros((count, 4), F), 0, parts[0], cases.N), cases.N
    for part in parts[1:]:
        acc_t, acc_r = plugin.fold_irradiance(acc_t, n, part, cases.ADD), ref.fold(acc_r, n, part, cases.ADD)
        n += cases.ADD
        _same(acc_t, acc_r, (count, n))
    # the mean of the parts, to rounding, and the sum of their m2
    mean = (parts[0][:, :3].astype(np.float64) * cases.N + (parts[1][:, :3].astype(np.float64) + parts[2][:, :3]) * cases.ADD) / n
    ok = np.isfinite(mean).all(axis=1)
    assert np.abs(acc_t[ok, :3] - mean[ok]).max() < 1e-6 * np.abs(mean[ok]).max()
    assert (acc_t[:, 3] == (parts[0][:, 3] + parts[1][:, 3]) + parts[2][:, 3]).all()


def test_fold_through_a_list_and_counts():
    count = 1000
    acc = cases.fresh_rows(count, seed=1, m=cases.N)
    active = np.nonzero(cases.pattern_mask(count, "random30", seed=9))[0].astype(np.uint32)
    fresh = cases.fresh_rows(len(active), seed=2)
    counts = np.full(count, cases.N, np.uint32)
    got, got_counts = plugin.fold_irradiance(acc, cases.N, fresh, cases.ADD, active=active, counts=counts)
    want, want_counts = ref.fold(acc, cases.N, fresh, cases.ADD, active=active, counts=counts)
    _same(got, want, "fold through a list")
    assert (got_counts == want_counts).all() and set(got_counts) == {cases.N, cases.N + cases.ADD}
    rest = np.setdiff1d(np.arange(count), active)
    _same(got[rest], acc[rest], "entries the list does not name")


# ---------------------------------------------------------------------------------------------------------------------------
# equalise
# ---------------------------------------------------------------------------------------------------------------------------
def _equalise_case(count, seed):
    acc, _, _ = cases.generated_list(count, "random30", seed=seed)
    counts = cases.counts_for(count, seed)
    # m2 as it would be after counts[i] samples with the list's relative spread
    acc[:, 3] = (acc[:, 3].astype(np.float64) * counts / cases.N).astype(F)
    acc[5 % count, 0] = np.nan
    acc[7 % count, 3] = np.inf
    counts[11 % count] = 1                                          # a count the rule has no variance for
    return acc, counts


@pytest.mark.parametrize("count", cases.SIZES)
def test_equalise_twin_equals_numpy(count):
    acc, counts = _equalise_case(count, seed=count)
    want = ref.equalise(acc, counts, cases.MAX)
    got = plugin.equalise_irradiance(acc, counts, cases.MAX)
    assert (_bits(got) == _bits(want)).all(), count
    assert (_bits(got[:, :3]) == _bits(acc[:, :3])).all(), "equalise moved an rgb"
    for i in {5 % count, 7 % count, 11 % count}:
        assert (_bits(got[i]) == _bits(acc[i])).all(), "a non-finite entry, or one without a variance, passes through byte for byte"


def test_equalise_hands_the_denoiser_the_entrys_own_variance():
    """Part 17's step 1 at samples = S_eq over the equalised list against the entry's own v.  No tolerance is fixed in advance: the
    largest relative difference is printed (DESIGN.md 5.24 records it).  Asserted: a positive v stays positive, and where
    n_i == S_eq the two agree exactly or as the restatement says."""
    count = 262145
    acc, counts = _equalise_case(count, seed=4)
    ok = np.isfinite(acc).all(axis=1) & (counts >= 2)
    own = ref.variance_of_mean(ref.luminance(acc[:, :3]), acc[:, 3], np.where(ok, counts, 2))
    eq = plugin.equalise_irradiance(acc, counts, cases.MAX)
    back = lmfilter_ref.entry_variance(eq[:, :3], eq[:, 3], cases.MAX)
    pos = ok & (own > 0)
    assert pos.sum() > count // 2
    rel = np.abs(back[pos].astype(np.float64) - own[pos]) / own[pos]
    same = ok & (counts == cases.MAX)
    exact = (_bits(back[same]) == _bits(own[same])).mean()
    print(f"[adaptive gather] equalise to {cases.MAX}: v recovered by the denoiser's step 1 against the entry's own, {pos.sum()} entries: "
          f"largest relative difference {rel.max():.3e}, median {np.median(rel):.3e}; bit-equal where n_i == S_eq: {exact * 100:.2f} % of {same.sum()}")
    assert (back[pos] > 0).all(), "a positive variance was lost"
    # where n_i == S_eq the algebra is the identity, but each of m2 -> v -> m2' -> v rounds: the restatement tells what comes back
    want = lmfilter_ref.entry_variance(acc[same, :3], ref.equalise(acc, counts, cases.MAX)[same, 3], cases.MAX)
    assert (_bits(back[same]) == _bits(want)).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the whole loop in numpy: the restatement is consistent with itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_loop_of_the_restatement_over_twin_steps():
    """The rounds of Part 19 driven from Python over the twins' steps equal ref.adaptive over the same fake gather."""
    count = 1000
    recv = cases.receivers(count)
    noise = np.random.RandomState(3).uniform(0.0, 0.6, count)

    def gather(first, samples):
        """`samples` deterministic pseudo-samples per entry from (entry, sample index): the same whatever the range is cut into"""
        j = (first + np.arange(samples))[None, :].astype(np.float64)
        e = 1.0 + noise[:, None] * np.sin(12.9898 * j + 78.233 * np.arange(count)[:, None])
        rows = np.zeros((count, 4), F)
        rows[:, 0] = rows[:, 1] = rows[:, 2] = e.mean(axis=1)
        rows[:, 3] = (e * e).sum(axis=1)
        return rows

    kw = dict(threshold=0.05, min_samples=8, add_samples=8, max_samples=40, dark_floor=0.01)
    want, want_counts, stats = ref.adaptive(gather, count, 100, 8, 8, 40, 0.05, 0.01, recv)
    assert len(set(want_counts)) >= 3 and want_counts.max() == 40 and 0.1 < (want_counts == 8).mean() < 0.9
    acc, counts = plugin.fold_irradiance(np.zeros((count, 4), F), 0, gather(100, 8), 8, counts=np.zeros(count, np.uint32))
    n, first, active = 8, 108, None
    while True:
        active, rows, _ = plugin.select_receivers(acc, recv, n, kw, active=active)
        if not len(active):
            break
        _same(rows, recv[active], "the receivers travel with the indices")
        acc, counts = plugin.fold_irradiance(acc, n, gather(first, 8)[active], 8, active=active, counts=counts)
        n, first = n + 8, first + 8
    _same(acc, want, "the loop")
    assert (counts == want_counts).all() and stats["maxCount"] == n
    assert stats["samples"] == int(want_counts.astype(np.int64).sum())
    assert stats["stoppedThreshold"] + stats["stoppedMaxSamples"] + stats["stoppedNonFinite"] == count


# ---------------------------------------------------------------------------------------------------------------------------
# refusals of the twins
# ---------------------------------------------------------------------------------------------------------------------------
REFUSED = [("minSamples", dict(min_samples=1)), ("minSamples", dict(min_samples=65537, max_samples=70000)), ("addSamples", dict(add_samples=0)),
           ("addSamples", dict(add_samples=65537)), ("maxSamples", dict(max_samples=cases.N - 1)), ("maxSamples", dict(max_samples=(1 << 24) + 1)),
           ("threshold", dict(threshold=0.0)), ("threshold", dict(threshold=float("nan"))), ("threshold", dict(threshold=float("inf"))),
           ("darkFloor", dict(dark_floor=-1.0)), ("darkFloor", dict(dark_floor=float("inf")))]


@pytest.mark.parametrize("word,kw", REFUSED)
def test_twin_refuses_parameters_out_of_range(word, kw):
    acc, recv, _ = cases.generated_list(10, "all")
    with pytest.raises(plugin.PluginError, match=word):
        plugin.select_receivers(acc, recv, cases.N, dict(PARAMS, **kw))


def test_twin_refusals_of_lists_and_structs():
    lib = plugin.load_library()
    acc, recv, _ = cases.generated_list(10, "all")
    for kw in (dict(min_samples=2), dict(min_samples=65536, max_samples=65536), dict(add_samples=65536), dict(max_samples=1 << 24), dict(dark_floor=0.0)):
        idx, _, stopped = plugin.select_receivers(acc, recv, cases.N, dict(PARAMS, **kw))                # the ends of the ranges
        assert len(idx) + int(stopped.sum()) == 10 and len(idx) == (0 if kw.get("add_samples") else 10), kw
    for n in (0, 1, (1 << 24) + 1):
        with pytest.raises(plugin.PluginError, match="n = "):
            plugin.select_receivers(acc, recv, n, PARAMS)
    with pytest.raises(plugin.PluginError, match=r"active\[1\] = 10"):
        plugin.select_receivers(acc, recv, cases.N, PARAMS, active=[0, 10])
    with pytest.raises(plugin.PluginError, match=r"active\[0\] = 12"):
        plugin.fold_irradiance(acc, 8, acc[:1], 8, active=[12])
    with pytest.raises(plugin.PluginError, match="activeCount"):
        plugin.select_receivers(acc, recv, cases.N, PARAMS, active=np.zeros(11, np.uint32))
    for m, n, word in ((0, 8, "m = 0"), (65537, 8, "m = 65537"), (8, (1 << 24) - 7, "n \\+ m")):
        with pytest.raises(plugin.PluginError, match=word):
            plugin.fold_irradiance(acc, n, acc, m)
    for s in (0, 1, (1 << 24) + 1):
        with pytest.raises(plugin.PluginError, match="samplesEq"):
            plugin.equalise_irradiance(acc, np.full(10, 16, np.uint32), s)
    a = abi.adaptive_gather(**PARAMS)
    out_a, out_r, n64 = np.zeros(10, np.uint32), np.zeros((10, 8), F), C.c_uint64(77)

    def call(a, acc_ptr=acc.ctypes.data, survivors=C.byref(n64)):
        return lib.PTSelectReceiversHost(None if a is None else C.byref(a), cases.N, None, 10, acc_ptr, recv.ctypes.data, 10, out_a.ctypes.data,
                                         out_r.ctypes.data, survivors, None)
    assert call(None) == 0 and b"adaptive == NULL" in lib.PTGetBVHBuildError()
    assert call(a, acc_ptr=None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert call(a, survivors=None) == 0 and b"survivors == NULL" in lib.PTGetBVHBuildError()
    a.reserved[2] = 1
    assert call(a) == 0 and b"reserved" in lib.PTGetBVHBuildError()
    a = abi.adaptive_gather(**PARAMS)
    a.structSize = 40
    assert call(a) == 0 and b"structSize" in lib.PTGetBVHBuildError()
    assert not out_a.any() and not out_r.any(), "a refused call wrote something"
    a = abi.adaptive_gather(**PARAMS)
    assert call(a) == 1 and n64.value == 10 and lib.PTGetBVHBuildError() == b""
    # empty lists are fine
    assert len(plugin.select_receivers(np.zeros((0, 4), F), np.zeros((0, 8), F), cases.N, PARAMS)[0]) == 0
    assert plugin.fold_irradiance(np.zeros((0, 4), F), 8, np.zeros((0, 4), F), 8).shape == (0, 4)
    assert plugin.equalise_irradiance(np.zeros((0, 4), F), np.zeros(0, np.uint32), 16).shape == (0, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# the sanitizers and the kernels' resources
# ---------------------------------------------------------------------------------------------------------------------------
def test_host_twins_under_sanitizers(tmp_path):
    """`make adaptive-gather-sanitize`: adaptive_gather_host.cpp and csrc/adaptive_gather_sanitize_main.cpp (its own main) with
    -fsanitize=address,undefined, built and run, nothing preloaded: it runs the whole loop over the twins in exactly sized arrays,
    equalises in place and out of place and makes the refusals, and must finish without a report."""
    csrc = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "adaptive-gather-sanitize", "ADAPTIVE_GATHER_SANITIZE_OUT=" + str(tmp_path / "adaptive_gather_sanitize")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "adaptive gather ok" in out.stdout, out.stdout + out.stderr


# VGPRs per kernel as DESIGN.md 5.24 lists them (hipcc's resource report); every kernel runs 8 waves per SIMD without scratch
KERNEL_VGPRS = {"pt_ag_count": 11, "pt_ag_scan": 20, "pt_ag_emit": 16, "pt_ag_fold": 25, "pt_ag_equalise": 14}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernel_resources():
    res = resources("pt_adaptive_gather.hip")
    assert len(res) == len(KERNEL_VGPRS) and all("pt_ag_" in k for k in res), sorted(res)
    for name, vgprs in KERNEL_VGPRS.items():
        found = [r for k, r in res.items() if f"{len(name)}{name}E" in k]
        assert len(found) == 1, (name, sorted(res))
        print(f"[resources] {name}: {found[0]}")
        assert found[0]["scratch"] == 0 and found[0]["vgpr_spill"] == 0, (name, found[0])
        assert found[0]["vgprs"] <= vgprs and found[0]["occupancy"] == 8, (name, found[0])
        assert found[0]["lds"] <= 256, (name, found[0])
    # the gather's own files know nothing of this part
    for other in ("pt_gather.hip", "pt_lmfilter.hip"):
        assert not [k for k in resources(other) if "pt_ag_" in k], other
