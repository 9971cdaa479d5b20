"""Probe placement (include/ptmi_plugin.h Part 18) without a GPU: exports, struct layout, argument checks, the host twins against
the numpy restatement of the rule (tests/placement_ref.py) bit for bit, the constructed cases of the rule (ties, no hits, all back,
a NaN normal, the inside threshold, the offset limit to the ulp, stored offsets), the placed lookup's promises, the sanitizer build
of the host twins and the compile-time resources of the kernels.  tests/test_gpu_probe_placement.py holds the
kernels to the rule."""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from kernel_resources import resources
import placement_ref
import volume_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
F = np.float32
U = np.uint32
NONE = 0xFFFFFFFF
CONTEXT_SYMBOLS = ["PTProbePlace", "PTProbePlaceHost", "PTProbeGridIrradiancePlaced"]
HOST_SYMBOLS = ["PTProbePlaceStepHost", "PTProbeGridIrradiancePlacedHost"]
EPS = 2.0 ** -23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _b(x):
    """the bits of one float32"""
    return int(np.array([x], F).view(U)[0])


def _f(b):
    return np.array([b], U).view(F)[0]


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def _params(**kw):
    args = dict(spacing=(0.5, 0.75, 0.5), max_distance=1.5, min_front_distance=0.1, backface_share=0.25, max_offset=0.45, iterations=4)
    args.update(kw)
    return abi.probe_place_params(**args)


def _records(t, normals, hit=None):
    """(n, 4) hit rows and (n, 12) surface rows from t (n,), normals (n, 3) and hit (n,) bool (None: all)"""
    t = np.asarray(t, F)
    n = t.shape[0]
    hits, surf = np.zeros((n, 4), F), np.zeros((n, 12), F)
    hits[:, 0] = t
    prim = np.arange(n, dtype=U)
    if hit is not None:
        prim[~np.asarray(hit, bool)] = NONE
    hits[:, 3] = prim.view(F)
    surf[:, 3], surf[:, 4:7] = t, np.asarray(normals, F)
    return hits, surf


def _same_stats(a, b):
    return all((a[name].view(U) == b[name].view(U)).all() for name in a.dtype.names)


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_placement_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in CONTEXT_SYMBOLS + HOST_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 18: probe placement" in header


def test_placement_structs_match_c_header():
    fields = {"PTProbePlacement": ["offset", "state"],
              "PTProbePlaceParams": ["spacing", "maxDistance", "minFrontDistance", "backfaceShare", "maxOffset", "iterations"],
              "PTProbePlaceStats": ["back", "front", "nearestBack", "nearestFront", "farthestFront", "tNearestBack", "tNearestFront", "tFarthestFront"]}
    lines = []
    for s, fs in fields.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    lines.append('printf("flags %u %u %u\\n", PT_PROBE_INSIDE, PT_PLACE_KEEP_OFFSETS, PT_PLACE_MAX_ITERATIONS);')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTProbePlacement"]) == C.sizeof(abi.PTProbePlacement) == 16
    assert int(got["PTProbePlaceParams"]) == C.sizeof(abi.PTProbePlaceParams) == 32
    assert int(got["PTProbePlaceStats"]) == C.sizeof(abi.PTProbePlaceStats) == 32
    for s, fs in fields.items():
        for f in fs:
            assert int(got[f"{s}.{f}"]) == getattr(getattr(abi, s), f).offset, (s, f)
    assert [int(got[f"PTProbePlaceParams.{f}"]) for f in fields["PTProbePlaceParams"]] == [0, 12, 16, 20, 24, 28]
    st = np.dtype(abi.PLACE_STATS_DTYPE)
    assert st.itemsize == 32 and [st.fields[f][1] for f in fields["PTProbePlaceStats"]] == [int(got[f"PTProbePlaceStats.{f}"]) for f in fields["PTProbePlaceStats"]]
    assert np.dtype(placement_ref.STATS_DTYPE) == st
    assert got["flags"].split() == ["1", "1", "16"]
    assert (abi.PT_PROBE_INSIDE, abi.PT_PLACE_KEEP_OFFSETS, abi.PT_PLACE_MAX_ITERATIONS) == (1, 1, 16)


def _bad_params():
    return {"spacing 0": _params(spacing=(0.5, 0.0, 0.5)), "spacing negative": _params(spacing=(-1, 1, 1)), "spacing inf": _params(spacing=(1, 1, math.inf)),
            "spacing nan": _params(spacing=(math.nan, 1, 1)),
            "maxDistance 0": _params(max_distance=0.0), "maxDistance negative": _params(max_distance=-1.0), "maxDistance inf": _params(max_distance=math.inf),
            "maxDistance nan": _params(max_distance=math.nan), "maxDistance far": _params(max_distance=abi.PT_FAR_PLANE),
            "minFrontDistance negative": _params(min_front_distance=-0.1), "minFrontDistance inf": _params(min_front_distance=math.inf),
            "minFrontDistance nan": _params(min_front_distance=math.nan),
            "backfaceShare negative": _params(backface_share=-0.1), "backfaceShare 1.5": _params(backface_share=1.5), "backfaceShare nan": _params(backface_share=math.nan),
            "maxOffset negative": _params(max_offset=-0.1), "maxOffset 0.5": _params(max_offset=0.5), "maxOffset nan": _params(max_offset=math.nan),
            "iterations 17": _params(iterations=17)}


def test_placement_argument_errors():
    """every refusal of Part 18 that needs no scene: the context's entry points check their arguments before they touch the GPU"""
    lib = plugin.load_library()
    buf = (C.c_float * 1024)()
    a = (C.addressof(buf) + 15) & ~15
    ok = _params()
    grid = plugin.probe_grid_desc((0, 0, 0), (1, 1, 1), (2, 2, 2), wrap=False, visibility=False)
    calls = {"PTProbePlace": lambda: lib.PTProbePlace(None, a, 1, 0, 4, C.byref(ok), 0, a, a),
             "PTProbePlaceHost": lambda: lib.PTProbePlaceHost(None, a, 1, 0, 4, C.byref(ok), 0, a, a),
             "PTProbeGridIrradiancePlaced": lambda: lib.PTProbeGridIrradiancePlaced(None, C.byref(grid), a, a, a, a, 1, a)}
    for name, call in calls.items():
        assert call() == abi.PT_ERR_INVALID_ARG, name
        assert b"ctx" in lib.PTGetLastError() and name.encode() in lib.PTGetLastError()
    ctx = C.c_void_p(1)         # never dereferenced: every call below is refused on its arguments alone
    for fn in (lib.PTProbePlace, lib.PTProbePlaceHost):
        for name, q in _bad_params().items():
            assert fn(ctx, a, 1, 0, 4, C.byref(q), 0, a, a) == abi.PT_ERR_INVALID_ARG, name
            assert name.split()[0].encode() in lib.PTGetLastError(), (name, lib.PTGetLastError())
        assert fn(ctx, a, 1, 0, 4, None, 0, a, a) == abi.PT_ERR_INVALID_ARG and b"params" in lib.PTGetLastError()
        for bad in (2, 0x80000000, 3):
            assert fn(ctx, a, 1, 0, 4, C.byref(ok), bad, a, a) == abi.PT_ERR_INVALID_ARG and b"flag" in lib.PTGetLastError(), bad
        for bad in (0, 65537):
            assert fn(ctx, a, 1, 0, bad, C.byref(ok), 0, a, a) == abi.PT_ERR_UNSUPPORTED and b"samples" in lib.PTGetLastError(), bad
        assert fn(ctx, None, 1, 0, 4, C.byref(ok), 0, a, a) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
        assert fn(ctx, a, 1, 0, 4, C.byref(ok), 0, None, a) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    for args in ((a + 8, a, a), (a, a + 4, a), (a, a, a + 8)):
        assert lib.PTProbePlace(ctx, args[0], 1, 0, 4, C.byref(ok), 0, args[1], args[2]) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    # the placed lookup: the grid's refusals, the pointers
    bad_grid = plugin.probe_grid_desc((0, 0, 0), (1, 0, 1), (2, 2, 2), wrap=False, visibility=False)
    assert lib.PTProbeGridIrradiancePlaced(ctx, C.byref(bad_grid), a, a, a, a, 1, a) == abi.PT_ERR_INVALID_ARG and b"spacing" in lib.PTGetLastError()
    assert lib.PTProbeGridIrradiancePlaced(ctx, None, a, a, a, a, 1, a) == abi.PT_ERR_INVALID_ARG
    vis = plugin.probe_grid_desc((0, 0, 0), (1, 1, 1), (2, 2, 2), wrap=False, visibility=True)
    assert lib.PTProbeGridIrradiancePlaced(ctx, C.byref(vis), a, None, a, a, 1, a) == abi.PT_ERR_INVALID_ARG and b"depth" in lib.PTGetLastError()
    assert lib.PTProbeGridIrradiancePlacedHost(C.byref(vis), a, None, a, a, 1, a) == 0 and b"depth" in lib.PTGetBVHBuildError()
    assert lib.PTProbeGridIrradiancePlacedHost(C.byref(bad_grid), a, a, a, a, 1, a) == 0 and b"spacing" in lib.PTGetBVHBuildError()
    for args in ((None, a, a), (a, None, a), (a, a, None)):
        assert lib.PTProbeGridIrradiancePlaced(ctx, C.byref(grid), args[0], a, a, args[1], 1, args[2]) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    for args in ((a + 8, a, a, a, a), (a, a + 8, a, a, a), (a, a, a + 8, a, a), (a, a, a, a + 4, a), (a, a, a, a, a + 8)):
        assert lib.PTProbeGridIrradiancePlaced(ctx, C.byref(grid), args[0], args[1], args[2], args[3], 1, args[4]) == abi.PT_ERR_INVALID_ARG
        assert b"aligned" in lib.PTGetLastError()
    # the twin: 0 and a message
    for name, q in _bad_params().items():
        assert lib.PTProbePlaceStepHost(a, 1, 0, 4, C.byref(q), a, a, 1, a, None) == 0 and name.split()[0].encode() in lib.PTGetBVHBuildError(), name
    assert lib.PTProbePlaceStepHost(a, 1, 0, 4, None, a, a, 1, a, None) == 0 and b"params" in lib.PTGetBVHBuildError()
    for bad in (0, 65537):
        assert lib.PTProbePlaceStepHost(a, 1, 0, bad, C.byref(ok), a, a, 1, a, None) == 0 and b"samples" in lib.PTGetBVHBuildError()
    for args in ((None, a, a, a), (a, None, a, a), (a, a, None, a), (a, a, a, None)):
        assert lib.PTProbePlaceStepHost(args[0], 1, 0, 4, C.byref(ok), args[1], args[2], 1, args[3], None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTProbePlaceStepHost(None, 0, 0, 4, C.byref(ok), None, None, 1, None, None) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------------
def _step(pos, hits, surf, q, move, stored, first_sample, seeds):
    """the twin and the restated rule over the same records: both results"""
    n = len(pos)
    samples = hits.shape[0] // n
    got = plugin.probe_place_step(pos, hits, surf, q, move=move, offsets=stored, first_sample=first_sample, seeds=seeds)
    d = plugin.probe_directions(pos, samples, first_sample=first_sample, seeds=seeds)[:, 3:6].reshape(n, samples, 3)
    want = placement_ref.steps(d, hits, surf, np.zeros((n, 3), F) if stored is None else stored, q, move)
    return got, want, d


@pytest.mark.parametrize("samples", [1, 2, 63, 64, 65, 70, 4096])
@pytest.mark.parametrize("move", [False, True])
def test_step_host_equals_the_restated_rule(samples, move):
    """random records: a third misses, a third back, a third front (the normal is the direction, or its opposite, bent a little)"""
    n, first, seeds = 4, 0xFFFFFFF0, [3, 0xFFFFFFF6, 11, 12]
    rng = np.random.default_rng(samples * 2 + int(move))
    pos = rng.uniform(-1, 1, (n, 3)).astype(F)
    q = _params(backface_share=0.3)
    d = plugin.probe_directions(pos, samples, first_sample=first, seeds=seeds)[:, 3:6]
    kind = rng.integers(0, 3, n * samples)                                  # 0 miss, 1 back, 2 front
    normals = _unit(np.where(kind[:, None] == 1, 1.0, -1.0) * d + rng.normal(0, 0.3, d.shape))
    t = rng.uniform(0.002, 0.4, n * samples).astype(F)
    t[rng.integers(0, n * samples, max(n * samples // 8, 1))] = F(0.05)     # equal distances
    t[kind == 0] = F(q.maxDistance)
    hits, surf = _records(t, normals, kind != 0)
    stored = np.array([(0, 0, 0), (0.05, -0.1, 0.02), (math.nan, 0, 0), (0.2, 0.3, -0.2)], F)
    got, want, _ = _step(pos, hits, surf, q, move, stored, first, seeds)
    assert (_bits(got[0]) == _bits(want[0])).all(), (got[0], want[0])
    assert (got[1] == want[1]).all(), (got[1], want[1])
    assert _same_stats(got[2], want[2]), (got[2], want[2])
    assert (got[2]["back"] + got[2]["front"] == (kind != 0).reshape(n, samples).sum(axis=1)).all()
    if samples >= 63:
        assert (got[2]["back"] > 0).all() and (got[2]["front"] > 0).all()
        if move:
            assert (_bits(got[0]) != _bits(placement_ref.steps(np.zeros((n, samples, 3), F), hits, surf, stored, q, False)[0])).any(), "no probe moved"
    print(f"[placement] {samples} samples, move {move}: back {got[2]['back']}, front {got[2]['front']}, states {got[1]}")


def _one(samples, t, normals, hit=None, q=None, move=True, stored=None, seed=9, first=0):
    q = q or _params()
    pos = np.array([(0.1, 0.2, 0.3)], F)
    hits, surf = _records(t, normals, hit)
    got, want, d = _step(pos, hits, surf, q, move, stored, first, [seed])
    assert (_bits(got[0]) == _bits(want[0])).all() and (got[1] == want[1]).all() and _same_stats(got[2], want[2]), (got, want)
    return got[0][0], int(got[1][0]), got[2][0], d[0]


@pytest.mark.parametrize("gap", [1, 64])
@pytest.mark.parametrize("side", ["back", "front"])
def test_equal_distances_go_to_the_lowest_sample(gap, side):
    """two samples with equal t at j and j + 1, and at j and j + 64 (the same lane's next round): the lowest j is the nearest and
    the farthest"""
    samples, j = 130, 5
    d = plugin.probe_directions(np.array([(0.1, 0.2, 0.3)], F), samples, seeds=[9])[:, 3:6]
    sign = 1.0 if side == "back" else -1.0
    t = np.full(samples, 0.3, F)
    t[[j, j + gap]] = F(0.05)                            # the nearest, twice
    far = [j + 2, j + 2 + gap]
    t[far] = F(0.7)                                      # the farthest, twice
    off, state, st, _ = _one(samples, t, (sign * d).astype(F), move=False)
    if side == "back":
        assert (st["back"], st["front"]) == (samples, 0) and state == abi.PT_PROBE_INSIDE
        assert st["nearestBack"] == j and _bits(st["tNearestBack"]) == _bits(F(0.05))
        assert st["nearestFront"] == NONE and st["farthestFront"] == NONE and st["tNearestFront"] == 0 and st["tFarthestFront"] == 0
    else:
        assert (st["back"], st["front"]) == (0, samples) and state == 0
        assert st["nearestFront"] == j and st["farthestFront"] == j + 2 and _bits(st["tFarthestFront"]) == _bits(F(0.7))
        assert st["nearestBack"] == NONE and st["tNearestBack"] == 0


def test_no_hit_leaves_the_probe_where_it_is():
    samples = 70
    stored = np.array([(0.1, -0.2, 0.05)], F)
    off, state, st, _ = _one(samples, np.full(samples, 1.5, F), np.zeros((samples, 3), F), hit=np.zeros(samples, bool), stored=stored)
    assert (st["back"], st["front"], state) == (0, 0, 0)
    assert st["nearestBack"] == st["nearestFront"] == st["farthestFront"] == NONE
    assert st["tNearestBack"] == st["tNearestFront"] == st["tFarthestFront"] == 0
    assert (_bits(off) == _bits(stored[0])).all()


def test_all_back_moves_through_the_nearest_face():
    samples = 70
    d = plugin.probe_directions(np.array([(0.1, 0.2, 0.3)], F), samples, seeds=[9])[:, 3:6]
    t = np.linspace(0.08, 0.2, samples).astype(F)
    t[33] = F(0.04)
    q = _params(min_front_distance=0.1)
    off, state, st, w = _one(samples, t, d, q=q)
    assert (st["back"], st["front"], st["nearestBack"], state) == (samples, 0, 33, abi.PT_PROBE_INSIDE)
    length = F(F(0.04) + F(F(q.minFrontDistance) * F(0.5)))
    assert (_bits(off) == _bits((w[33] * length).astype(F))).all()           # o = 0: 0 + w * len


def test_a_nan_normal_counts_as_front():
    samples = 8
    d = plugin.probe_directions(np.array([(0.1, 0.2, 0.3)], F), samples, seeds=[9])[:, 3:6]
    normals = d.copy()
    normals[2] = (math.nan, 0.0, 0.0)
    normals[5] = (math.nan, math.nan, math.nan)
    off, state, st, _ = _one(samples, np.full(samples, 0.5, F), normals, move=False)
    assert (st["back"], st["front"]) == (6, 2) and st["nearestFront"] == 2 and st["farthestFront"] == 2


@pytest.mark.parametrize("back, inside", [(16, False), (17, True)])
def test_the_inside_threshold(back, inside):
    """64 samples and backfaceShare = 0.25: 16 back samples are not inside, 17 are"""
    samples = 64
    d = plugin.probe_directions(np.array([(0.1, 0.2, 0.3)], F), samples, seeds=[9])[:, 3:6]
    sign = np.where(np.arange(samples) < back, 1.0, -1.0)[:, None]
    off, state, st, _ = _one(samples, np.full(samples, 0.5, F), (sign * d).astype(F), q=_params(backface_share=0.25), move=False)
    assert (st["back"], st["front"]) == (back, samples - back)
    assert state == (abi.PT_PROBE_INSIDE if inside else 0)


@pytest.mark.parametrize("ulps, accepted", [(0, True), (-1, True), (1, False)])
def test_the_offset_limit_to_the_ulp(ulps, accepted):
    """A candidate on the limit and one ulp inside it is accepted, one ulp outside is refused and leaves o bit for bit.  One sample,
    seen from the front at distance 0: the candidate is o - w * minFrontDistance; the stored o is chosen so that the y component
    lands where it should (x and z stay far inside)."""
    q = _params(spacing=(4.0, 0.75, 4.0), min_front_distance=0.05, max_offset=0.45)
    lim = F(F(q.maxOffset) * F(q.spacing[1]))
    w = plugin.probe_directions(np.array([(0.1, 0.2, 0.3)], F), 1, seeds=[9])[0, 3:6]
    assert abs(w[1]) > 0.01
    step = F(w[1] * F(F(q.minFrontDistance) - F(0.0)))                     # cand.y = y - step
    sign = F(-1.0) if step > 0 else F(1.0)                                # the move goes along -w
    target = _f(_b(lim) + ulps) * sign
    found = None
    y0 = F(target + step)
    for k in range(-4, 5):                                               # a stored y with y - step == target in float32
        y = _f(_b(y0) + k)
        if _b(F(y - step)) == _b(target) and abs(y) <= lim:
            found = y
            break
    assert found is not None, (y0, step, target)
    stored = np.array([(0.0, found, 0.0)], F)
    off, state, st, _ = _one(1, np.zeros(1, F), (-w).reshape(1, 3).astype(F), q=q, stored=stored)
    assert (st["front"], st["nearestFront"]) == (1, 0)
    if accepted:
        assert _b(off[1]) == _b(target) and abs(off[1]) <= lim and _b(off[1]) != _b(found)
    else:
        assert abs(target) > lim and (_bits(off) == _bits(stored[0])).all()


def test_stored_offsets_out_of_limit_read_as_zero():
    """PT_PLACE_KEEP_OFFSETS on the twin's inout: a stored offset past the limit on one axis, or with a NaN, is read as 0, whole"""
    samples = 4
    q = _params()                                                         # limits 0.225, 0.3375, 0.225
    miss = np.zeros(samples, bool)
    lim = (F(q.maxOffset) * np.array([q.spacing[a] for a in range(3)], F)).astype(F)
    for stored, kept in (((0.2, -0.3, 0.1), True), ((0.23, 0.0, 0.0), False), ((0.1, 0.1, -0.3), False), ((0.0, math.nan, 0.0), False),
                         ((math.inf, 0.0, 0.0), False), ((lim[0], lim[1], -lim[2]), True), ((lim[0], _f(_b(lim[1]) + 1), 0.0), False)):
        for move in (False, True):
            off, state, st, _ = _one(samples, np.full(samples, 1.5, F), np.zeros((samples, 3), F), hit=miss, q=q, stored=np.array([stored], F), move=move)
            want = np.array(stored, F) if kept else np.zeros(3, F)
            assert (_bits(off) == _bits(want)).all(), (stored, off)


# ---------------------------------------------------------------------------------------------------------------------------
# the placed lookup
# ---------------------------------------------------------------------------------------------------------------------------
_ORIGIN, _SPACING = (-0.5, 0.25, -0.75), (0.5, 0.75, 0.625)


def _grid(origin, spacing, counts, flags=0, bias=0.0):
    return plugin.probe_grid_desc(origin, spacing, counts, wrap=bool(flags & 1), visibility=bool(flags & 2), normal_bias=bias)


def _queries(counts, rng):
    """the query kinds of tests/test_probe_volume.py: inside, outside every face, on a probe, on the last plane, a NaN, far off a corner"""
    hi = [_ORIGIN[a] + _SPACING[a] * (counts[a] - 1) for a in range(3)]
    inside = np.stack([rng.uniform(_ORIGIN[a], max(hi[a], _ORIGIN[a] + 1e-3), 12) for a in range(3)], axis=1)
    outside = []
    for a in range(3):
        for side in (-1, 1):
            p = [0.5 * (_ORIGIN[b] + hi[b]) + 0.1 for b in range(3)]
            p[a] = _ORIGIN[a] - 0.7 if side < 0 else hi[a] + 0.7
            outside.append(p)
    on_probe = [_ORIGIN[0], _ORIGIN[1], _ORIGIN[2]]
    last_plane = [hi[0], 0.5 * (_ORIGIN[1] + hi[1]) + 0.05, hi[2]]
    nan = [math.nan, 0.5, 0.5]
    corner = [hi[0] + 3.0, hi[1] + 3.0, _ORIGIN[2] - 3.0]
    P = np.array(list(inside) + outside + [on_probe, last_plane, nan, corner], F)
    N = _unit(rng.normal(0, 1, P.shape))
    return P, N


def _volume(counts, rng):
    n = counts[0] * counts[1] * counts[2]
    sh = rng.normal(0.3, 1, (n, 9, 3)).astype(F)
    mean = rng.uniform(0.1, 1.2, (n, 64)).astype(F)
    depth = np.stack([mean, mean * mean + rng.uniform(0, 0.05, (n, 64)).astype(F)], axis=2).astype(F)
    return n, sh, depth


@pytest.mark.parametrize("counts", [(3, 2, 2), (1, 1, 1), (2, 1, 3)])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_placed_lookup_host_equals_the_restated_rule(counts, flags):
    rng = np.random.default_rng(300 + sum(counts))
    n, sh, depth = _volume(counts, rng)
    P, N = _queries(counts, rng)
    bias = 0.0 if flags in (0, 3) else 0.03
    g = _grid(_ORIGIN, _SPACING, counts, flags, bias)
    d = depth if flags & 2 else None
    # without a placement: Part 16's lookup, bit for bit
    plain = plugin.probe_grid_irradiance(g, sh, d, P, N)
    lib = plugin.load_library()
    rows, recv, same = plugin.probe_coeff_rows(sh), plugin.receiver_rows(P, N), np.empty((len(P), 4), F)
    assert lib.PTProbeGridIrradiancePlacedHost(C.byref(g), rows.ctypes.data, None if d is None else d.ctypes.data, None, recv.ctypes.data, len(P), same.ctypes.data) == 1
    assert (_bits(same) == _bits(plain)).all()
    # random offsets (some -0.0, some 0) and states
    off = (rng.uniform(-0.45, 0.45, (n, 3)) * np.array(_SPACING)).astype(F)
    off[rng.uniform(0, 1, (n, 3)) < 0.2] = F(-0.0)
    states = (rng.uniform(0, 1, n) < 0.3).astype(U)
    if n > 1:
        states[0], states[1] = 0, 1
    pl = plugin.probe_placement_rows(off, states)
    got = plugin.probe_grid_irradiance(g, sh, d, P, N, placement=pl)
    for k in range(len(P)):
        rgb, sw = placement_ref.lookup(_ORIGIN, _SPACING, counts, flags, bias, sh, depth, pl, P[k], N[k])
        assert (_bits(got[k, :3]) == _bits(rgb)).all() and _bits(got[k, 3:4])[0] == _bits(sw), (k, got[k], rgb, sw)
    if n > 1:
        assert (_bits(got) != _bits(plain)).any()
    # every corner buried: rgb 0 and m2 = 0
    buried = plugin.probe_grid_irradiance(g, sh, d, P, N, placement=plugin.probe_placement_rows(off, np.ones(n, U)))
    assert (_bits(buried) == 0).all()
    # zero offsets and live states: the plain lookup's values (the add of +0 can only turn a -0 into +0, which no later step keeps)
    zero = plugin.probe_grid_irradiance(g, sh, d, P, N, placement=plugin.probe_placement_rows(None, None, n))
    finite = np.isfinite(plain).all(axis=1)
    assert (zero[finite] == plain[finite]).all()


def test_one_of_two_probes_buried_gives_the_other_probe():
    g = _grid((0, 0, 0), (1, 1, 1), (2, 1, 1))
    rng = np.random.default_rng(21)
    sh = rng.uniform(0.2, 1.0, (2, 9, 3)).astype(F)
    sh[:, 1:] *= F(0.2)
    P = np.array([(0.8, 0.0, 0.0), (0.25, 0.3, -0.2)], F)
    N = _unit([(0.3, 0.9, 0.2), (0.0, 0.0, 1.0)])
    pl = plugin.probe_placement_rows(np.zeros((2, 3), F), [abi.PT_PROBE_INSIDE, 0])
    got = plugin.probe_grid_irradiance(g, sh, None, P, N, placement=pl)
    own = plugin.probe_irradiance(sh, N, [1, 1])[:, :3].astype(np.float64)
    rel = np.abs(got[:, :3] - own) / own
    print(f"[placement] one of two buried: relative difference to the live probe's own E {rel.max():.2e}")
    assert rel.max() <= 4 * EPS                                          # (w * E) / w
    # m2 is the live corner's weight: its trilinear weight, the flags being off (crush leaves 1 alone)
    assert _bits(got[0, 3:4])[0] == _bits(np.array([0.8], F))[0] and _bits(got[1, 3:4])[0] == _bits(np.array([0.25], F))[0]


def test_a_buried_black_probe_no_longer_darkens_its_cell():
    """coefficients of constant 1 on the live probes and 0 on one buried probe: the placed lookup gives 1 at every query, within
    the bound of the "equal probes" case of tests/test_probe_volume.py; the unplaced lookup with the flags off gives 1 - tri_buried"""
    counts = (3, 2, 2)
    rng = np.random.default_rng(5)
    buried = 4                                                            # (ix, iy, iz) = (1, 1, 0)
    one = np.zeros((9, 3), F)
    one[0] = F(1.0 / (3.14159265 * 0.28209479))                          # E(N) = A_0 * sh * Y_0 = 1 up to rounding
    sh = np.tile(one[None], (12, 1, 1))
    sh[buried] = 0
    hi = [_ORIGIN[a] + _SPACING[a] * (counts[a] - 1) for a in range(3)]
    P = np.stack([rng.uniform(_ORIGIN[a], hi[a], 40) for a in range(3)], axis=1).astype(F)
    N = _unit(rng.normal(0, 1, P.shape))
    g = _grid(_ORIGIN, _SPACING, counts)
    states = np.zeros(12, U)
    states[buried] = abi.PT_PROBE_INSIDE
    want = plugin.probe_irradiance(one[None], N, np.zeros(len(P), U))[:, :3].astype(np.float64)
    got = plugin.probe_grid_irradiance(g, sh, None, P, N, placement=plugin.probe_placement_rows(np.zeros((12, 3), F), states))
    rel = np.abs(got[:, :3] - want) / want
    print(f"[placement] buried black probe: largest relative difference of the placed lookup to 1 {rel.max():.2e}")
    assert np.abs(want - 1.0).max() < 1e-6 and rel.max() <= 4 * EPS
    # unplaced: the black probe takes its trilinear share away
    plain = plugin.probe_grid_irradiance(g, sh, None, P, N).astype(np.float64)
    Q = volume_ref.grid_positions(_ORIGIN, _SPACING, counts)[buried].astype(np.float64)
    tri = np.prod(np.maximum(1.0 - np.abs(P.astype(np.float64) - Q) / np.array(_SPACING), 0.0), axis=1)
    assert (tri > 0.05).any()
    assert np.abs(plain[:, 0] - (1.0 - tri) * want[:, 0]).max() <= 1e-6
    assert np.abs(got[:, 3] - (1.0 - tri)).max() <= 1e-6                  # and the placed support is what the others hold


# ---------------------------------------------------------------------------------------------------------------------------
# the rest
# ---------------------------------------------------------------------------------------------------------------------------
def test_placement_sanitize_target_runs_clean():
    """the host twins under AddressSanitizer + UBSan in a stand-alone program (csrc/placement_sanitize_main.cpp)"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", CSRC, "placement-sanitize", "PLACEMENT_SANITIZE_OUT=" + os.path.join(d, "placement_sanitize")],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "placement ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


KERNELS = ["pt_probe_place_rays", "pt_probe_place_step", "pt_probe_grid_irradiance_placed"]
SHADE_VGPR_BUDGET = 128             # what tests/test_kernel_resources.py holds pt_wf_shade<false, PTRayMap> to


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_placement_kernels_fit_the_shade_kernels_budget():
    res = resources("pt_placement.hip")
    assert len(res) == len(KERNELS), sorted(res)
    for name in KERNELS:
        hits = [r for k, r in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1, (name, sorted(res))
        r = hits[0]
        print(f"[resources] {name}: {r}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgprs"] <= SHADE_VGPR_BUDGET, (name, r)
    step = [r for k, r in res.items() if "pt_probe_place_step" in k][0]
    assert step["lds"] == 0, step                                         # the merge is cross-lane, not through LDS


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU tests' scene in closed form: what tests/test_gpu_probe_placement.py's composition case must not be empty of
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_composition_probes_cover_every_outcome():
    """the twin over plane distances (tests/placement_cases.py), 70 samples and 3 iterations: a probe ends buried, probes move, a
    probe stays on its grid point and live -- so the bit-for-bit comparison on the GPU compares all three"""
    import placement_cases
    q = abi.probe_place_params(0.5, min_front_distance=0.1, iterations=3)
    off, states, st = placement_cases.place(placement_cases.PROBES, placement_cases.SEEDS, 70, q)
    moved = (off != 0).any(axis=1)
    print(f"[placement] closed form, 70 samples, 3 iterations: states {states}, |offset| {np.linalg.norm(off, axis=1)}, back {st['back']}, front {st['front']}")
    assert list(states) == [0, 0, 0, 0, abi.PT_PROBE_INSIDE]
    assert list(moved) == [True, True, False, True, False]
    assert not placement_cases.in_cube(placement_cases.PROBES[0] + off[0]) and placement_cases.in_cube(placement_cases.PROBES[0])
    assert (np.abs(off) <= F(0.45) * F(0.5)).all()
    # without a relocation step the cube's probe is buried: every sample sees a face from behind
    q0 = abi.probe_place_params(0.5, min_front_distance=0.1, iterations=0)
    off0, states0, st0 = placement_cases.place(placement_cases.PROBES, placement_cases.SEEDS, 70, q0)
    assert (off0 == 0).all() and list(states0) == [1, 0, 0, 0, 1] and st0["back"][0] == 70 and st0["front"][0] == 0
