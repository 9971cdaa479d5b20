"""HAS_ENVIRONMENT_TEXTURE at its edges, on the CPU: the oracle's environment functions (oracle_env_probe) over the maps and inputs of
tests/env_cases.py -- black, one-hot, 1 x 1, one row, one column, odd sizes, inf / NaN / negative / subnormal texels -- against the numpy
restatement of tests/env_ref.py, against np.searchsorted, against a float64 blend, and against known answers.  What holds here is what
tests/test_gpu_env.py then holds the kernels to, bit for bit."""
import math

import numpy as np
import pytest

import env_cases as ec
import env_ref
import math_cases as mc

F32, F64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32).ravel()


def _same_bits(name, x, got, want):
    """bit for bit, a NaN matched by any NaN; x: one input word per output word, for the report"""
    x = np.ascontiguousarray(x).view(np.uint32).ravel()
    mc.assert_same_bits(name, x, np.zeros_like(x), _bits(got), _bits(want), "oracle", "restatement")


@pytest.mark.parametrize("name", ec.MAP_NAMES)
def test_cdf_and_search_equal_the_restatement(oracle, name):
    """what 0 and 1: the CDF in the order the loop of pt_env_cdf.h / MakeView writes it (memory order: cdf[y * W + x]), and both
    searches as literal loops, over every CDF entry with its float neighbours, +-0, the sum, twice the sum, negative, inf, NaN."""
    texels = ec.maps()[name]
    h, w = texels.shape[:2]
    want_cdf = env_ref.cdf(texels)
    got_cdf, total = ec.oracle_probe(name, 0)
    _same_bits(f"{name} cdf", np.arange(w * h, dtype=np.uint32), got_cdf[:, 0], want_cdf)
    assert _bits([total])[0] == _bits(want_cdf[-1:])[0] or (math.isnan(total) and np.isnan(want_cdf[-1]))
    assert not mc.mismatches(_bits(ec.cdf_of(texels)), _bits(want_cdf)).size            # what the input sets were built from
    values = ec.inputs(1, name)
    got, _ = ec.oracle_probe(name, 1)
    _same_bits(f"{name} search", np.repeat(values, 2), got, env_ref.binary_search(want_cdf, w, h, values))


@pytest.mark.parametrize("name", ec.MONOTONE_FINITE)
def test_search_is_searchsorted_on_monotone_maps(oracle, name):
    """Where the CDF is finite and monotone the searched cell is the first row whose LAST entry exceeds the value (the last row if
    none does), then the first column of that row whose entry exceeds it (the last column if none does)."""
    texels = ec.maps()[name]
    h, w = texels.shape[:2]
    c = env_ref.cdf(texels).reshape(h, w)
    assert np.isfinite(c).all() and (np.diff(c.ravel()) >= 0).all()
    values = ec.inputs(1, name)
    keep = ~np.isnan(values)
    values, got = values[keep], ec.oracle_probe(name, 1)[0][keep]
    yy = np.minimum(np.searchsorted(c[:, -1], values, side="right"), h - 1)
    xx = np.array([min(np.searchsorted(c[r], v, side="right"), w - 1) for r, v in zip(yy, values)])
    assert np.array_equal(got[:, 0], xx.astype(F32) / F32(w)) and np.array_equal(got[:, 1], yy.astype(F32) / F32(h))
    x, y = env_ref.binary_search_cell(c.ravel(), w, h, values)
    assert np.array_equal(y, yy) and np.array_equal(x, xx)


def _blend_error(texels, uv, got):
    """worst error of `got` (n, 3) against the float64 blend in ulps of the largest tap, over the elements whose blend is finite;
    elsewhere (an inf or NaN tap or weight) got must be inf / NaN exactly where the blend is"""
    ref, largest = env_ref.bilinear64(texels, uv)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        assert np.array_equal(np.isnan(got[~fin]), np.isnan(ref[~fin])) and np.array_equal(got[~fin][~np.isnan(ref[~fin])], ref[~fin][~np.isnan(ref[~fin])])
        ulp = np.maximum(np.spacing(largest.astype(F32)).astype(F64), 2.0 ** -149)
        err = np.abs(got.astype(F64) - ref) / ulp
    return float(err[fin].max()) if fin.any() else 0.0


def test_sample_level_against_a_float64_blend(oracle, capsys):
    """what 4 over every map and every uv pair.  The blend takes the restatement's float32 weights, so the rounding of the
    coordinates is not charged to it.  Prints the measured worst error; env_cases.BILINEAR_ULP_BOUND is twice the recorded one."""
    worst = {}
    for name in ec.MAP_NAMES:
        got, _ = ec.oracle_probe(name, 4)
        worst[name] = _blend_error(ec.maps()[name], ec.inputs(4, name), got)
    w = max(worst.values())
    with capsys.disabled():
        print(f"\n[env] bilinear: worst error {w:.4f} ulp of the largest tap ({max(worst, key=worst.get)}); recorded {ec.BILINEAR_ULP_MEASURED}, bound {ec.BILINEAR_ULP_BOUND}")
        print("[env] bilinear per map: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert abs(w - ec.BILINEAR_ULP_MEASURED) < 1e-3, "env_cases.BILINEAR_ULP_MEASURED is not what the oracle measures: re-derive the bound"
    assert ec.BILINEAR_ULP_BOUND == math.ceil(2 * ec.BILINEAR_ULP_MEASURED)
    assert w <= ec.BILINEAR_ULP_BOUND


def _finite_rows(a):
    return np.isfinite(a).all(axis=1)


@pytest.mark.parametrize("name", ec.CONSTANT)
def test_constant_map_returns_its_texel_exactly(oracle, name):
    """a + t (a - a) == a for every finite weight: what 4 at every finite uv pair, what 2 at every finite direction and every
    rotation, return the texel's bits."""
    texel = ec.maps()[name][0, 0, :3]
    got, _ = ec.oracle_probe(name, 4)
    ok = _finite_rows(ec.inputs(4, name))
    assert ok.sum() > 60000 and (_bits(got[ok]).reshape(-1, 3) == _bits(texel)[None, :]).all()
    for rotation in ec.ROTATIONS:
        got, _ = ec.oracle_probe(name, 2, rotation)
        ok = _finite_rows(ec.inputs(2, name))
        assert ok.sum() > 60000 and (_bits(got[ok, :3]).reshape(-1, 3) == _bits(texel)[None, :]).all(), rotation


@pytest.mark.parametrize("name", sorted(ec.ONE_HOT))
def test_one_hot_map_draws_its_texel(oracle, name):
    """On a one-hot map every draw with RandomFloat < 1 lands on the bright texel: zeros before it are stepped over (`value < cdf` is
    false at equality), and the colour is the texel's (its lattice point is that texel's corner).  A draw of exactly 1 is the
    sum itself, which no entry exceeds: both searches run to their last index, the cell is (W - 1, H - 1)."""
    texels = ec.maps()[name]
    h, w = texels.shape[:2]
    x, y = ec.ONE_HOT[name]
    states = ec.inputs(3, name)
    one = env_ref.random_float(states) == F32(1.0)
    assert one.sum() == 128 and (~one).sum() > 60000
    for rotation in (0.0, 0.15, -0.35):
        got, _ = ec.oracle_probe(name, 3, rotation)
        for mask, (cx, cy) in ((~one, (x, y)), (one, (w - 1, h - 1))):
            rows = got[mask]
            assert (_bits(rows).reshape(-1, 8) == _bits(rows[0])[None, :]).all(), "the draws of one cell differ"
            assert np.abs(rows[0, :3].astype(F64) - env_ref.lattice_direction(w, h, cx, cy, rotation)).max() < 2e-6, (rotation, cx, cy)


def _pdf_counts(pdf):
    return (int((pdf > 0).sum()), int((pdf < 0).sum()), int((pdf == 0).sum()), int(np.isnan(pdf).sum()))


def test_pdf_shares_per_map(oracle, capsys):
    """The sign of the pdf sample_env_map reports, per map, at rotation 0, counted over inputs(3, .) and held to the recorded counts.
    all-black: every pdf is 0 / 0; one inf texel: luminance / inf, exactly 0, or NaN on the texel itself; a negative pdf is a draw from
    memory row 0 (theta = fl(pi), pt_sin < 0): every draw of a one-row map, about 2.5 % of the ordinary sky's."""
    counts = {}
    for name in ec.MAP_NAMES:
        got, _ = ec.oracle_probe(name, 3)
        counts[name] = _pdf_counts(got[:, 3])
        n = len(got)
        with capsys.disabled():
            print(f"{chr(10) if name == ec.MAP_NAMES[0] else ''}[env] pdf shares {name}: > 0 {counts[name][0] / n:.4f}, < 0 {counts[name][1] / n:.4f}, == 0 {counts[name][2] / n:.4f}, NaN {counts[name][3] / n:.4f}   {counts[name]}")
    n = ec.N_MAX
    assert counts["black_w8h4"] == (0, 0, 0, n)
    assert counts["w1h1"] == (0, n, 0, 0) and counts["w8h1"] == (0, n, 0, 0)
    assert counts["one_inf_texel"][0] == 0 and counts["one_inf_texel"][1] == 0 and counts["one_inf_texel"][2] > 0
    assert 0.015 * n < counts["sky_w64h32"][1] < 0.035 * n and counts["sky_w64h32"][0] + counts["sky_w64h32"][1] == n
    assert counts == ec.PDF_COUNTS


def test_sin_theta_on_the_lattice_is_never_zero(oracle):
    """sample_env_map's theta is fl(v' * fl(pi)) with v' = 1 - y / H, y in 0 ... H - 1: for every height up to 1,024 pt_sin(theta) is
    negative in row 0 (theta = fl(pi), which lies above pi), positive in every other row and never 0 -- so `if (sinTheta == 0) pdf = 0`
    (util/sky.hlsl:80) never fires on a map, whatever its texels, and no test of frames or draws can tell whether it is there."""
    hs = np.arange(1, 1025)
    y = np.concatenate([np.arange(h) for h in hs]).astype(F32)
    h = np.repeat(hs, hs).astype(F32)
    v = F32(1.0) - y / h
    theta = v * F32(3.14159265358979323846)
    s = mc.floats(oracle.math_n(mc.FN["sin"], mc.bits(theta)))
    assert (s[y == 0] < 0).all() and (s[y > 0] > 0).all() and len(s) == 1024 * 1025 // 2


def test_rng_preimages_round_to_one(oracle):
    """env_cases' top states: one pt_rng_next step (the oracle's) takes them onto 0xFFFFFF80 ... 0xFFFFFFFF, whose float is 1."""
    top = ec.rng_preimages(np.arange(0xFFFFFF80, 0x100000000, dtype=np.uint64))
    assert np.array_equal(oracle.math_n(mc.FN["rng_next"], top), np.arange(0xFFFFFF80, 0x100000000, dtype=np.uint64).astype(np.uint32))
    assert np.array_equal(env_ref.rng_next(top), oracle.math_n(mc.FN["rng_next"], top))
    assert (mc.floats(oracle.math_n(mc.FN["random_float"], top)) == F32(1.0)).all()
    assert np.isin(top, ec.inputs(3, "sky_w64h32")).all()


def test_eval_env_map_colour_is_the_blend_at_its_own_uv(oracle):
    """what 2's colour against the float64 blend at the uv eval_env_map forms is covered on the device side by bit equality with the
    oracle; here the colour of every finite direction lies within the taps' range on the positive maps (a convex blend up to the bound)."""
    for name in ("sky_w64h32", "w5h3", "w7h2", "checker_w4h4"):
        t = ec.maps()[name][..., :3]
        lo, hi = float(t.min()), float(t.max())
        slack = ec.BILINEAR_ULP_BOUND * float(np.spacing(F32(hi)))
        for rotation in ec.ROTATIONS:
            got, _ = ec.oracle_probe(name, 2, rotation)
            ok = _finite_rows(ec.inputs(2, name))
            assert (got[ok, :3] >= lo - slack).all() and (got[ok, :3] <= hi + slack).all(), (name, rotation)
