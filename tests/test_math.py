"""include/ptmi_math.h: the canonical elementary functions stay within a few ulp of libm, and the RNG
reproduces the known-answer vectors computed from util/random.hlsl:5-16."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import math_cases as mc
from math_cases import FN


def _ulp_err(got, ref64):
    return mc.ulp_err(mc.bits(got), ref64)


def _apply(lib, fn, x, y=None):
    """Float32 arrays in and out through the batch entry (oracle_math_n, bit patterns); a uint32 array is passed as the integers."""
    as_bits = lambda a: a if a.dtype == np.uint32 else mc.bits(a)
    from oracle import pyoracle
    return mc.floats(pyoracle.math_n(fn, as_bits(x), None if y is None else as_bits(y), lib=lib))


@pytest.fixture(scope="module")
def lib(oracle):
    return oracle.load_oracle()


@pytest.fixture(scope="module")
def evaluate(oracle):
    """evaluate(fn, xbits, ybits=None) -> result bits: the oracle's evaluation of include/ptmi_math_switch.h."""
    return oracle.math_n


def test_sin_cos(lib):
    rng = np.random.RandomState(1)
    x = rng.uniform(0.0, 6.3, 20000).astype(np.float32)          # the shader only passes angles in [0, 2pi]
    assert np.abs(_apply(lib, 0, x) - np.sin(x.astype(np.float64))).max() < 1.5e-7
    assert np.abs(_apply(lib, 1, x) - np.cos(x.astype(np.float64))).max() < 1.5e-7
    big = rng.uniform(-2000.0, 2000.0, 5000).astype(np.float32)
    assert np.abs(_apply(lib, 0, big) - np.sin(big.astype(np.float64))).max() < 2e-6


def test_log_exp_pow_acos(lib):
    rng = np.random.RandomState(2)
    u = np.exp(-rng.uniform(0, 80, 20000)).astype(np.float32)
    assert _ulp_err(_apply(lib, 2, u), np.log(u.astype(np.float64))).max() <= 2.0
    assert _ulp_err(_apply(lib, 3, u), np.log2(u.astype(np.float64))).max() <= 3.0
    e = rng.uniform(-125, 125, 20000).astype(np.float32)
    assert _ulp_err(_apply(lib, 4, e), np.exp2(e.astype(np.float64))).max() <= 3.0
    a = rng.uniform(-1, 1, 20000).astype(np.float32)
    assert _ulp_err(_apply(lib, 6, a), np.arccos(a.astype(np.float64))).max() <= 3.0
    b = rng.uniform(1e-6, 1.0, 5000).astype(np.float32)
    y = rng.uniform(0, 1, 5000).astype(np.float32)
    rel = np.abs(_apply(lib, 5, b, y).astype(np.float64) / np.power(b.astype(np.float64), y.astype(np.float64)) - 1)
    assert rel.max() < 5e-6                                        # pow = exp2(y*log2(x)), as HLSL defines it


def test_atan2_fmod(lib):
    """Environment-map lookups (util/sky.hlsl:46-53) need atan2 and fmod."""
    rng = np.random.RandomState(3)
    y = rng.normal(0, 1, 20000).astype(np.float32)
    x = rng.normal(0, 1, 20000).astype(np.float32)
    got = _apply(lib, 10, y, x)
    assert np.abs(got - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() < 4e-7
    f = lambda a, b: lib.oracle_math(10, a, b)
    assert f(0.0, 0.0) == 0.0 and f(1.0, 0.0) == np.float32(np.pi / 2) and f(-1.0, 0.0) == np.float32(-np.pi / 2)
    assert f(0.0, -1.0) == np.float32(np.pi) and f(0.0, 1.0) == 0.0 and np.isnan(f(float("nan"), 1.0))
    a = rng.uniform(-3, 3, 5000).astype(np.float32)
    m = _apply(lib, 11, a, np.ones_like(a))
    assert np.array_equal(m, np.fmod(a, np.float32(1.0)))           # HLSL fmod keeps the sign of x, like C fmod


def test_special_values(lib):
    f = lambda fn, x, y=0.0: lib.oracle_math(fn, x, y)
    assert f(2, 1.0) == 0.0 and f(4, 0.0) == 1.0 and f(6, 1.0) == 0.0
    assert f(2, 0.0) == -np.inf and np.isnan(f(2, -1.0)) and np.isnan(f(6, 1.5))
    assert f(5, 0.0, 0.5) == 0.0 and f(5, 0.25, 0.5) == 0.5 and f(5, 1.0, 2.2) == 1.0
    assert f(4, -130.0) > 0 and f(4, 200.0) == np.inf
    assert f(8, 4.0) == 2.0 and f(9, 4.0) == 0.25 and f(9, 0.0) == np.inf


KNOWN = {   # state after each call : float returned
    0x00000000: [(0xa8beea3c, 0.659163117), (0x0a2a1484, 0.039704591), (0x1e93be90, 0.119441897), (0x75134d09, 0.457325757)],
    0x00000001: [(0xb94dd992, 0.723844171), (0x7d3246cc, 0.489048421), (0xcb994a9c, 0.795307815), (0x4dd1f399, 0.303984851)],
    0x12345678: [(0x199714cb, 0.0999615639), (0xe91f039e, 0.910629511), (0x76c6835c, 0.463966578), (0xbc936622, 0.736624122)],
    0xffffffff: [(0x982ff7a5, 0.594481945), (0xbefdfcf3, 0.746063054), (0x37723005, 0.216586113), (0xd7a537c4, 0.842364788)],
}


def test_rng_known_answers(lib):
    for seed, seq in KNOWN.items():
        s = C.c_uint32(seed)
        for state, value in seq:
            f = lib.oracle_random_float(C.byref(s))
            assert s.value == state
            assert np.float32(f) == np.float32(value)


def test_rng_top_states_round_to_one(lib):
    """(float)0xFFFFFF80 / 2^32 == 1.0: RandomFloat is inclusive of 1 -- the reason the light
    pick is clamped and the reason NaN NEE directions exist (util/random.hlsl:34-41)."""
    assert np.float32(0xFFFFFF7F) / np.float32(4294967296.0) < 1.0
    assert np.float32(0xFFFFFF80) / np.float32(4294967296.0) == 1.0
    # per-pixel seed example of SURVEY.md Appendix D: W = 256, pixel (10, 3), CurrentSample 0
    assert (3 * 256 + 10) * (0 + 1) + 0x12345678 == 0x12345982


def test_texture_wrap_closed_form_equals_the_reference_loops(lib):
    """util/texture.hlsl:41-48 wraps with `while (u > 1) u -= 1; while (u < 0) u += 1`.  The kernels use the closed form
    pt_wrap01 (bounded cost, no hang for huge / infinite uv); it must give the literal loops' result bit for bit."""
    rng = np.random.RandomState(5)
    vals = np.concatenate([
        rng.uniform(-8, 8, 4000), rng.uniform(-3000, 3000, 3000), rng.normal(0, 1e-6, 500), rng.uniform(-2e5, 2e5, 300),
        np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 1.0000001, -1.0000001, 0.99999994, -1e-10, 1e-10, 3.5, -2.5, 4096.0, -4096.0,
                  16777215.0, -16777215.0, 16777216.0, -16777216.0, 3e7, -3e7, 1e30, float("inf"), float("-inf")]),
        np.arange(-40, 40) + np.float32(2 ** -23), np.arange(-40, 40) - np.float32(2 ** -23),
    ]).astype(np.float32)
    closed = _apply(lib, 12, vals)
    loops = _apply(lib, 13, vals)
    assert np.array_equal(closed.view(np.uint32), loops.view(np.uint32))
    assert ((closed >= 0) & (closed <= 1)).all()
    assert np.isnan(lib.oracle_math(12, float("nan"), 0.0)) and np.isnan(lib.oracle_math(13, float("nan"), 0.0))


def test_unorm8_equals_division_by_255_for_every_byte(lib):
    """The kernels turn a texel channel into a float with pt_unorm8 (mul + 2 fma); the oracle divides by 255 as
    util/texture.hlsl does.  All 256 inputs, bit for bit."""
    b = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.array([lib.oracle_math(14, float(v), 0.0) for v in b], dtype=np.float32), b / np.float32(255.0))
    fast = _apply(lib, 14, b.astype(np.uint32))
    div = _apply(lib, 15, b.astype(np.uint32))
    assert np.array_equal(fast.view(np.uint32), div.view(np.uint32))
    assert np.array_equal(div, (b / np.float32(255.0)).astype(np.float32))
    # ... and the same bytes with high bits set (pt_unorm8 masks with 0xFF), and any 32 bits at all
    u = mc.cases("unorm8")[0]
    want = ((u & 0xFF).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    assert np.array_equal(_apply(lib, 14, u).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(_apply(lib, 15, u).view(np.uint32), want.view(np.uint32))


# ---- the header function by function, on the input sets of tests/math_cases.py (shared with tests/test_gpu_math.py) -------------------
def test_accuracy_on_the_domain_sets(evaluate):
    """log <= 2, log2 <= 3, exp2 <= 3, acos <= 3, asin / atan <= 4 ulp of the float32 rounding of numpy's float64 result (ulp floored at
    2^-149: subnormal arguments of log and subnormal results of exp2 count); sin / cos <= 1.5e-7 absolute over [0, 2 pi] and the whole
    reach of the reduction, +-1.2e4."""
    mc.check_accuracy(evaluate)


def test_pow_is_exp2_of_y_log2_x_on_the_wide_set(evaluate):
    """pow(x, y) == exp2(fl(y * log2(x))), bit for bit, composed from the oracle's own log2 and exp2 and one float32 multiplication in
    numpy: bases over all positive exponents, exponents in +-40, the named special cases, the specials grid and random bit patterns."""
    x, y = mc.cases("pow")
    with np.errstate(all="ignore"):
        t = mc.floats(y) * mc.floats(evaluate(FN["log2"], x))
    mc.assert_same_bits("pow", x, y, evaluate(FN["pow"], x, y), evaluate(FN["exp2"], mc.bits(t)), "pow", "exp2(y*log2 x)")
    f = lambda a, b: mc.floats(evaluate(FN["pow"], mc.bits([a]), mc.bits([b])))[0]
    inf = float("inf")
    assert np.isnan(f(0.0, 0.0)) and f(0.0, 2.0) == 0.0 and f(0.0, -2.0) == inf and np.isnan(f(-2.0, 2.0))        # HLSL's pow, not C's
    assert np.isnan(f(1.0, inf)) and np.isnan(f(1.0, -inf)) and f(inf, 2.0) == inf and f(inf, -2.0) == 0.0 and f(3.0, 0.0) == 1.0
    # inf before the exp2 fix.  y * log2 x = 127.8 carries log2's 3 ulp and half an ulp of the product, ulp(127.8) = 2^-17: 3.5 * 2^-17 * ln 2 = 1.9e-5
    assert abs(float(f(3e38, 1.0)) / 3e38 - 1) < 1.9e-5


def _old_exp2_bits(xb):
    """pt_exp2 as it was before its scaling was clamped at the top: a literal restatement in numpy float32 (one rounding per
    operation, no contraction), the frozen copy the fixed function is compared with."""
    F = np.float32
    x = mc.floats(xb)
    with np.errstate(all="ignore"):
        fi = np.floor(x)
        xc = np.where(np.isnan(x) | (x >= 128) | (x < -150), F(0), x)               # the early returns are put back below
        fi = np.floor(xc)
        f = xc - fi
        i = fi.astype(np.int32)
        step = f > F(0.5)
        i = np.where(step, i + 1, i)
        f = np.where(step, f - F(1), f).astype(F)
        p = F(1.535336188319500e-4)
        for c in (1.339887440266574e-3, 9.618437357674640e-3, 5.550332471162809e-2, 2.402264791363012e-1, 6.931472028550421e-1, 1.0):
            p = (p * f + F(c)).astype(F)
        i1 = np.where(i < -126, -126, i).astype(np.int32)                            # the old scaling: no clamp at the top
        i2 = i - i1
        s1 = ((i1 + 127).astype(np.uint32) << 23).view(F)
        r = (p * s1).astype(F)
        r = np.where(i2 != 0, r * ((i2 + 127).astype(np.uint32) << 23).view(F), r).astype(F)
    out = r.view(np.uint32).copy()
    out[x >= 128] = 0x7F800000
    out[x < -150] = 0
    out[np.isnan(x)] = xb[np.isnan(x)]
    return out


def test_exp2_is_finite_and_monotone_up_to_128_and_unchanged_below(evaluate):
    """pt_exp2 scaled p by 2^i in one step for i > -126, and i = 128 (x in (127.5, 128): f > 0.5 rounds i up) made that scale
    asfloat(255 << 23) = inf.  Every float of [127, 128) must give a finite result within the 3-ulp bound, the function must not
    decrease over a sorted sample of [-151, 128), and the fix (i1 clamped to [-126, 127], the rest in a second exact step) must leave
    every result outside (127.5, 128) as the old scaling had it."""
    top = mc.exp2_top()
    got = evaluate(FN["exp2"], top)
    assert np.isfinite(mc.floats(got)).all(), f"{(~np.isfinite(mc.floats(got))).sum()} of {top.size} results in [127, 128) are not finite"
    err = mc.ulp_err(got, np.exp2(mc.floats(top).astype(np.float64))).max()
    print(f"exp2 on [127, 128): worst error {err:.4g} ulp")
    assert err <= mc.ULP_BOUND["exp2"]
    s = np.sort(np.concatenate([mc.floats(mc.domain("exp2")), mc.floats(top), mc.floats(mc.neighbourhood(127.5)), np.float32([-151, -150, -149, -126, 0])]))
    s = s[(s >= -151) & (s < 128)]
    r = mc.floats(evaluate(FN["exp2"], mc.bits(s)))
    assert (np.diff(r) >= 0).all(), "exp2 decreases at x = " + str(s[:-1][np.diff(r) < 0][:10])
    x = mc.cases("exp2")[0]
    f = mc.floats(x)
    outside = ~((f > 127.5) & (f < 128))
    old = _old_exp2_bits(x)
    assert (mc.floats(old[~outside]) == np.inf).all()                               # the restatement has the defect, so it is the old function
    mc.assert_same_bits("exp2", x[outside], np.zeros_like(x[outside]), evaluate(FN["exp2"], x)[outside], old[outside], "new", "old")


def _f2u(v):
    return 0 if v != v or v <= 0 else min(int(v) if abs(v) != float("inf") else 1 << 64, 0xFFFFFFFF)


def _f2i(v):
    return 0 if v != v else max(-(1 << 31), min(int(v) if abs(v) != float("inf") else (1 << 64 if v > 0 else -(1 << 64)), (1 << 31) - 1))


def test_conversions_truncate_saturate_and_send_nan_to_zero(evaluate):
    """pt_f2u / pt_f2i: D3D / WebGPU semantics, against a plain restatement of "truncate, saturate, NaN -> 0"."""
    named = np.array([np.nan, np.inf, -np.inf, -0.0, -0.5, 0.5, 1.5, -1.5, 2.0 ** 31 - 128, 2.0 ** 31, -2.0 ** 31, -2.0 ** 31 - 256,
                      2.0 ** 32 - 256, 2.0 ** 32, 2.0 ** 63, -2.0 ** 63, 3e38, -3e38], dtype=np.float32)
    x = np.concatenate([mc.bits(named), mc.specials(), mc.exponent_grid(), mc.branch(), mc.random_bits()[:4096]])
    u, i = evaluate(FN["f2u"], x), evaluate(FN["f2i"], x)
    f = mc.floats(x)
    want_u = np.array([_f2u(float(v)) for v in f], dtype=np.uint64).astype(np.uint32)
    want_i = np.array([_f2i(float(v)) for v in f], dtype=np.int64).astype(np.int32).view(np.uint32)
    assert u[0] == 0 and u[1] == 0xFFFFFFFF and u[2] == 0 and u[12] == 0xFFFFFF00 and u[13] == 0xFFFFFFFF
    assert i[0] == 0 and i[1] == 0x7FFFFFFF and i[2] == 0x80000000 and i[8] == 0x7FFFFF80 and i[9] == 0x7FFFFFFF and i[11] == 0x80000000
    mc.assert_same_bits("f2u", x, np.zeros_like(x), u, want_u)
    mc.assert_same_bits("f2i", x, np.zeros_like(x), i, want_i)


def test_roundings_and_rsqrt(evaluate):
    """pt_rint on ties (to even, the zero results keeping the argument's sign); pt_floor / pt_ceil / pt_trunc / pt_rint against numpy
    and pt_rsqrt against float32(1 / float32(sqrt(x))) over the whole core set."""
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 2.0 ** 23 - 0.5, 2.0 ** 23 + 0.5, -(2.0 ** 23 - 0.5)], dtype=np.float32)
    want = np.array([0.0, -0.0, 2.0, -2.0, 2.0, -2.0, 2.0 ** 23, 2.0 ** 23, -(2.0 ** 23)], dtype=np.float32)
    assert np.array_equal(evaluate(FN["rint"], mc.bits(ties)), mc.bits(want))
    x = np.concatenate([mc.core(), mc.branch()])
    f, zero = mc.floats(x), np.zeros_like(x)
    with np.errstate(all="ignore"):
        for name, ref in (("floor", np.floor(f)), ("ceil", np.ceil(f)), ("trunc", np.trunc(f)), ("rint", np.rint(f)),
                          ("rsqrt", np.float32(1.0) / np.sqrt(f)), ("sqrt", np.sqrt(f)), ("rcp", np.float32(1.0) / f)):
            assert ref.dtype == np.float32
            mc.assert_same_bits(name, x, zero, evaluate(FN[name], x), mc.bits(ref), "oracle", "numpy")


def _min_max_rule(x, y, is_max):
    """IEEE minNum / maxNum as the device computes them: a NaN operand is ignored (NaN only when both are), and -0 orders below +0."""
    a, b = mc.floats(x), mc.floats(y)
    with np.errstate(all="ignore"):
        pick_a = np.isnan(b) | ((a > b) if is_max else (a < b))
        r = np.where(pick_a, x, y)
        both_zero = (a == 0) & (b == 0)
        return np.where(both_zero, (x & y) if is_max else (x | y), r).astype(np.uint32)


def test_min_max_clamp_saturate_lerp(evaluate):
    """min / max ignore a NaN operand and order -0 below +0, whichever operand comes first (the rule the device's instructions follow,
    tests/test_gpu_math.py); clamp and saturate are built from them; lerp(0, x, y) = 0 + y * (x - 0)."""
    x, y = mc.cases("min")
    z = mc.bits(np.zeros(x.size, np.float32))
    mn, mx = evaluate(FN["min"], x, y), evaluate(FN["max"], x, y)
    mc.assert_same_bits("min", x, y, mn, _min_max_rule(x, y, False))
    mc.assert_same_bits("max", x, y, mx, _min_max_rule(x, y, True))
    pz, nz = mc.bits([0.0]), mc.bits([-0.0])
    assert evaluate(FN["max"], pz, nz)[0] == pz[0] and evaluate(FN["max"], nz, pz)[0] == pz[0]
    assert evaluate(FN["min"], pz, nz)[0] == nz[0] and evaluate(FN["min"], nz, pz)[0] == nz[0]
    mc.assert_same_bits("clamp0", x, y, evaluate(FN["clamp0"], x, y), _min_max_rule(_min_max_rule(x, z, True), y, False))
    one = mc.bits(np.ones(x.size, np.float32))
    mc.assert_same_bits("saturate", x, z, evaluate(FN["saturate"], x), _min_max_rule(_min_max_rule(x, z, True), one, False))
    with np.errstate(all="ignore"):
        lerp = np.float32(0) + mc.floats(y) * (mc.floats(x) - np.float32(0))
    mc.assert_same_bits("lerp0", x, y, evaluate(FN["lerp0"], x, y), mc.bits(lerp))


def test_atan_fmod_asin_special_cases_and_the_grids(evaluate):
    """atan2 over N(0,1)^2 within the existing bound; fmod against C's fmod where x / y is exact enough to be the same function
    (y = 1); asin / acos / atan at their edges."""
    x, y = mc.binary_extra("atan2")
    got = mc.floats(evaluate(FN["atan2"], x, y))
    assert np.abs(got - np.arctan2(mc.floats(x).astype(np.float64), mc.floats(y).astype(np.float64))).max() < 4e-7
    x, y = mc.binary_extra("fmod")
    n = mc.DOMAIN_N
    assert np.array_equal(evaluate(FN["fmod"], x[:n], y[:n]), mc.bits(np.fmod(mc.floats(x[:n]), np.float32(1.0))))
    assert mc.is_nan_bits(evaluate(FN["fmod"], x[2 * n:], y[2 * n:])[~mc.is_nan_bits(x[2 * n:]) & (np.abs(mc.floats(x[2 * n:])) < np.inf)
                                                                     & (np.abs(mc.floats(y[2 * n:])) == 0)]).all()        # x / 0 -> inf or NaN
    f = lambda name, v: mc.floats(evaluate(FN[name], mc.bits([v])))[0]
    assert f("asin", 1.0) == np.float32(np.pi / 2) and f("asin", -1.0) == np.float32(-np.pi / 2) and np.isnan(f("asin", 1.0000001))
    assert f("acos", -1.0) == np.float32(np.pi) and f("acos", 1.0) == 0.0 and np.isnan(f("asin", np.nan)) and np.isnan(f("acos", -1.0000001))
    assert f("atan", np.inf) == np.float32(np.pi / 2) and f("atan", -np.inf) == np.float32(-np.pi / 2) and f("atan", 0.0) == 0.0


def test_sincos_reduction_and_rng_batches(evaluate, lib):
    """The reduction's quadrant is rint(x * 2/pi) mod 4 and its argument stays within pi/4 (+ the rounding of k) over the documented
    reach; the batch RNG entries reproduce the known answers and chain (state out of rng_next == state behind random_float)."""
    x = mc.domain("sin")
    f = mc.floats(x)
    k = np.rint(f * np.float32(0.636619772367581343))
    assert np.array_equal(evaluate(FN["reduce_quadrant"], x), (k.astype(np.int64) & 3).astype(np.uint32))
    assert np.abs(mc.floats(evaluate(FN["reduce_arg"], x))).max() <= np.pi / 4 + 1e-3
    s = mc.rng_states()
    for step in range(4):
        nxt = evaluate(FN["rng_next"], s)
        r = evaluate(FN["random_float"], s)
        assert np.array_equal(r, mc.bits(nxt.astype(np.float32) / np.float32(4294967296.0)))
        for j, seed in enumerate(mc.KNOWN_SEEDS):
            assert nxt[j] == KNOWN[seed][step][0] and mc.floats(r)[j] == np.float32(KNOWN[seed][step][1])
        s = nxt
    c = C.c_uint32(int(mc.rng_states()[100]))
    for _ in range(4):
        lib.oracle_random_float(C.byref(c))
    assert c.value == s[100]


def test_wrap01_closed_form_on_the_core_set(evaluate):
    """pt_wrap01 against the literal loops on every element the loops can afford (tests/math_cases.py wrap_loop_inputs)."""
    x = mc.cases("wrap01_loops")[0]
    mc.assert_same_bits("wrap01", x, np.zeros_like(x), evaluate(FN["wrap01"], x), evaluate(FN["wrap01_loops"], x), "closed form", "loops")


def test_functions_are_compiler_independent(evaluate):
    """tests/test_oracle.py::test_oracle_is_compiler_independent, extended from frames to the functions themselves: the oracle built by
    clang at -O1 without -mfma (make -C oracle clang) gives the bits of the g++ build for every function number on every input set
    (a NaN result compared as NaN)."""
    from oracle import pyoracle
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clang = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(clang) and shutil.which("clang++") is None:
        pytest.skip("no clang++")
    subprocess.check_call(["make", "-C", os.path.join(root, "oracle"), "clang"] + ([] if os.path.exists(clang) else ["CLANGXX=clang++"]),
                          stdout=subprocess.DEVNULL)
    other = C.CDLL(os.path.join(root, "oracle", "_build", "liboracle_clang.so"))
    assert set(FN.values()) == set(range(len(FN)))
    for name, fn in FN.items():
        x, y = mc.cases(name)
        mc.assert_same_bits(name, x, y, pyoracle.math_n(fn, x, y, lib=other), evaluate(fn, x, y), "clang", "g++")
