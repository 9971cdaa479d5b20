"""The input sets of the tests that pin include/ptmi_math.h function by function: tests/test_math.py (the oracle's evaluation, on the
CPU) and tests/test_gpu_math.py (the same switch inside a kernel, against the oracle).  Everything is deterministic (fixed seeds) and
built from bit patterns, so signalling NaNs, payloads and subnormals arrive as written.

FN names the function numbers of include/ptmi_math_switch.h.  cases(fn) is everything that function is evaluated on: (xbits, ybits),
uint32 arrays of one length.  The float functions take a float's bits; unorm8 and the RNG take the integer itself."""
import functools

import numpy as np

U32, F32, F64 = np.uint32, np.float32, np.float64

FN = dict(sin=0, cos=1, log=2, log2=3, exp2=4, pow=5, acos=6, asin=7, sqrt=8, rcp=9, atan2=10, fmod=11, wrap01=12, wrap01_loops=13,
          unorm8=14, unorm8_div=15, atan=16, rsqrt=17, floor=18, ceil=19, rint=20, trunc=21, min=22, max=23, clamp0=24, saturate=25,
          lerp0=26, f2u=27, f2i=28, rng_next=29, random_float=30, reduce_arg=31, reduce_quadrant=32)
NAME = {v: k for k, v in FN.items()}
BINARY = ("pow", "atan2", "fmod", "min", "max", "clamp0", "lerp0")       # clamp0 = clamp(x, 0, y), lerp0 = lerp(0, x, y)
INTEGER_IN = ("unorm8", "unorm8_div", "rng_next", "random_float")

SIGN = U32(0x80000000)
QNAN, QNAN_PAYLOAD, SNAN = 0x7FC00000, 0x7FC12345, 0x7F800001
KNOWN_SEEDS = (0x00000000, 0x00000001, 0x12345678, 0xFFFFFFFF)           # tests/test_math.py KNOWN


def bits(f):
    return np.ascontiguousarray(f, dtype=F32).view(U32)


def floats(b):
    return np.ascontiguousarray(b, dtype=U32).view(F32)


def both_signs(b):
    b = np.asarray(b, dtype=U32)
    return np.concatenate([b & ~SIGN, b | SIGN])


# ---- unary core set ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def specials():
    """0, smallest / largest subnormal, smallest normal, 1, FLT_MAX, inf, quiet NaN, quiet NaN with a payload, signalling NaN: both signs."""
    return both_signs([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000, QNAN, QNAN_PAYLOAD, SNAN])


@functools.lru_cache(None)
def exponent_grid():
    """Every exponent 0...255 x 16 mantissas (0, 1, 0x400000, 0x7FFFFF, 12 fixed random ones) x both signs."""
    m = np.concatenate([[0, 1, 0x400000, 0x7FFFFF], np.random.RandomState(7).randint(0, 1 << 23, 12)]).astype(U32)
    e = np.arange(256, dtype=U32) << 23
    return both_signs((e[:, None] | m[None, :]).ravel())


@functools.lru_cache(None)
def random_bits(n=1 << 20, seed=11):
    return np.random.RandomState(seed).randint(0, 1 << 32, n, dtype=np.uint64).astype(U32)


@functools.lru_cache(None)
def core():
    return np.concatenate([specials(), exponent_grid(), random_bits()])


# ---- branch neighbourhoods -----------------------------------------------------------------------------------------------------
def neighbourhood(c, half=8):
    """The 2*half+1 consecutive floats centred on fl(c), with both signs."""
    b = int(bits([abs(c)])[0])
    return both_signs(np.arange(b - half, b + half + 1, dtype=np.int64).clip(0, 0x7F800000).astype(U32))


BRANCH_CONSTANTS = (0.5, 1.0, 0.707106781186547524, 0.4142135623730950, 2.414213562373095,      # asin/acos, log_split, atan
                    150.0, 126.0, 125.5, 127.0, 127.5, 128.0,                                   # exp2 (the negative ones by sign)
                    2.0 ** 24, 2.0 ** 31, 2.0 ** 32, 2.0 ** 63,                                 # wrap01, f2i, f2u, beyond every integer
                    0.0031308)                                                                  # the sRGB knee of the present blit


@functools.lru_cache(None)
def branch():
    sets = [neighbourhood(c) for c in BRANCH_CONSTANTS]
    sets += [neighbourhood(k * np.pi / 4) for k in range(65)]                                   # octant borders of the reduction
    sets += [neighbourhood(k * np.pi / 2, 32) for k in (8191.5, 8192.0, 8192.5)]                # rint(x * 2/pi) crosses 2^13
    return np.concatenate(sets)


# ---- per-function domain sets (the accuracy checks run on these) ---------------------------------------------------------------
DOMAIN_N = 1 << 18


@functools.lru_cache(None)
def domain(name):
    """uint32 bits of the 2^18-sample domain set(s) of `name`; None when the function has none."""
    r = np.random.RandomState(1000 + FN[name])
    if name in ("sin", "cos", "reduce_arg", "reduce_quadrant"):
        r = np.random.RandomState(1000)                                   # one set for the four of them
        return bits(np.concatenate([r.uniform(0.0, 2 * np.pi, DOMAIN_N), r.uniform(-1.2e4, 1.2e4, DOMAIN_N)]))
    if name in ("log", "log2"):
        r = np.random.RandomState(1002)
        normal = (r.randint(1, 255, DOMAIN_N).astype(U32) << 23) | r.randint(0, 1 << 23, DOMAIN_N).astype(U32)
        return np.concatenate([normal, r.randint(1, 1 << 23, 1 << 16).astype(U32)])             # ... and 2^16 subnormals
    if name == "exp2":
        return bits(np.minimum(r.uniform(-151.0, 128.0, DOMAIN_N).astype(F32), np.nextafter(F32(128), F32(0))))
    if name in ("asin", "acos"):
        r = np.random.RandomState(1006)
        return bits(r.uniform(-1.0, 1.0, DOMAIN_N))
    if name == "atan":                                                    # all three ranges of the reduction: 2^-30 ... 2^30, both signs
        return bits(np.exp2(r.uniform(-30.0, 30.0, DOMAIN_N)) * r.choice([-1.0, 1.0], DOMAIN_N))
    return None


@functools.lru_cache(None)
def exp2_top():
    """Every float of [127, 128)."""
    return np.arange(int(bits([127.0])[0]), int(bits([128.0])[0]), dtype=U32)


# ---- binary sets ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def grid():
    s = specials()
    return np.repeat(s, s.size), np.tile(s, s.size)


@functools.lru_cache(None)
def random_pairs():
    return random_bits(DOMAIN_N, 21), random_bits(DOMAIN_N, 22)


def _positive_all_exponents(r, n):
    return (r.randint(0, 255, n).astype(U32) << 23) | r.randint(0, 1 << 23, n).astype(U32)      # subnormals included, no inf / NaN


@functools.lru_cache(None)
def binary_extra(name):
    r = np.random.RandomState(2000 + FN[name])
    n = DOMAIN_N
    if name == "pow":
        x, y = [_positive_all_exponents(r, n)], [bits(r.uniform(-40.0, 40.0, n))]
        inf, one, zero = F32(np.inf), F32(1), F32(0)
        ys = np.array([-inf, -40.0, -2.0, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0, 2.2, 40.0, inf], dtype=F32)
        xs = np.array([0.0, -0.0, 1e-40, 0.25, 1.0, 2.0, 3e38, inf, -1e-40, -0.25, -1.0, -2.0, -inf], dtype=F32)
        # (0, 0), (0, y>0), (0, y<0), (x<0, y), (1, +-inf), (inf, y), (x, 0): the grid xs x ys holds them all
        x.append(bits(np.repeat(xs, ys.size)))
        y.append(bits(np.tile(ys, xs.size)))
        return np.concatenate(x), np.concatenate(y)
    if name == "atan2":
        return bits(r.normal(0, 1, n)), bits(r.normal(0, 1, n))
    if name == "fmod":
        a = bits(r.uniform(-3.0, 3.0, n))                                 # y = 1
        b = bits(r.normal(0, 100.0, n))                                   # random y
        c = np.concatenate([specials(), bits(r.normal(0, 100.0, 108))])   # y in {0, inf, NaN}
        ysp = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, QNAN, SNAN], dtype=U32)
        return (np.concatenate([a, b, np.repeat(c, ysp.size)]),
                np.concatenate([np.full(n, bits([1.0])[0], dtype=U32), bits(r.normal(0, 1.0, n)), np.tile(ysp, c.size)]))
    return np.zeros(0, U32), np.zeros(0, U32)


# ---- other sets ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def unorm8_inputs():
    """All 256 bytes, and the same bytes with random high bits set (pt_unorm8 masks with 0xFF)."""
    b = np.arange(256, dtype=U32)
    hi = np.random.RandomState(14).randint(1, 1 << 24, 256).astype(U32) << 8
    return np.concatenate([b, b | hi])


@functools.lru_cache(None)
def rng_states():
    return np.concatenate([np.array(KNOWN_SEEDS, dtype=U32), random_bits(1 << 16, 29)])


@functools.lru_cache(None)
def wrap_loop_inputs():
    """The literal loops of util/texture.hlsl (fn 13) take |u| iterations, so they run on the elements of core() and branch() with
    |u| < 2^12 or |u| >= 2^24 (where the guard answers) or NaN, and on the large values of tests/test_math.py's own list; the closed
    form (fn 12) runs on everything."""
    b = np.concatenate([core(), branch()])
    a = np.abs(floats(b))
    keep = ~((a >= 4096.0) & (a < 16777216.0))
    return np.concatenate([b[keep], bits([16777215.0, -16777215.0, 2e5, -2e5, 65536.5, -65536.5])])


@functools.lru_cache(None)
def cases(name):
    """(xbits, ybits): every element function `name` is evaluated on."""
    if name in BINARY:
        parts = [grid(), random_pairs(), binary_extra(name)]
        x, y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    else:
        if name == "wrap01_loops":
            x = wrap_loop_inputs()
        elif name in ("unorm8", "unorm8_div"):
            x = np.concatenate([unorm8_inputs(), random_bits(1 << 16, 15)])
        elif name in ("rng_next", "random_float"):
            x = rng_states()
        else:
            x = np.concatenate([core(), branch()] + ([domain(name)] if domain(name) is not None else [])
                               + ([exp2_top()] if name == "exp2" else []))
        y = np.zeros_like(x)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


# ---- measures and comparisons ----------------------------------------------------------------------------------------------------
def ulp_err(got_bits, ref64):
    """|got - ref| in ulps of the float32 rounding of ref, the ulp floored at 2^-149 (subnormal results count)."""
    with np.errstate(all="ignore"):
        ref32 = ref64.astype(F32)
        ulp = np.maximum(np.spacing(np.abs(ref32)).astype(F64), 2.0 ** -149)
        return np.abs(floats(got_bits).astype(F64) - ref64) / ulp


def is_nan_bits(b):
    return (b & U32(0x7FFFFFFF)) > U32(0x7F800000)


def mismatches(got, want):
    """Indices where the bits differ; a NaN in `want` is matched by any NaN (sign and payload of a NaN are not part of the contract)."""
    got, want = np.asarray(got, dtype=U32), np.asarray(want, dtype=U32)
    return np.flatnonzero((got != want) & ~(is_nan_bits(want) & is_nan_bits(got)))


def assert_same_bits(name, x, y, got, want, got_label="got", want_label="want"):
    bad = mismatches(got, want)
    if bad.size:
        lines = [f"{name}: {bad.size} of {len(want)} elements differ"]
        for i in bad[:10]:
            lines.append(f"  {name}(x=0x{int(x[i]):08X}, y=0x{int(y[i]):08X}): {want_label} 0x{int(want[i]):08X}  {got_label} 0x{int(got[i]):08X}")
        raise AssertionError("\n".join(lines))


# ---- float64 references and the project's bounds ---------------------------------------------------------------------------------
REFERENCE = dict(sin=np.sin, cos=np.cos, log=np.log, log2=np.log2, exp2=np.exp2, acos=np.arccos, asin=np.arcsin, atan=np.arctan)
ULP_BOUND = dict(log=2.0, log2=3.0, exp2=3.0, acos=3.0, asin=4.0, atan=4.0)
SINCOS_ABS_BOUND = 1.5e-7                                                 # over [0, 2 pi] and +-1.2e4


def accuracy(name, evaluate):
    """The worst error of `name` over its domain set(s), `evaluate(fn, xbits) -> result bits`: ulps (log, log2, exp2, acos, asin,
    atan) or absolute (sin, cos)."""
    x = domain(name)
    got = evaluate(FN[name], x)
    with np.errstate(all="ignore"):
        ref = REFERENCE[name](floats(x).astype(F64))
    if name in ("sin", "cos"):
        return float(np.abs(floats(got).astype(F64) - ref).max())
    return float(ulp_err(got, ref).max())


def check_accuracy(evaluate, report=print):
    for name in ("log", "log2", "exp2", "acos", "asin", "atan", "sin", "cos"):
        err = accuracy(name, evaluate)
        bound = SINCOS_ABS_BOUND if name in ("sin", "cos") else ULP_BOUND[name]
        report(f"{name}: worst error {err:.4g} {'absolute' if name in ('sin', 'cos') else 'ulp'} (bound {bound:g})")
        assert err <= bound, (name, err, bound)
