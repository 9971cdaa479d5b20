"""A numpy restatement of the integer side of HAS_ENVIRONMENT_TEXTURE (util/sky.hlsl:7-42, PathTracer.cs:297-306): the CDF, the two
binary searches and the texel addressing of the bilinear fetch.  It shares no code with the oracle or the kernels; tests/test_env.py
holds the oracle to it bit for bit, tests/test_gpu_env.py holds the device to the oracle.

The float32 arithmetic here is numpy's, one IEEE operation per line where the order matters."""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64


def cdf(texels):
    """cdf[i] = the float32 running sum of texel i's grey value, texels in memory order (row 0 first, column 0 first in a row):
    sum += (0.299 r + 0.587 g) + 0.114 b, one addition per texel."""
    t = np.ascontiguousarray(texels, dtype=F32).reshape(-1, 4)
    out = np.empty(len(t), dtype=F32)
    s = F32(0.0)
    with np.errstate(all="ignore"):
        for i in range(len(t)):
            grey = (F32(0.299) * t[i, 0] + F32(0.587) * t[i, 1]) + F32(0.114) * t[i, 2]
            s = F32(s + grey)
            out[i] = s
    return out


def binary_search_cell(c, w, h, values):
    """(x, y) of util/sky.hlsl:7-42 for every value: the two loops as written, all values stepped together.  A comparison with a
    NaN is false, as in the shader."""
    c = np.asarray(c, dtype=F32)
    values = np.asarray(values, dtype=F32)

    def search(upper0, index):
        lower = np.zeros(len(values), dtype=I64)
        upper = np.full(len(values), upper0, dtype=I64)
        while True:
            live = lower < upper
            if not live.any():
                return lower
            mid = (lower + upper) >> 1
            with np.errstate(invalid="ignore"):
                less = values < c[np.where(live, index(mid), 0)]
            upper = np.where(live & less, mid, upper)
            lower = np.where(live & ~less, mid + 1, lower)
    y = np.clip(search(h - 1, lambda mid: mid * w + w - 1), 0, h - 1)
    x = np.clip(search(w - 1, lambda mid: y * w + mid), 0, w - 1)
    return x, y


def binary_search(c, w, h, values):
    """(u, v) = (x / W, y / H) in float32, (n, 2)"""
    x, y = binary_search_cell(c, w, h, values)
    return np.stack([x.astype(F32) / F32(w), y.astype(F32) / F32(h)], axis=1)


def _f2i(x):
    """float -> int32 as pt_f2i: NaN -> 0, saturating"""
    with np.errstate(invalid="ignore"):
        x = np.where(np.isnan(x), F32(0), x)
        return np.clip(x.astype(F64), -2147483648.0, 2147483647.0).astype(I64)


def taps(w, h, uv):
    """The addressing of SampleLevel restated: (x0, x1, y0, y1, ax, ay) for uv pairs (n, 2).  Texel centres at (i + 0.5) / size, memory
    row r at v = 1 - (r + 0.5) / H, clamp addressing; ax, ay are the float32 weights of the x1 column and the y1 row."""
    uv = np.asarray(uv, dtype=F32)
    with np.errstate(all="ignore"):
        fx = uv[:, 0] * F32(w) - F32(0.5)
        fy = (F32(1.0) - uv[:, 1]) * F32(h) - F32(0.5)
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
    x0, y0 = _f2i(x0f), _f2i(y0f)
    x1 = np.where(x0 < 2147483647, x0 + 1, x0)
    y1 = np.where(y0 < 2147483647, y0 + 1, y0)
    cx, cy = (lambda v: np.clip(v, 0, w - 1)), (lambda v: np.clip(v, 0, h - 1))
    return cx(x0), cx(x1), cy(y0), cy(y1), ax.astype(F32), ay.astype(F32)


def bilinear64(texels, uv):
    """(blend (n, 3) float64, largest |tap| (n, 3) float64): the four taps of taps() blended in float64 with the float32 weights,
    columns first, in the lerp's own form a + t (b - a), so that an inf or NaN tap or weight spreads exactly as it does in float32."""
    t = np.asarray(texels, dtype=F32)
    h, w = t.shape[:2]
    x0, x1, y0, y1, ax, ay = taps(w, h, uv)
    a, b, c, d = (t[yy, xx, :3].astype(F64) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    ax, ay = ax.astype(F64)[:, None], ay.astype(F64)[:, None]
    with np.errstate(all="ignore"):
        top, bot = a + ax * (b - a), c + ax * (d - c)
        return top + ay * (bot - top), np.max(np.abs(np.stack([a, b, c, d])), axis=0)


def rng_next(state):
    """pt_rng_next over uint32 arrays"""
    s = np.asarray(state, dtype=np.uint64)
    old = (s + 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((old >> ((old >> 28) + 4)) ^ old) * 277803737) & 0xFFFFFFFF
    return ((word >> 22) ^ word).astype(np.uint32)


def random_float(state):
    return rng_next(state).astype(F32) / F32(4294967296.0)


def lattice_direction(w, h, x, y, rotation):
    """The direction sample_env_map returns for texel (x, y), in float64: u = x / W - rotation, v' = 1 - y / H, phi = 2 pi u,
    theta = pi v' (util/sky.hlsl:71-86)."""
    phi, theta = (x / w - rotation) * 2.0 * np.pi, (1.0 - y / h) * np.pi
    return np.array([-np.sin(theta) * np.cos(phi), np.cos(theta), -np.sin(theta) * np.sin(phi)])
