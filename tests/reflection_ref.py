"""The reflection-probe rule (include/ptmi_plugin.h Part 20) restated in numpy float32, for tests/test_reflection.py and
tests/test_gpu_reflection.py: texel directions, the capture's seeding and fold, the GGX prefilter and the lookup with its wrap and
box projection.  Written from the header's text, not from reflection_rule.h; every operation is one float32 operation in the
rule's order.  The RNG step is gather_ref's."""
import numpy as np

from gather_ref import F, M32, luminance, rng_next

ONE, TWO, HALF = F(1.0), F(2.0), F(0.5)


def texel_count(res, levels=1):
    return sum((res >> k) ** 2 for k in range(levels))


def sgn(x):
    return np.where(x < 0, F(-1.0), F(1.0)).astype(F)


def direction(R, u, v, su, sv):
    """direction(R, u, v, su, sv) of arrays (or scalars) -> d (..., 3) float32, len (...,) float32"""
    u, v = np.asarray(u).astype(F), np.asarray(v).astype(F)
    a = ((u + F(su)) / F(R)) * TWO - ONE if np.isscalar(su) else ((u + su.astype(F)) / F(R)) * TWO - ONE
    b = ((v + F(sv)) / F(R)) * TWO - ONE if np.isscalar(sv) else ((v + sv.astype(F)) / F(R)) * TWO - ONE
    z = (ONE - np.abs(a)) - np.abs(b)
    x = np.where(z < 0, (ONE - np.abs(b)) * sgn(a), a).astype(F)
    y = np.where(z < 0, (ONE - np.abs(a)) * sgn(b), b).astype(F)
    ln = np.sqrt((x * x + y * y) + z * z).astype(F)
    return np.stack([x / ln, y / ln, z / ln], axis=-1).astype(F), ln


def centres(R):
    """the centre directions of an R x R map in texel order v * R + u, and their len"""
    t = np.arange(R * R)
    return direction(R, t % R, t // R, 0.5, 0.5)


def oct_coords(D):
    D = np.asarray(D, F)
    s = (np.abs(D[..., 0]) + np.abs(D[..., 1])) + np.abs(D[..., 2])
    a, b = D[..., 0] / s, D[..., 1] / s
    a2 = (ONE - np.abs(b)) * sgn(a)
    b2 = (ONE - np.abs(a)) * sgn(b)
    neg = D[..., 2] < 0
    return np.where(neg, a2, a).astype(F), np.where(neg, b2, b).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------------------------------------------
def random_float(s):
    s = rng_next(s)
    return s, F(np.uint32(s)) / F(4294967296.0)


def rays(positions, seeds, R, first_sample, samples):
    """PTReflectionRays' rows: (n * R * R * samples, 8) float32, slot-major"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    n = pos.shape[0]
    out = np.zeros((n * R * R * samples, 8), F)
    r1, r2 = np.empty(len(out), F), np.empty(len(out), F)
    state = np.empty(len(out), np.uint32)
    k = 0
    for i in range(n):
        for t in range(R * R):
            s0 = (rng_next(int(seeds[i]) & M32) + t) & M32
            s0 = rng_next(s0)
            for j in range(samples):
                s = (s0 + first_sample + j) & M32
                s, r1[k] = random_float(s)
                s, r2[k] = random_float(s)
                state[k] = s
                k += 1
    t = np.tile(np.repeat(np.arange(R * R), samples), n)
    d, _ = direction(R, t % R, t // R, r1, r2)
    out[:, 0:3] = np.repeat(pos, R * R * samples, axis=0)
    out[:, 3:6] = d
    out[:, 6] = state.view(F)
    return out


def fold(radiance, samples):
    """radiance (texels * samples, >= 3) -> (texels, 4): ascending j from +0.0f, rgb / (float)samples, aux = the sum of lum^2"""
    L = np.asarray(radiance, F)[:, :3].reshape(-1, samples, 3)
    acc = np.zeros((L.shape[0], 3), F)
    m2 = np.zeros(L.shape[0], F)
    for j in range(samples):
        acc = acc + L[:, j]
        lum = luminance(L[:, j])
        m2 = m2 + lum * lum
    return np.concatenate([acc / F(samples), m2[:, None]], axis=1).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# prefilter
# ---------------------------------------------------------------------------------------------------------------------------
def lobe_g(k, levels):
    rho = F(k) / F(levels - 1)
    alpha = rho * rho
    a2 = alpha * alpha
    return F(a2 - ONE)


def weights(n, l, J, g):
    """the weight of every (output, source) pair it is called with, and whether the source counts"""
    c = (n[..., 0] * l[..., 0] + n[..., 1] * l[..., 1]) + n[..., 2] * l[..., 2]
    h = (ONE + c) * HALF
    t = h * g + ONE
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (c * J) / (t * t)
    return w.astype(F), c > 0


def prefilter(base, R, levels):
    """base (n, R * R, 4) -> (n, texel_count(R, levels), 4); one output texel sums the sources in ascending s"""
    base = np.asarray(base, F)
    n = base.shape[0]
    out = np.empty((n, texel_count(R, levels), 4), F)
    out[:, :R * R] = base
    l, ln = centres(R)
    J = (ONE / ((ln * ln) * ln)).astype(F)
    first = R * R
    for k in range(1, levels):
        Rk = R >> k
        nd, _ = centres(Rk)
        g = lobe_g(k, levels)
        acc = np.zeros((n, Rk * Rk, 3), F)
        sw = np.zeros(Rk * Rk, F)
        for s in range(R * R):
            w, on = weights(nd, l[s][None, :], J[s], g)
            acc = np.where(on[None, :, None], acc + w[None, :, None] * base[:, s, None, :3], acc).astype(F)
            sw = np.where(on, sw + w, sw).astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, first:first + Rk * Rk, :3] = acc / sw[None, :, None]
        out[:, first:first + Rk * Rk, 3] = sw[None, :]
        first += Rk * Rk
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# lookup
# ---------------------------------------------------------------------------------------------------------------------------
def box_project(bmin, bmax, P, Q, D):
    """vectorised over queries: (q, 3) each -> the direction read"""
    bmin, bmax, P, Q, D = (np.asarray(x, F) for x in (bmin, bmax, P, Q, D))
    inside = ((bmin <= P) & (P <= bmax)).all(axis=1)
    t = np.full(len(D), np.inf, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            ta = np.where(D[:, a] > 0, (bmax[:, a] - P[:, a]) / D[:, a], (bmin[:, a] - P[:, a]) / D[:, a]).astype(F)
            t = np.where(D[:, a] != 0, np.fmin(t, ta), t).astype(F)
        ok = inside & (t > 0) & np.isfinite(t)
        v = ((P + D * t[:, None]) - Q).astype(F)
        r = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F)
        ok &= r > 0
        proj = (v / r[:, None]).astype(F)
    return np.where(ok[:, None], proj, D).astype(F)


def select_levels(roughness, levels):
    r = np.asarray(roughness, F)
    r = np.where(r > 0, r, F(0.0)).astype(F)
    r = np.where(r < 1, r, F(1.0)).astype(F)
    lam = r * F(levels - 1)
    k0 = np.minimum(lam.astype(np.uint32), levels - 2).astype(np.int64)
    return k0, (lam - k0.astype(F)).astype(F)


def wrap(Rk, x, y):
    out = (x < 0) | (x >= Rk)
    x, y = np.where(out, np.where(x < 0, -1 - x, 2 * Rk - 1 - x), x), np.where(out, Rk - 1 - y, y)
    out = (y < 0) | (y >= Rk)
    y, x = np.where(out, np.where(y < 0, -1 - y, 2 * Rk - 1 - y), y), np.where(out, Rk - 1 - x, x)
    return x, y


def lerp(p, q, f):
    return (p + f * (q - p)).astype(F)


def bilinear(level, Rk, a, b):
    """level (q, Rk * Rk, 3): every query's own probe's level -> (q, 3)"""
    x = (a * HALF + HALF) * F(Rk) - HALF
    y = (b * HALF + HALF) * F(Rk) - HALF
    x0f, y0f = np.floor(x).astype(F), np.floor(y).astype(F)
    fx, fy = (x - x0f).astype(F)[:, None], (y - y0f).astype(F)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    rows = np.arange(len(a))
    tap = []
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = wrap(Rk, x0 + dx, y0 + dy)
            tap.append(level[rows, ty * Rk + tx])
    return lerp(lerp(tap[0], tap[1], fx), lerp(tap[2], tap[3], fx), fy)


def lookup(maps, R, levels, queries, probe_positions=None, boxes=None):
    """maps (n, texel_count, 4); queries (q, 8) PTReflectionQuery rows; boxes (n, 8) rows with probe_positions (n, 3) -> (q, 4)"""
    maps, qr = np.asarray(maps, F), np.asarray(queries, F)
    q = len(qr)
    probe = qr[:, 7].copy().view(np.uint32).astype(np.int64)
    live = probe < maps.shape[0]
    pi = np.where(live, probe, 0)
    D = qr[:, 4:7]
    if boxes is not None:
        bx = np.asarray(boxes, F)
        D = box_project(bx[pi, 0:3], bx[pi, 4:7], qr[:, 0:3], np.asarray(probe_positions, F)[pi], D)
    a, b = oct_coords(D)
    k0, f = select_levels(qr[:, 3], levels)
    out = np.zeros((q, 4), F)
    for k in range(levels - 1):
        sel = np.nonzero(live & (k0 == k))[0]
        if not len(sel):
            continue
        o0, o1, o2 = texel_count(R, k), texel_count(R, k + 1), texel_count(R, k + 2)
        A = bilinear(maps[pi[sel], o0:o1, :3], R >> k, a[sel], b[sel])
        B = bilinear(maps[pi[sel], o1:o2, :3], R >> (k + 1), a[sel], b[sel])
        out[sel, :3] = lerp(A, B, f[sel][:, None])
        out[sel, 3] = 1.0
    return out
