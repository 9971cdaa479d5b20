"""The rule of baked-light shading (include/ptmi_plugin.h Part 21; csrc/shade_rule.h) restated in numpy.

Every operation is a binary32 operation in the order the header writes it: the arrays are float32 throughout, and numpy's + - * /
and sqrt round each result once.  The DFG quadrature in float64 at the bottom is the same integral on a much finer grid, for the
error bound."""
import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
MISS = 1
INV_PI = F(0.31830988618379067)

# cos and sin of 2 pi (q + 0.5) / 64, rounded from float64: this module's own copy of the header's literals
C = np.array([
    0.99879545, 0.9891765, 0.97003126, 0.94154406, 0.9039893, 0.8577286, 0.8032075, 0.7409511,
    0.671559, 0.5956993, 0.51410276, 0.42755508, 0.33688986, 0.24298018, 0.14673047, 0.049067676,
    -0.049067676, -0.14673047, -0.24298018, -0.33688986, -0.42755508, -0.51410276, -0.5956993, -0.671559,
    -0.7409511, -0.8032075, -0.8577286, -0.9039893, -0.94154406, -0.97003126, -0.9891765, -0.99879545,
    -0.99879545, -0.9891765, -0.97003126, -0.94154406, -0.9039893, -0.8577286, -0.8032075, -0.7409511,
    -0.671559, -0.5956993, -0.51410276, -0.42755508, -0.33688986, -0.24298018, -0.14673047, -0.049067676,
    0.049067676, 0.14673047, 0.24298018, 0.33688986, 0.42755508, 0.51410276, 0.5956993, 0.671559,
    0.7409511, 0.8032075, 0.8577286, 0.9039893, 0.94154406, 0.97003126, 0.9891765, 0.99879545,
], dtype=np.float32)
S = np.array([
    0.049067676, 0.14673047, 0.24298018, 0.33688986, 0.42755508, 0.51410276, 0.5956993, 0.671559,
    0.7409511, 0.8032075, 0.8577286, 0.9039893, 0.94154406, 0.97003126, 0.9891765, 0.99879545,
    0.99879545, 0.9891765, 0.97003126, 0.94154406, 0.9039893, 0.8577286, 0.8032075, 0.7409511,
    0.671559, 0.5956993, 0.51410276, 0.42755508, 0.33688986, 0.24298018, 0.14673047, 0.049067676,
    -0.049067676, -0.14673047, -0.24298018, -0.33688986, -0.42755508, -0.51410276, -0.5956993, -0.671559,
    -0.7409511, -0.8032075, -0.8577286, -0.9039893, -0.94154406, -0.97003126, -0.9891765, -0.99879545,
    -0.99879545, -0.9891765, -0.97003126, -0.94154406, -0.9039893, -0.8577286, -0.8032075, -0.7409511,
    -0.671559, -0.5956993, -0.51410276, -0.42755508, -0.33688986, -0.24298018, -0.14673047, -0.049067676,
], dtype=np.float32)


def azimuth_float64():
    ang = 2.0 * np.pi * (np.arange(64, dtype=np.float64) + 0.5) / 64.0
    return np.cos(ang), np.sin(ang)


def smith_g(c, alpha):
    a = alpha * alpha
    b = c * c
    return (F(2) * c) / (c + np.sqrt((a + b) - a * b))


def fold(v):
    """sh_rule.h's tree over the last axis (64 lane partials)"""
    v = v.copy()
    h = 32
    while h >= 1:
        v[..., :h] = v[..., :h] + v[..., h:2 * h]
        h >>= 1
    return v[..., 0]


def dfg_entries(res, i, j, alpha_for_a2=False, without_g=False):
    """entries (i[k], j[k]) of the res x res table -> (k, 2) float32.  alpha_for_a2 / without_g: two WRONG rules (a2 = alpha; G = 1)
    that the error bound of the table must tell from the right one."""
    i = np.asarray(i, np.uint32).reshape(-1, 1)
    j = np.asarray(j, np.uint32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        mu = (i.astype(F) + F(0.5)) / F(res)
        rho = (j.astype(F) + F(0.5)) / F(res)
        alpha = rho * rho
        a2 = alpha if alpha_for_a2 else alpha * alpha
        Vx, Vz = np.sqrt(F(1) - mu * mu), mu
        gV = smith_g(mu, alpha)
        Cq = C.reshape(1, 64)
        a = np.zeros((i.shape[0], 64), F)
        b = np.zeros((i.shape[0], 64), F)
        for p in range(64):
            xi = (F(p) + F(0.5)) / F(64)
            c2 = (F(1) - xi) / (F(1) + (a2 - F(1)) * xi)
            Hx = np.sqrt(F(1) - c2) * Cq
            Hz = np.sqrt(c2)
            vh = Vx * Hx + Vz * Hz
            nl = (F(2) * vh) * Hz - Vz
            ok = (nl > 0) & (vh > 0)
            G = np.ones_like(vh) if without_g else gV * smith_g(nl, alpha)
            gv = (G * vh) / (Hz * mu)
            m = F(1) - vh
            m2 = m * m
            Fc = (m2 * m2) * m
            a = np.where(ok, a + (F(1) - Fc) * gv, a)
            b = np.where(ok, b + Fc * gv, b)
    return np.stack([fold(a) / F(4096), fold(b) / F(4096)], axis=-1).astype(F)


def dfg_table(res, **wrong):
    jj, ii = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    return dfg_entries(res, ii.ravel(), jj.ravel(), **wrong).reshape(res, res, 2)


def dfg_quadrature(res, radial=1024, azimuth=256):
    """the same integral in float64 with radial x azimuth midpoint samples -> (res, res, 2) float64"""
    out = np.zeros((res, res, 2))
    xi = ((np.arange(radial) + 0.5) / radial).reshape(-1, 1)
    ang = 2.0 * np.pi * (np.arange(azimuth) + 0.5) / azimuth
    cq = np.cos(ang).reshape(1, -1)

    def g1(c, alpha):
        a, b = alpha * alpha, c * c
        return 2.0 * c / (c + np.sqrt(a + b - a * b))

    for j in range(res):
        rho = (j + 0.5) / res
        alpha = rho * rho
        a2 = alpha * alpha
        c2 = (1.0 - xi) / (1.0 + (a2 - 1.0) * xi)
        st, Hz = np.sqrt(1.0 - c2), np.sqrt(c2)
        for i in range(res):
            mu = (i + 0.5) / res
            Vx = np.sqrt(1.0 - mu * mu)
            vh = Vx * (st * cq) + mu * Hz
            nl = 2.0 * vh * Hz - mu
            ok = (nl > 0) & (vh > 0)
            with np.errstate(all="ignore"):
                gv = g1(mu, alpha) * g1(np.where(ok, nl, 1.0), alpha) * vh / (Hz * mu)
            Fc = (1.0 - vh) ** 5
            out[j, i, 0] = np.where(ok, (1.0 - Fc) * gv, 0.0).sum() / (radial * azimuth)
            out[j, i, 1] = np.where(ok, Fc * gv, 0.0).sum() / (radial * azimuth)
    return out


# ---- terms ----
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def choose_probe(P, probes, boxes):
    """P (n, 3); probes (k, 3) or None; boxes (k, 8) rows or None -> (n,) uint32"""
    n = P.shape[0]
    best = np.full(n, NONE, np.uint32)
    bestD = np.zeros(n, F)
    k = 0 if probes is None else probes.shape[0]
    for pas in ((0, 1) if boxes is not None else (1,)):
        open_ = best == NONE                     # the second pass only runs where the first found nothing
        for q in range(k):
            cand = open_.copy()
            if pas == 0:
                lo, hi = boxes[q, 0:3], boxes[q, 4:7]
                cand &= np.all((lo <= P) & (P <= hi), axis=1)
            v = P - probes[q].reshape(1, 3)
            d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            take = cand & ((best == NONE) | (d2 < bestD))
            best = np.where(take, np.uint32(q), best)
            bestD = np.where(take, d2, bestD)
    return best


def terms(materials, rays, surfaces, probes=None, boxes=None):
    """materials (n, 12), rays (n, 8), surfaces (n, 12) float32 rows -> terms (n, 12), receivers (n, 8), queries (n, 8)"""
    M = np.ascontiguousarray(materials, F).reshape(-1, 12)
    n = M.shape[0]
    miss = (M.view(np.uint32)[:, 11] & MISS) != 0
    D = np.ascontiguousarray(rays, F)[:, 3:6]
    P = np.ascontiguousarray(surfaces, F)[:, 0:3]
    N = np.ascontiguousarray(surfaces, F)[:, 4:7].copy()
    with np.errstate(all="ignore"):
        ln = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
        Vd = (-D) / ln[:, None]
        d = _dot(N, Vd)
        N = np.where((d < 0)[:, None], -N, N)
        d = _dot(N, Vd)
        R = (F(2) * d)[:, None] * N - Vd
        base, metallic = M[:, 0:3], M[:, 3:4]
        T = np.zeros((n, 12), F)
        T[:, 0:3] = base * (F(1) - metallic)
        T[:, 3] = np.sqrt(M[:, 7])
        T[:, 4:7] = F(0.04) + metallic * (base - F(0.04))
        T[:, 7] = np.fmax(d, F(1e-4))
        T[:, 8:11] = M[:, 4:7]
        T[:, 11] = M[:, 8]
    probe = choose_probe(P, None if probes is None else np.ascontiguousarray(probes, F).reshape(-1, 3),
                         None if boxes is None else np.ascontiguousarray(boxes, F).reshape(-1, 8))
    recv = np.zeros((n, 8), F)
    recv[:, 0:3], recv[:, 4:7] = P, N
    qr = np.zeros((n, 8), F)
    qr[:, 0:3], qr[:, 3], qr[:, 4:7] = P, T[:, 3], R
    qr.view(np.uint32)[:, 7] = probe
    T[miss] = 0
    recv[miss] = 0
    qr[miss] = 0
    qr.view(np.uint32)[miss, 7] = NONE
    return T, recv, qr


# ---- compose ----
def table_coord(v, res):
    with np.errstate(all="ignore"):
        x = v * F(res) - F(0.5)
        x = np.where(x > 0, x, F(0))
        x = np.where(x < F(res - 1), x, F(res - 1))
    i = x.astype(np.uint32)
    x0 = np.minimum(i, np.uint32(res - 2))
    return x0, x - x0.astype(F)


def lerp(p, q, f):
    return p + f * (q - p)


def dfg_lookup(dfg, n_dot_v, rho):
    d = np.ascontiguousarray(dfg, F)
    res = d.shape[0]
    x0, fx = table_coord(n_dot_v, res)
    y0, fy = table_coord(rho, res)
    fx, fy = fx[:, None], fy[:, None]
    return lerp(lerp(d[y0, x0], d[y0, x0 + 1], fx), lerp(d[y0 + 1, x0], d[y0 + 1, x0 + 1], fx), fy)         # (n, 2)


def compose(terms_rows, irradiance, reflection, dfg):
    T = np.ascontiguousarray(terms_rows, F).reshape(-1, 12)
    E = np.ascontiguousarray(irradiance, F).reshape(-1, 4)[:, 0:3]
    sp = np.ascontiguousarray(reflection, F).reshape(-1, 4)[:, 0:3]
    miss = ~(T[:, 7] > 0)
    with np.errstate(all="ignore"):
        ab = dfg_lookup(dfg, T[:, 7], T[:, 3])
        A, B = ab[:, 0:1], ab[:, 1:2]
        d = (T[:, 0:3] * E) * INV_PI
        s = sp * (T[:, 4:7] * A + B)
        out = np.ones((T.shape[0], 4), F)
        out[:, 0:3] = T[:, 8:11] + T[:, 11:12] * (d + s)
    out[miss] = 0
    return out
