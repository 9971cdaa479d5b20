"""The direct-light rule (include/ptmi_plugin.h Part 24) restated in numpy from the header's text, not from the C++: float32
arrays, one numpy operation per operator of the rule, in the order written.  `rays` and `accumulate` are what the host twins and
the kernels must equal bit for bit; `contributions_f64` evaluates the same formula in float64."""
import numpy as np

F = np.float32
U = np.uint32
SPOT, DIRECTIONAL, POINT, RECTANGLE = 0, 1, 2, 3
EPSILON = F(0.0001)
FAR_PLANE = F(100000.0)
INV_PI = F(0.31830988618379067)
PI = F(3.14159265)
CENTERED = 1


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v, one):
    s = one / np.sqrt(_dot(v, v))
    return v * s[..., None]


def _saturate(x):
    return np.fmin(np.fmax(x, x.dtype.type(0)), x.dtype.type(1))


def rng_next(s):
    old = (s + U(747796405) + U(2891336453)).astype(U)
    word = (((old >> ((old >> U(28)) + U(4))) ^ old) * U(277803737)).astype(U)
    return ((word >> U(22)) ^ word).astype(U)


def random_float(s):
    s = rng_next(s)
    return s, s.astype(F) / F(4294967296.0)


def smith_g(c, alpha, T):
    a = alpha * alpha
    b = c * c
    return (T(2) * c) / (c + np.sqrt((a + b) - a * b))


def pairs_of(kind, strata):
    return 1 if kind in (POINT, SPOT) else strata * strata if kind == RECTANGLE else 0


def pair_count(lights, strata):
    L = np.asarray(lights, F).reshape(-1, 16)
    return sum(pairs_of(int(k), strata) for k in L[:, 3].view(U))


def _light(row, T):
    """the record and its derived rows n, nn in type T (float32 for the rule, float64 for the formula)"""
    row = np.asarray(row, F)
    kind = int(row[3:4].view(U)[0])
    rec = {"kind": kind, "position": row[0:3].astype(T), "emission": row[4:7].astype(T), "range": T(row[7]), "u": row[8:11].astype(T), "area": T(row[11]),
           "v": row[12:15].astype(T)}
    u, v = rec["u"], rec["v"]
    n = np.zeros(3, T)
    with np.errstate(all="ignore"):
        if kind == RECTANGLE:
            n = _normalize(np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], T), T(1))
        elif kind == SPOT:
            n = _normalize(u, T(1))
        rec["n"], rec["nn"] = n, _normalize(n, T(1))
    return rec


def _pair(T, lt, strata, k, x1, x2, O, N, Vd, alpha, a2, n_dot_v, diffuse, f0):
    """steps 5 to 7 for pair k of one light over all entries in type T -> (counts (n,), L (n, 3), c (n, 3))"""
    one = T(1)
    b, a = divmod(k, strata)
    if lt["kind"] == RECTANGLE:
        r1 = (T(a) + x1) / T(strata)
        r2 = (T(b) + x2) / T(strata)
        p = (lt["position"] + lt["u"] * r1[:, None]) + lt["v"] * r2[:, None]
        q = p - O
        dist = np.sqrt(_dot(q, q))
        L = q / dist[:, None]
    else:
        q = O - lt["position"]
        dist = np.sqrt(_dot(q, q))
        L = -(q * (one / dist)[:, None])
    r = dist / lt["range"]
    falloff = _saturate((one / (one + (T(25) * r) * r)) * _saturate((one - r) * T(5)))
    falloff = np.where(dist > lt["range"], T(0), falloff)
    if lt["kind"] != POINT:
        cos_theta = _dot(_normalize(-L, one), lt["nn"])
        if lt["kind"] == RECTANGLE:
            falloff = np.where(cos_theta < 0, T(0), falloff)
        else:
            vx, vy = lt["v"][0], lt["v"][1]
            scaled = falloff * ((cos_theta - vx) / (vy - vx))
            falloff = np.where(cos_theta < vx, T(0), np.where((cos_theta > vx) & (cos_theta < vy), scaled, falloff))
    Li = lt["emission"] * falloff[:, None]
    nl = _dot(N, L)
    H = Vd + L
    length = np.sqrt(_dot(H, H))
    lobe = length > 0
    H = H / length[:, None]
    nh, vh = _dot(N, H), _dot(Vd, H)
    nh = np.where(nh > 0, nh, T(0))
    vh = np.where(vh > 0, vh, T(0))
    t = (nh * nh) * (a2 - one) + one
    D = a2 / ((T(PI) * t) * t)
    G = smith_g(n_dot_v, alpha, T) * smith_g(nl, alpha, T)
    m = one - vh
    Fc = ((m * m) * (m * m)) * m
    Fr = f0 + (one - f0) * Fc[:, None]
    sp = (D * G) / ((T(4) * nl) * n_dot_v)
    f = diffuse * T(INV_PI)
    f = np.where(lobe[:, None], f + Fr * sp[:, None], f)
    w = np.ones_like(nl)
    if lt["kind"] == RECTANGLE:
        w = ((lt["area"] * np.abs(_dot(lt["n"][None], L))) / (dist * dist)) / T(strata * strata)
    c = ((Li * f) * nl[:, None]) * w[:, None]
    counts = (nl > 0) & np.isfinite(c).all(axis=1) & (c > 0).any(axis=1)
    return counts, L, c


def _entries(T, rays, terms, receivers, min_alpha):
    rays, terms, receivers = (np.asarray(x, F) for x in (rays, terms, receivers))
    D = rays[:, 3:6].astype(T)
    length = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
    Vd = (-D) / length[:, None]
    rho = terms[:, 3].astype(T)
    alpha = rho * rho
    alpha = np.where(T(min_alpha) > alpha, T(min_alpha), alpha)
    N = receivers[:, 4:7].astype(T)
    O = receivers[:, 0:3].astype(T) + N * T(EPSILON)
    return dict(O=O, N=N, Vd=Vd, alpha=alpha, a2=alpha * alpha, n_dot_v=terms[:, 7].astype(T), diffuse=terms[:, 0:3].astype(T), f0=terms[:, 4:7].astype(T))


def _walk(T, lights, rays, terms, receivers, strata, seed, flags, min_alpha):
    """yields (pair offset, counts, L, c, O) per pair of every light, in pair order, evaluated in type T (the jitter is the rule's
    float32 draw in either case)"""
    terms = np.asarray(terms, F)
    n = terms.shape[0]
    hit = terms[:, 7] > 0
    with np.errstate(all="ignore"):
        e = _entries(T, rays, terms, receivers, min_alpha)
        s = rng_next(np.full(n, seed & 0xFFFFFFFF, U))
        s = (s + np.arange(n, dtype=np.uint64).astype(U)).astype(U)
        pair = 0
        for row in np.asarray(lights, F).reshape(-1, 16):
            lt = _light(row, T)
            for k in range(pairs_of(lt["kind"], strata)):
                x1 = x2 = np.full(n, 0.5, T)
                if lt["kind"] == RECTANGLE and not flags & CENTERED:
                    s, d1 = random_float(s)
                    s, d2 = random_float(s)
                    x1, x2 = d1.astype(T), d2.astype(T)
                counts, L, c = _pair(T, lt, strata, k, x1, x2, **e)
                yield pair, counts & hit, L, c, e["O"]
                pair += 1


def rays(lights, rays_in, terms, receivers, strata=1, seed=0, flags=0, min_alpha=0.0):
    """steps 2 to 7 -> (pair rays (n * pairs, 8), contributions (n * pairs, 4)) float32"""
    n, pairs = np.asarray(terms).shape[0], pair_count(lights, strata)
    out_rays, contrib = np.zeros((n, pairs, 8), F), np.zeros((n, pairs, 4), F)
    for pair, counts, L, c, O in _walk(F, lights, rays_in, terms, receivers, strata, seed, flags, F(min_alpha)):
        out_rays[counts, pair, 0:3] = O[counts]
        out_rays[counts, pair, 3:6] = L[counts]
        out_rays[counts, pair, 6] = FAR_PLANE
        contrib[counts, pair, 0:3] = c[counts]
    return out_rays.reshape(-1, 8), contrib.reshape(-1, 4)


def contributions_f64(lights, rays_in, terms, receivers, strata=1, seed=0, flags=0, min_alpha=0.0):
    """the same formula in float64 over the float32 inputs -> (counts (n * pairs,), c (n * pairs, 3))"""
    n, pairs = np.asarray(terms).shape[0], pair_count(lights, strata)
    ok, out = np.zeros((n, pairs), bool), np.zeros((n, pairs, 3), np.float64)
    for pair, counts, L, c, O in _walk(np.float64, lights, rays_in, terms, receivers, strata, seed, flags, float(F(min_alpha))):
        ok[:, pair] = counts
        out[counts, pair] = c[counts]
    return ok.reshape(-1), out.reshape(-1, 3)


def accumulate(terms, contrib, pair_hits, pairs):
    """step 8 -> (n, 4) float32; pair_hits: (n * pairs, 4) PTRayHit rows"""
    terms = np.asarray(terms, F)
    n = terms.shape[0]
    c = np.asarray(contrib, F).reshape(n, pairs, 4)
    prim = np.ascontiguousarray(pair_hits, dtype=F).view(U).reshape(n, pairs, 4)[:, :, 3]
    out = np.zeros((n, 4), F)
    for k in range(pairs):
        add = (prim[:, k] == 0xFFFFFFFF) & (c[:, k, 0:3] > 0).any(axis=1)
        out[add, 0:3] = out[add, 0:3] + c[add, k, 0:3]
    hit = terms[:, 7] > 0
    out[hit, 3] = 1
    out[~hit] = 0
    return out
