"""The lightmap lookup of include/ptmi_plugin.h Part 22 restated in numpy (csrc/lightmap_lookup_rule.h is its one definition).

Every operator is one float32 operation in the order the rule writes it; numpy rounds every elementwise float32 operation once,
so the twin and the kernels must give these bits.  Bindings are the dicts plugin.lightmap_bindings takes."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF


def step1(material_count, rays, hits, surfaces):
    """(miss, back): a miss as Part 21 step 2 defines it; d < 0 of the normal as the surface record gives it"""
    prim = hits.view(np.uint32)[:, 3]
    miss = (prim == NONE) | (surfaces.view(np.uint32)[:, 7] >= np.uint32(material_count))
    D, N = rays[:, 3:6], surfaces[:, 4:7]
    with np.errstate(all="ignore"):
        length = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
        Vd = (-D) / length[:, None]
        d = (N[:, 0] * Vd[:, 0] + N[:, 1] * Vd[:, 1]) + N[:, 2] * Vd[:, 2]
        back = d < F(0)
    return miss, back & ~miss


def choose(bindings, miss, back, prim, instance):
    """step 2: the first binding in ascending order that matches"""
    chosen = np.full(prim.shape[0], NONE, np.uint32)
    for k, b in enumerate(bindings):
        inside = (prim - np.uint32(b["first_prim"])).astype(np.uint32) < np.uint32(b["prim_count"])            # wraps, as the uint32 does
        whose = np.ones_like(miss) if b.get("instance") is None else instance == np.uint32(b["instance"])
        side = ~back | bool(b.get("two_sided"))
        chosen[~miss & (chosen == NONE) & inside & whose & side] = k
    return chosen


def _axis(u, size):
    """x, whether it is in reach, the fraction, the two taps' inside flags and clamped coordinates"""
    with np.errstate(all="ignore"):
        x = u * F(size) - F(0.5)
        ok = (x > F(-1.0)) & (x < F(size))
        xs = np.where(ok, x, F(0))
        xf = np.floor(xs)
        x0 = xf.astype(np.int32)
        f = xs - xf
    in0, in1 = x0 >= 0, x0 + 1 < size
    return x, ok, f, in0, in1, np.where(in0, x0, 0), np.where(in1, x0 + 1, size - 1)


def _blend(va, vb, a, b, f):
    with np.errstate(all="ignore"):
        both = a + f[:, None] * (b - a)
    return np.where((va & vb)[:, None], both, np.where(va[:, None], a, b)), va | vb


def lookup(bindings, tri_attrs, material_count, rays, hits, surfaces, details=False):
    """(irradiance (n, 4) float32, binding (n,) uint32); with details also the footprint coordinates x, y (float32, NaN where no
    binding was chosen)"""
    rays, hits, surfaces = (np.ascontiguousarray(a, F) for a in (rays, hits, surfaces))
    n = rays.shape[0]
    miss, back = step1(material_count, rays, hits, surfaces)
    prim, instance = hits.view(np.uint32)[:, 3], surfaces.view(np.uint32)[:, 10]
    chosen = choose(bindings, miss, back, prim, instance)
    out, which = np.zeros((n, 4), F), np.full(n, NONE, np.uint32)
    X, Y = np.full(n, np.nan, F), np.full(n, np.nan, F)
    for k, b in enumerate(bindings):
        e = np.flatnonzero(chosen == k)
        if not e.size:
            continue
        image = np.ascontiguousarray(b["image"], F)
        h, w = image.shape[0], image.shape[1]
        p = prim[e] - np.uint32(b["first_prim"])
        if b.get("uvs") is not None:
            uv = np.asarray(b["uvs"], F).reshape(-1, 6)[p]
        else:
            a = tri_attrs[prim[e]]
            uv = np.concatenate([a["uv0"], a["uv1"], a["uv2"]], axis=1).astype(F)
        b1, b2 = hits[e, 1], hits[e, 2]
        with np.errstate(all="ignore"):
            w0 = F(1.0) - b1 - b2
            U = (uv[:, 0] * w0 + uv[:, 2] * b1) + uv[:, 4] * b2
            V = (uv[:, 1] * w0 + uv[:, 3] * b1) + uv[:, 5] * b2
        x, okx, fx, inx0, inx1, cx0, cx1 = _axis(U, w)
        y, oky, fy, iny0, iny1, cy0, cy1 = _axis(V, h)
        X[e], Y[e] = x, y
        t00, t10, t01, t11 = image[cy0, cx0], image[cy0, cx1], image[cy1, cx0], image[cy1, cx1]
        with np.errstate(invalid="ignore"):
            v00, v10 = inx0 & iny0 & (t00[:, 3] > F(0)), inx1 & iny0 & (t10[:, 3] > F(0))
            v01, v11 = inx0 & iny1 & (t01[:, 3] > F(0)), inx1 & iny1 & (t11[:, 3] > F(0))
        r0, row0 = _blend(v00, v10, t00[:, 0:3], t10[:, 0:3], fx)
        r1, row1 = _blend(v01, v11, t01[:, 0:3], t11[:, 0:3], fx)
        E, found = _blend(row0, row1, r0, r1, fy)
        found &= okx & oky
        out[e[found], 0:3] = E[found]
        which[e[found]] = k
    return (out, which, X, Y) if details else (out, which)
