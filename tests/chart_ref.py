"""The lightmap chart rule (include/ptmi_plugin.h Part 14, csrc/chart_rule.h) restated in numpy: int64 edge functions, fp32 steps one
operator at a time, fp64 divides.  Vectorised over texels and looped over triangles; nothing here calls the library.  Besides the
lists it returns what the cases assert about themselves: per-texel cover counts and whether a sample fell exactly on an edge."""
import numpy as np

F = np.float32
NO_OWNER = 0xFFFFFFFF


def records(tris):
    """(3T, 4) float32 triangle rows (or their bytes) -> v0, e1, e2 (T, 3) float32 and primIdx (T,) by record"""
    t = np.ascontiguousarray(np.asarray(tris).view(np.uint8).reshape(-1)).view(np.float32).reshape(-1, 3, 4)
    return t[:, 2, :3].copy(), t[:, 1, :3].copy(), t[:, 0, :3].copy(), t[:, 2, 3].copy().view(np.uint32)


def snap(u, size):
    """One coordinate: (ok, int64)"""
    with np.errstate(all="ignore"):
        s = F(u) * F(size * 256)
    if not (np.abs(s) <= F(8388608.0)):
        return False, 0
    return True, int(np.rint(s))


def setup(uv, width, height):
    """uv: 6 floats -> (X[3], Y[3], A) as Python ints, or None: not in the chart"""
    X, Y = [], []
    for k in range(3):
        okx, x = snap(uv[2 * k], width)
        oky, y = snap(uv[2 * k + 1], height)
        if not (okx and oky):
            return None
        X.append(x)
        Y.append(y)
    A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    return (X, Y, A) if A != 0 else None


def edge(ax, ay, bx, by, sx, sy):
    """E(a, b; s) on int64 arrays"""
    return np.int64(bx - ax) * (sy - np.int64(ay)) - np.int64(by - ay) * (sx - np.int64(ax))


def cross(e1, e2):
    with np.errstate(all="ignore"):
        c = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], F)
        d = F(F(c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    return c, d


def normalize(v):
    """(n, 3) float32 rows: v * (1 / sqrt((x*x + y*y) + z*z))"""
    with np.errstate(all="ignore"):
        d = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        s = F(1.0) / np.sqrt(d)
        return v * s[:, None]


def instance_normal(w2l, n):
    if w2l is None:
        return n
    w = np.asarray(w2l, F).reshape(16)
    with np.errstate(all="ignore"):
        t = np.stack([((n[:, 0] * w[4 * r] + n[:, 1] * w[4 * r + 1]) + n[:, 2] * w[4 * r + 2]) + F(0.0) * w[4 * r + 3] for r in range(3)], axis=1)
    return normalize(t.astype(F))


def rasterize(tris, attrs, width, height, uvs=None, l2w=None, w2l=None, seed=0):
    """-> dict: texels (n,) uint32 ascending, recv (n, 8) float32, owner (H, W) uint32 (primIdx or NO_OWNER), cover (H, W) number of
    primitives covering each texel, on_edge: a covered sample with an edge value of exactly 0 exists, owners: the set of primIdx that
    own texels, covered (T,): texels each primitive covers (owned or not), shared01 (H, W): texels primitives 0 and 1 both cover"""
    v0, e1, e2, prim = records(tris)
    T = len(prim)
    attrs = np.asarray(attrs).reshape(T)
    owner = np.full((height, width), NO_OWNER, np.uint32)
    cover = np.zeros((height, width), np.int32)
    rec_of = np.zeros(T, np.int64)
    covered = np.zeros(T, np.int64)
    pair = None
    snapped = {}
    on_edge = False
    ys, xs = np.mgrid[0:height, 0:width]
    sx, sy = xs.astype(np.int64) * 256 + 128, ys.astype(np.int64) * 256 + 128
    for t in range(T):
        p = int(prim[t])
        rec_of[p] = t
        uv = np.asarray(uvs, F).reshape(T, 6)[p] if uvs is not None else np.concatenate([attrs[p]["uv0"], attrs[p]["uv1"], attrs[p]["uv2"]]).astype(F)
        s = setup(uv, width, height)
        d = cross(e1[t], e2[t])[1]
        if s is None or d == 0 or not np.isfinite(d):
            continue
        X, Y, A = s
        snapped[p] = s
        sign = -1 if A < 0 else 1
        w = [sign * edge(X[a], Y[a], X[b], Y[b], sx, sy) for a, b in ((1, 2), (2, 0), (0, 1))]
        inside = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)
        on_edge = on_edge or bool((inside & ((w[0] == 0) | (w[1] == 0) | (w[2] == 0))).any())
        cover += inside
        covered[p] = int(inside.sum())
        if p in (0, 1):
            pair = inside if pair is None else (pair & inside)
        owner[inside & (np.uint32(p) < owner)] = p
    flat = owner.reshape(-1)
    texels = np.nonzero(flat != NO_OWNER)[0].astype(np.uint32)
    recv = np.zeros((len(texels), 8), F)
    for p in np.unique(flat[texels]):
        p = int(p)
        sel = np.nonzero(flat[texels] == p)[0]
        idx = texels[sel].astype(np.int64)
        X, Y, A = snapped[p]
        px, py = (idx % width) * 256 + 128, (idx // width) * 256 + 128
        with np.errstate(all="ignore"):
            b1 = (edge(X[2], Y[2], X[0], Y[0], px, py).astype(np.float64) / np.float64(A)).astype(F)
            b2 = (edge(X[0], Y[0], X[1], Y[1], px, py).astype(np.float64) / np.float64(A)).astype(F)
            t = rec_of[p]
            pos = (v0[t][None, :] + e1[t][None, :] * b1[:, None]) + e2[t][None, :] * b2[:, None]
            b0 = F(1.0) - b1 - b2
            n = (attrs[p]["normal0"].astype(F)[None, :] * b0[:, None] + attrs[p]["normal1"].astype(F)[None, :] * b1[:, None]) + \
                attrs[p]["normal2"].astype(F)[None, :] * b2[:, None]
            n = instance_normal(w2l, normalize(n.astype(F)))
            bad = ~np.isfinite(n).all(axis=1)
            if bad.any():
                g = np.repeat(cross(e1[t], e2[t])[0][None, :], len(sel), axis=0)
                n[bad] = instance_normal(w2l, normalize(g))[bad]
            if l2w is not None:
                m = np.asarray(l2w, F).reshape(16)
                pos = np.stack([((m[r] * pos[:, 0] + m[4 + r] * pos[:, 1]) + m[8 + r] * pos[:, 2]) + m[12 + r] for r in range(3)], axis=1)
        recv[sel, 0:3] = pos
        recv[sel, 4:7] = n
        recv[sel, 3] = ((idx + seed) & 0xFFFFFFFF).astype(np.uint32).view(F)
    return {"texels": texels, "recv": recv, "owner": owner, "cover": cover, "on_edge": on_edge, "owners": set(int(p) for p in np.unique(flat[texels])),
            "covered": covered, "shared01": pair if pair is not None else np.zeros((height, width), bool)}


DY = (-1, -1, -1, 0, 0, 1, 1, 1)
DX = (-1, 0, 1, -1, 1, -1, 0, 1)


def resolve(texels, irr, width, height, dilate):
    """-> (H, W, 4) float32: the scatter, then `dilate` passes"""
    img = np.zeros((height * width, 4), F)
    t = np.asarray(texels, np.int64)
    assert (t < width * height).all()
    img[t, 0:3] = np.asarray(irr, F).reshape(-1, 4)[:, 0:3]
    img[t, 3] = 1.0
    img = img.reshape(height, width, 4)
    for _ in range(dilate):
        pad = np.zeros((height + 2, width + 2, 4), F)
        pad[1:-1, 1:-1] = img
        acc = np.zeros((height, width, 3), F)
        n = np.zeros((height, width), np.int32)
        for dy, dx in zip(DY, DX):
            nb = pad[1 + dy:1 + dy + height, 1 + dx:1 + dx + width]
            on = nb[..., 3] != 0
            with np.errstate(all="ignore"):
                acc = np.where(on[..., None], acc + nb[..., 0:3], acc).astype(F)
            n += on
        out = img.copy()
        fill = (img[..., 3] == 0) & (n > 0)
        with np.errstate(all="ignore"):
            out[fill, 0:3] = (acc[fill] / n[fill].astype(F)[:, None]).astype(F)
        out[fill, 3] = 0.5
        img = out
    return img
