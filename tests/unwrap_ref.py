"""The unwrap rule of include/ptmi_plugin.h Part 23 restated in numpy (csrc/unwrap_rule.h is its one definition; this file is
written from that header's text, not from the twin's code).

Every operator is one float32 operation in the order the rule writes it; numpy rounds every elementwise float32 operation once,
so the twin and the kernels must give these bits.  Charts are sets: vertex identity is np.unique over the corners' 96 bits, links
are equal rows of (lo id, hi id, class), components are found by lowering labels until nothing changes."""
import numpy as np

F = np.float32
NO_CHART = 0xFFFFFFFF
EXCLUDED = 0xFF
CHART_DTYPE = [("firstPrim", "<u4"), ("cls", "<u4"), ("triCount", "<u4"), ("reserved", "<u4"), ("umin", "<f4"), ("vmin", "<f4"), ("umax", "<f4"), ("vmax", "<f4")]
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(F)[0]


def corners_of(tris=None, vertices=None):
    """(T, 3, 3) float32 with + 0.0f applied: rows 3p .. 3p + 2 of the vertices, or v0, v0 + e1, v0 + e2 of the record of p"""
    if vertices is not None:
        c = np.ascontiguousarray(vertices, F).reshape(-1, 3, 4)[:, :, :3].copy()
    else:
        rows = np.ascontiguousarray(np.asarray(tris).view(np.uint8).reshape(-1)).view(F).reshape(-1, 3, 4)
        prim = rows[:, 2, 3].copy().view(np.uint32)
        assert sorted(prim) == list(range(len(rows))), "every primitive once"
        e2, e1, v0 = rows[:, 0, :3], rows[:, 1, :3], rows[:, 2, :3]
        with np.errstate(all="ignore"):
            rec = np.stack([v0, v0 + e1, v0 + e2], axis=1)
        c = np.empty_like(rec)
        c[prim] = rec
    with np.errstate(all="ignore"):
        return (c + F(0.0)).astype(F)


def classes(c):
    """(T,) uint32: 2 a + (g[a] < 0), or EXCLUDED"""
    with np.errstate(all="ignore"):
        finite = (np.abs(c) <= F(3.402823466e38)).all(axis=(1, 2))
        e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        d = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        ok = finite & (d != F(0)) & (np.abs(d) <= F(3.402823466e38))
        m = np.abs(g)
        a = np.zeros(len(c), np.uint32)
        a[m[:, 1] > m[:, 0]] = 1                                        # a later axis wins only by >
        best = np.maximum(m[:, 0], np.where(m[:, 1] > m[:, 0], m[:, 1], m[:, 0]))
        a[m[:, 2] > best] = 2
        neg = g[np.arange(len(c)), a] < F(0)
    return np.where(ok, 2 * a + neg, EXCLUDED).astype(np.uint32)


def labels_of(c, cls):
    """(T,) uint32: the lowest primIdx of every included primitive's component (its own index for an excluded one), and the
    number of pairs of equal neighbours in the sorted edge list"""
    T = len(c)
    bits = c.reshape(-1, 3).view(np.uint32)
    _, vid = np.unique(bits, axis=0, return_inverse=True)
    vid = vid.reshape(T, 3).astype(np.int64)
    inc = np.flatnonzero(cls != EXCLUDED)
    a = vid[inc][:, [0, 1, 2]].reshape(-1)
    b = vid[inc][:, [1, 2, 0]].reshape(-1)
    rows = np.stack([np.minimum(a, b), np.maximum(a, b), np.repeat(cls[inc].astype(np.int64), 3)], axis=1)
    prim = np.repeat(inc, 3)
    order = np.lexsort((prim, rows[:, 2], rows[:, 1], rows[:, 0]))
    rows, prim = rows[order], prim[order]
    same = (rows[1:] == rows[:-1]).all(axis=1) if len(rows) > 1 else np.zeros(0, bool)
    p, q = prim[1:][same], prim[:-1][same]
    label = np.arange(T, dtype=np.int64)
    while True:
        before = label.copy()
        low = np.minimum(label[p], label[q])
        np.minimum.at(label, p, low)
        np.minimum.at(label, q, low)
        while True:                                                     # every label follows its label down
            nxt = label[label]
            if (nxt == label).all():
                break
            label = nxt
        if (label == before).all():
            break
    return label.astype(np.uint32), int(same.sum())


def unwrap_charts(tris=None, vertices=None):
    """(chart_of_prim (T,) uint32, charts (n,) CHART_DTYPE, stats dict without the sweeps)"""
    c = corners_of(tris, vertices)
    cls = classes(c)
    label, linked = labels_of(c, cls)
    T = len(c)
    inc = cls != EXCLUDED
    heads = np.flatnonzero(inc & (label == np.arange(T)))
    place = np.full(T, NO_CHART, np.uint32)
    place[heads] = np.arange(len(heads), dtype=np.uint32)
    of = np.where(inc, place[label], NO_CHART).astype(np.uint32)
    charts = np.zeros(len(heads), CHART_DTYPE)
    charts["firstPrim"], charts["cls"] = heads, cls[heads]
    charts["umin"], charts["vmin"], charts["umax"], charts["vmax"] = np.inf, np.inf, -np.inf, -np.inf
    who = np.flatnonzero(inc)
    axis = (cls[label[who]] >> 1).astype(np.int64)
    np.add.at(charts["triCount"], of[who], 1)
    for k in range(3):
        u = c[who, k, (axis + 1) % 3]
        v = c[who, k, (axis + 2) % 3]
        np.minimum.at(charts["umin"], of[who], u)
        np.maximum.at(charts["umax"], of[who], u)
        np.minimum.at(charts["vmin"], of[who], v)
        np.maximum.at(charts["vmax"], of[who], v)
    stats = {"excluded": int((~inc).sum()), "linked_edges": linked, "single_charts": int((charts["triCount"] == 1).sum())}
    return of, charts, stats


def sides(charts, tpu, padding):
    """(w, h, fits) per chart"""
    with np.errstate(all="ignore"):
        su = (charts["umax"] - charts["umin"]) * F(tpu)
        sv = (charts["vmax"] - charts["vmin"]) * F(tpu)
    fits = (su <= F(8192)) & (sv <= F(8192))
    w = np.where(fits, np.ceil(np.where(fits, su, 0)).astype(np.int64) + 1 + 2 * padding, 0)
    h = np.where(fits, np.ceil(np.where(fits, sv, 0)).astype(np.int64) + 1 + 2 * padding, 0)
    return w, h, fits


def pack_charts(charts, width, height, tpu, padding):
    """(origins (n, 2) int32 or None, rows_used): rows_used is set whenever every width fits"""
    w, h, fits = sides(charts, tpu, padding)
    if not fits.all() or (w > width).any():
        return None, 0
    order = sorted(range(len(charts)), key=lambda i: (-h[i], -w[i], charts["firstPrim"][i], i))
    origins = np.zeros((len(charts), 2), np.int32)
    x = y = shelf = 0
    ok = True
    for i in order:
        if x + w[i] > width:
            y, x, shelf = y + shelf, 0, 0
        if x == 0:
            shelf = h[i]
        if y + h[i] > height:
            ok = False
        origins[i] = (x, y)
        x += w[i]
    return (origins if ok else None), int(y + shelf)


def emit_uvs(chart_of_prim, charts, origins, width, height, tpu, padding, tris=None, vertices=None):
    """(T, 6) float32"""
    c = corners_of(tris, vertices)
    T = len(c)
    uvs = np.full((T, 6), QUIET_NAN, F)
    who = np.flatnonzero(chart_of_prim < len(charts))
    ch = charts[chart_of_prim[who]]
    o = np.asarray(origins, np.int32).reshape(-1, 2)[chart_of_prim[who]]
    axis = (ch["cls"] >> 1).astype(np.int64)
    with np.errstate(all="ignore"):
        for k in range(3):
            u = c[who, k, (axis + 1) % 3]
            v = c[who, k, (axis + 2) % 3]
            uvs[who, 2 * k] = ((((u - ch["umin"]) * F(tpu)) + (o[:, 0] + padding).astype(F)) + F(0.5)) / F(width)
            uvs[who, 2 * k + 1] = ((((v - ch["vmin"]) * F(tpu)) + (o[:, 1] + padding).astype(F)) + F(0.5)) / F(height)
    return uvs
