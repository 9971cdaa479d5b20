"""The morph rule (include/ptmi_plugin.h Part 12) restated in numpy float32, for the tests.

Written from the rule, not from the C++: every array is float32 and every line of arithmetic below is ONE elementwise IEEE binary32
operation (numpy never contracts a product and a sum), in the rule's order.  The skin step is tests/skin_ref.py's.  Only listed
entries are applied: the fold walks each corner's own entries and never invents a zero for a target the corner does not list."""
import numpy as np

import skin_ref

F = np.float32


def fold(start, stream, weights):
    """start (n, 3) float32; stream (offsets (n + 1,), entries MORPH_ENTRY[]) or None -> (acc (n, 3), listed (n,) bool):
    acc = acc + w[target] * d per component, for each entry of the corner in order"""
    acc = np.array(start, F, copy=True)
    n = len(acc)
    if stream is None:
        return acc, np.zeros(n, bool)
    off = np.asarray(stream[0]).astype(np.int64)
    ent = stream[1]
    w = np.asarray(weights, F)
    count = off[1:] - off[:-1]
    with np.errstate(all="ignore"):
        for s in range(int(count.max()) if n else 0):
            sel = np.nonzero(count > s)[0]                   # the corners that have an s-th entry
            e = ent[off[sel] + s]
            ws = w[e["target"].astype(np.int64)]
            for a, f in enumerate(("dx", "dy", "dz")):
                product = ws * e[f]
                acc[sel, a] = acc[sel, a] + product
    assert acc.dtype == F
    return acc, count > 0


def normalized(m, rest):
    """m * (1 / sqrt(dot(m, m))); a dot that is 0 or not finite keeps REST"""
    with np.errstate(all="ignore"):
        xx = m[:, 0] * m[:, 0]
        yy = m[:, 1] * m[:, 1]
        zz = m[:, 2] * m[:, 2]
        d = xx + yy
        d = d + zz
        root = np.sqrt(d)
        s = F(1.0) / root
        out = m * s[:, None]
    keep = (d == 0) | ~np.isfinite(d)
    out[keep] = rest[keep]
    assert out.dtype == F
    return out


def skinned_direction(b, m, rest):
    """skin_ref.directions of m, but its fallback (the dot of B3 m is 0 or not finite) yields REST, not m"""
    with np.errstate(all="ignore"):
        t = skin_ref.rows3(b, m[:, 0], m[:, 1], m[:, 2])
        xx = t[:, 0] * t[:, 0]
        yy = t[:, 1] * t[:, 1]
        zz = t[:, 2] * t[:, 2]
        d = xx + yy
        d = d + zz
    out = skin_ref.directions(b, m)
    keep = (d == 0) | ~np.isfinite(d)
    out[keep] = rest[keep]
    return out


def morph(rest, position, weights, normal=None, tangent=None, rest_attrs=None, skin=None, palette=None):
    """rest (3T, 4); position / normal / tangent CSR streams (offsets, entries) or None (position is required); skin = (joints,
    weights) with palette, or both None -> (vertices (3T, 4) float32, attribute records or None, bounds (2, 3) float32: min, max)"""
    rest = np.asarray(rest, F)
    acc, _ = fold(rest[:, :3], position, weights)
    b = None
    if palette is not None:
        b = skin_ref.blend(skin[0], skin[1], palette)
        verts = skin_ref.positions(b, np.concatenate([acc, np.zeros((len(acc), 1), F)], axis=1))
    else:
        verts = np.zeros((len(acc), 4), F)
        verts[:, :3] = acc
    attrs = None
    if rest_attrs is not None:
        attrs = np.array(rest_attrs, copy=True)             # tangent w, pads, uvs and materialIndex: the rest record's
        rows = attrs.view(F).reshape(-1, 8, 4)              # a record as 8 rows of 4 floats
        for first, stream in ((0, normal), (3, tangent)):
            r = rows[:, first:first + 3, :3].reshape(-1, 3).copy()          # corner 3t + c is row first + c of record t
            m, listed = fold(r, stream, weights)
            if b is not None:
                out = skinned_direction(b, m, r)
            else:
                out = r.copy()                              # no entry, no palette: bit for bit
                out[listed] = normalized(m[listed], r[listed])
            rows[:, first:first + 3, :3] = out.reshape(-1, 3, 3)
    return verts, attrs, np.stack([verts[:, :3].min(axis=0), verts[:, :3].max(axis=0)])
