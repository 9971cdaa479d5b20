"""The skinning rule (include/ptmi_plugin.h Part 11) restated in numpy float32, for the tests.

Written from the rule, not from the C++: every array is float32 and every line below is ONE elementwise IEEE binary32 operation
(numpy never contracts a product and a sum), in the rule's order, left to right.  The square root and the division are correctly
rounded in numpy as on both sides of the product.  Min and max only select values."""
import numpy as np

F = np.float32


def blend(joints, weights, palette):
    """(n, 4) uint16, (n, 4) float32, (J, 12) float32 -> (n, 12): ((w0 M[j0] + w1 M[j1]) + w2 M[j2]) + w3 M[j3], all four terms"""
    j = np.asarray(joints).astype(np.int64)
    w = np.asarray(weights, F)
    m = np.asarray(palette, F).reshape(-1, 12)
    t0 = w[:, 0:1] * m[j[:, 0]]
    t1 = w[:, 1:2] * m[j[:, 1]]
    t2 = w[:, 2:3] * m[j[:, 2]]
    t3 = w[:, 3:4] * m[j[:, 3]]
    b = t0 + t1
    b = b + t2
    b = b + t3
    assert b.dtype == F
    return b


def rows3(b, x, y, z):
    """(B[r][0] x + B[r][1] y) + B[r][2] z for the three rows -> (n, 3)"""
    out = np.empty((len(b), 3), F)
    for r in range(3):
        px = b[:, 4 * r] * x
        py = b[:, 4 * r + 1] * y
        pz = b[:, 4 * r + 2] * z
        s = px + py
        s = s + pz
        out[:, r] = s
    return out


def positions(b, rest):
    """(n, 12), (n, 4) -> (n, 4): rows3 + the translation; w = 0"""
    rest = np.asarray(rest, F)
    p = rows3(b, rest[:, 0], rest[:, 1], rest[:, 2])
    out = np.zeros((len(b), 4), F)
    for r in range(3):
        out[:, r] = p[:, r] + b[:, 4 * r + 3]
    return out


def directions(b, v):
    """(n, 12), (n, 3) -> (n, 3): v' = B3 v, v' * (1 / sqrt(dot(v', v'))); a dot that is 0 or not finite keeps v"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        t = rows3(b, v[:, 0], v[:, 1], v[:, 2])
        xx = t[:, 0] * t[:, 0]
        yy = t[:, 1] * t[:, 1]
        zz = t[:, 2] * t[:, 2]
        d = xx + yy
        d = d + zz
        root = np.sqrt(d)
        s = F(1.0) / root
        out = t * s[:, None]
    keep = (d == 0) | ~np.isfinite(d)
    out[keep] = v[keep]
    assert out.dtype == F
    return out


def skin(rest, joints, weights, palette, rest_attrs=None):
    """-> (vertices (3T, 4) float32, attribute records or None, bounds (2, 3) float32: min, max)"""
    b = blend(joints, weights, palette)
    verts = positions(b, rest)
    attrs = None
    if rest_attrs is not None:
        attrs = np.array(rest_attrs, copy=True)             # pads, uvs and materialIndex: the rest record's
        rows = attrs.view(F).reshape(-1, 8, 4)              # a record as 8 rows of 4 floats
        bt = b.reshape(-1, 3, 12)
        for corner in range(3):
            rows[:, corner, :3] = directions(bt[:, corner], rows[:, corner, :3].copy())
            rows[:, 3 + corner, :3] = directions(bt[:, corner], rows[:, 3 + corner, :3].copy())
    return verts, attrs, np.stack([verts[:, :3].min(axis=0), verts[:, :3].max(axis=0)])
