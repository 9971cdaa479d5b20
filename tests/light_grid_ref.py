"""The light-grid rule (include/ptmi_plugin.h Part 25, csrc/light_grid_rule.h's header comment) restated in numpy: float32 arrays,
one numpy operation per operator of the rule, in the order written, every cell of the grid at once.  `build` is what the host twin
and the kernels must equal byte for byte; `cell_of` is the cell rule; `box` the inflated boxes."""
import numpy as np

import direct_ref as dref

F = np.float32
U = np.uint32
SPOT, DIRECTIONAL, POINT, RECTANGLE = 0, 1, 2, 3
PAD_CELL = F(2.0 ** -10)
PAD_EXTENT = F(2.0 ** -20)
SLACK = F(1.0009765625)
PLANE_MARGIN = F(2.0 ** -16)


def cell_count(dims):
    return int(dims[0]) * int(dims[1]) * int(dims[2])


def cell_of(origin, cell_size, dims, X):
    """the cell index of every row of X (n, 3) float32; cells = the overflow cell"""
    origin, cs, X = np.asarray(origin, F), F(cell_size), np.asarray(X, F).reshape(-1, 3)
    d = np.asarray(dims, U)
    with np.errstate(all="ignore"):
        t = (X - origin[None]) / cs
        inside = (t >= F(0)) & (t < d.astype(F)[None])
        i = np.where(inside, t, F(0)).astype(U)
    cell = (i[:, 2] * d[1] + i[:, 1]) * d[0] + i[:, 0]
    return np.where(inside.all(axis=1), cell, U(cell_count(dims))).astype(U)


def box(origin, cell_size, dims):
    """(lo, hi), each (cells, 3) float32: the inflated box of every cell in cell order"""
    origin, cs = np.asarray(origin, F), F(cell_size)
    d = np.asarray(dims, U)
    c = np.arange(cell_count(dims), dtype=U)
    i = np.stack([c % d[0], (c // d[0]) % d[1], c // (d[0] * d[1])], axis=1)
    pad = cs * PAD_CELL + (np.abs(origin) + cs * d.astype(F)) * PAD_EXTENT
    lo = (origin[None] + cs * i.astype(F)) - pad[None]
    hi = (origin[None] + cs * (i + U(1)).astype(F)) + pad[None]
    return lo, hi


def lists(row, lo, hi):
    """(cells,) bool: which cells list the light"""
    lt = dref._light(row, F)
    kind = lt["kind"]
    n = lo.shape[0]
    if kind not in (POINT, SPOT, RECTANGLE):
        return np.zeros(n, bool)
    e = lt["emission"]
    if not (e[0] != 0 or e[1] != 0 or e[2] != 0):
        return np.zeros(n, bool)
    rect = kind == RECTANGLE
    u, v, pos = lt["u"], lt["v"], lt["position"]
    with np.errstate(all="ignore"):
        R = lt["range"]
        if rect:
            R = lt["range"] + F(0.5) * (np.sqrt(dref._dot(u, u)) + np.sqrt(dref._dot(v, v)))
        Rr = R * SLACK
        R2 = Rr * Rr
        C = (pos + F(0.5) * u) + F(0.5) * v if rect else pos
        d = np.where(C[None] < lo, lo - C[None], np.where(C[None] > hi, C[None] - hi, F(0)))
        d2 = dref._dot(d, d)
        listed = ~(d2 > R2)
        if rect or (kind == SPOT and v[0] >= 0):
            N = lt["n"]
            ee = (lo + hi) * F(0.5) - pos[None]
            h = (hi - lo) * F(0.5)
            s = dref._dot(ee, N[None]) + ((np.abs(N[0]) * h[:, 0] + np.abs(N[1]) * h[:, 1]) + np.abs(N[2]) * h[:, 2])
            listed &= ~(s + Rr * PLANE_MARGIN < F(0))
    return listed


def build(lights, origin, cell_size, dims):
    """(offsets (cells + 2,), indices (total,), rect_before (L + 1,)) uint32"""
    L = np.asarray(lights, F).reshape(-1, 16)
    lo, hi = box(origin, cell_size, dims)
    cells = lo.shape[0]
    listed = np.zeros((cells + 1, L.shape[0]), bool)
    for l in range(L.shape[0]):
        listed[:cells, l] = lists(L[l], lo, hi)
    listed[cells, :] = True                                               # the overflow cell: every light
    counts = listed.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(U)
    indices = np.nonzero(listed)[1].astype(U)                             # row-major: cell by cell, ascending light index
    is_rect = L[:, 3].view(U) == RECTANGLE
    rect_before = np.concatenate([[0], np.cumsum(is_rect)]).astype(U)
    return offsets, indices, rect_before
