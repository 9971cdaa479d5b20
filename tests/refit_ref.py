"""The CWBVH refit rule (include/ptmi_plugin.h Part 9) restated in numpy float32, for the tests.

Written from the rule, not from the C++: selections are made on Python floats (a float32 is exactly a double, and a
compare-and-select only picks values), every rounded operation (the subtractions of the triangle records, the extent, the
offset from lo, the division by the grid cell) is one numpy float32 operation, and the exponent is found with exact
arithmetic as the smallest e with 255 * 2^e >= extent."""
import math

import numpy as np

F = np.float32
INF = float("inf")


def exponent(extent) -> int:
    """Smallest e with 255 * 2^e >= extent, clamped to -120 ... 126; extents that are not > 1e-36f take -120."""
    extent = F(extent)
    if not (extent > F(1e-36)):
        return -120
    if not math.isfinite(float(extent)):
        return 126
    x = float(extent)
    e = math.frexp(x)[1] - 9
    while x > 255.0 * 2.0 ** e:          # exact in doubles: a float32 times a power of two against 255 times a power of two
        e += 1
    return min(max(e, -120), 126)


def clamp_byte(v) -> int:
    v = float(v)
    return int(0.0 if v < 0.0 else (255.0 if v > 255.0 else v))


def _fold(acc, box):
    mn, mx = acc
    for a in range(3):
        if box[0][a] < mn[a]:
            mn[a] = box[0][a]
        if box[1][a] > mx[a]:
            mx[a] = box[1][a]


def refit(nodes, tris, vertices):
    """nodes, tris: the uint8 arrays of a CWBVH (5 x 16 bytes per node, 3 x 16 bytes per triangle record); vertices:
    (3 * triangles, 4) float32 in primitive order.  Returns the refitted (nodes, tris) as new uint8 arrays."""
    nodes = np.array(nodes, dtype=np.uint8, copy=True).reshape(-1, 80)
    tris = np.array(tris, dtype=np.uint8, copy=True).reshape(-1, 48)
    words = nodes.view(np.uint32)                       # (n, 20)
    lo_out = nodes.view(np.float32)
    tf, tu = tris.view(np.float32), tris.view(np.uint32)    # (records, 12)
    v = np.ascontiguousarray(vertices, dtype=np.float32)[:, :3].reshape(-1, 3, 3)
    prim = tu[:, 11].astype(np.int64)
    # triangle records: e2, e1 (w = 0), v0 | primIdx -- one IEEE subtraction per component
    tf[:, 0:3] = v[prim, 2] - v[prim, 0]
    tf[:, 3] = 0.0
    tf[:, 4:7] = v[prim, 1] - v[prim, 0]
    tf[:, 7] = 0.0
    tf[:, 8:11] = v[prim, 0]
    vl = v.astype(np.float64).tolist()                  # exact

    def leaf_box(first_record, count):
        box = ([INF] * 3, [-INF] * 3)
        for r in range(first_record, first_record + count):         # record order, vertices 0, 1, 2
            for p in vl[int(prim[r])]:
                _fold(box, (p, p))
        return box

    def node_box(n):
        child_base, tri_base = int(words[n, 4]), int(words[n, 5])
        meta = nodes[n, 24:32]
        slots, inner = {}, 0
        box = ([INF] * 3, [-INF] * 3)
        for s in range(8):                              # ascending slot order
            m = int(meta[s])
            if m == 0:
                continue
            if (m & 0x18) == 0x18:
                slots[s] = node_box(child_base + inner)
                inner += 1
            else:
                slots[s] = leaf_box((tri_base + 3 * (m & 31)) // 3, bin(m >> 5).count("1"))
            _fold(box, slots[s])
        lo = [F(x) for x in box[0]]
        e = [exponent(F(box[1][a]) - lo[a]) for a in range(3)]
        q = np.zeros(48, np.uint8)
        for s, b in slots.items():
            for a in range(3):
                cell = F(2.0 ** e[a])
                q[8 * a + s] = clamp_byte(np.floor((F(b[0][a]) - lo[a]) / cell))
                q[24 + 8 * a + s] = clamp_byte(np.ceil((F(b[1][a]) - lo[a]) / cell))
        lo_out[n, 0:3] = lo
        nodes[n, 12:15] = [x & 255 for x in e]          # imask (byte 15) and row n1 stay
        nodes[n, 32:80] = q
        return box

    with np.errstate(over="ignore", invalid="ignore"):
        node_box(0)
    return nodes.reshape(-1), tris.reshape(-1)


def decoded_boxes_contain(nodes, tris, vertices):
    """Every occupied slot's decoded box (lo + q * 2^e, in exact arithmetic) contains the child's true box: the vertices of a
    leaf's triangles, the union of the vertices below an inner child.  Also: every exponent lies in -120 ... 126.  Returns the
    number of slots checked."""
    from fractions import Fraction
    nodes = np.asarray(nodes, np.uint8).reshape(-1, 80)
    words, lof = nodes.view(np.uint32), nodes.view(np.float32)
    tu = np.asarray(tris, np.uint8).reshape(-1, 48).view(np.uint32)
    v = np.asarray(vertices, np.float32)[:, :3].reshape(-1, 3, 3).astype(np.float64)
    checked = 0

    def true_box(n):
        nonlocal checked
        child_base, tri_base = int(words[n, 4]), int(words[n, 5])
        e = nodes[n, 12:15].view(np.int8).astype(int)
        assert all(-120 <= x <= 126 for x in e), e
        inner, boxes = 0, []
        for s in range(8):
            m = int(nodes[n, 24 + s])
            if m == 0:
                assert not nodes[n, 32 + s:80:8].any()              # bytes of empty slots stay 0
                continue
            if (m & 0x18) == 0x18:
                mn, mx = true_box(child_base + inner)
                inner += 1
            else:
                r0 = (tri_base + 3 * (m & 31)) // 3
                p = v[tu[r0:r0 + bin(m >> 5).count("1"), 11].astype(np.int64)].reshape(-1, 3)
                mn, mx = p.min(axis=0), p.max(axis=0)
            for a in range(3):
                lo, cell = Fraction(float(lof[n, a])), Fraction(2) ** int(e[a])
                assert lo + int(nodes[n, 32 + 8 * a + s]) * cell <= Fraction(float(mn[a])), (n, s, a, "lo")
                assert lo + int(nodes[n, 56 + 8 * a + s]) * cell >= Fraction(float(mx[a])), (n, s, a, "hi")
            checked += 1
            boxes.append((mn, mx))
        return np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)

    true_box(0)
    return checked
