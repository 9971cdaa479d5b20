"""The rule of the device CWBVH builder (PTBuildBVHDevice, csrc/bvh_builder_gpu.hip) restated in numpy float32,
for the tests.

Written from the rule, not from the kernels, in the style of refit_ref.py: selections are made on exact values, every rounded
operation is one numpy float32 operation in the order the rule gives, and the Morton key is interleaved with a plain loop over
bits.  The rule:

  triangle box   componentwise min / max of the three vertices; centroid 0.5f * (mn + mx)
  scene bounds   min / max of the centroids per axis
  key            per axis t = ext > 0 ? (c - lo) / ext : 0, clamped to [0, 1]; q = min(uint(t * 2^21), 2^21 - 1); bit 3b + 2 of
                 the key is bit b of q.x, bit 3b + 1 of q.y, bit 3b of q.z
  order          stable sort by key
  binary tree    over sorted positions [a, b]: split below the highest differing bit of the two keys, or, for equal keys, of
                 the two positions (a top-down recursion: the tree Karras's per-node search finds)
  wide node      a subtree of <= 3 triangles is a leaf child; start from the root's two children (a root of <= 3 triangles: one
                 leaf child); while there are fewer than 8, open the expandable child with the largest (ex*ey + ey*ez) + ez*ex
                 (strict >, the first wins a tie); the left child takes its place, the right one is appended
  slots          cost[s][i] = ((cx*dx) + (cy*dy)) + (cz*dz), c = child centre - node centre (centres 0.5f * (mn + mx)), d = -1
                 where bit 4 / 2 / 1 of s is set, else +1; `count` rounds, each taking the smallest cost over free slots x
                 unplaced children (slots outer, children inner, strict <); no cost compares: first unplaced child, first free slot
  encode         refit_ref.refit's: origin = min of the union, e per axis from F(max) - origin, floor / ceil of (x - origin) / 2^e
                 clamped to 0 ... 255, inner meta (1 << 5) | (24 + s) with the imask bit, leaf meta (unary count << 5) | first
                 triangle of the leaf within the node, records e2, e1, v0 | primitive
  numbering      nodes breadth first, a node's inner children consecutive in slot order, triangle rows in the same node order;
                 childBase = 0 without inner children, triBase = 0 without leaf children

Areas and costs that are NaN or infinite (extents whose products overflow float32 AND a zero extent beside them) are outside the
rule; none of the tests' inputs has one."""
import bisect

import numpy as np

from refit_ref import F, clamp_byte, exponent

INF = float("inf")
PARTS = (("origin", 0, 12), ("exponents", 12, 15), ("imask", 15, 16), ("bases", 16, 24), ("meta", 24, 32), ("low bytes", 32, 56), ("high bytes", 56, 80))


def morton_keys(c):
    """c: (n, 3) float32 centroids.  The 63-bit keys as Python ints."""
    lo, hi = c.min(axis=0), c.max(axis=0)
    q = np.zeros(c.shape, np.int64)
    for a in range(3):
        ext = F(hi[a] - lo[a])
        if ext > 0:
            t = (c[:, a] - lo[a]) / ext                                     # float32 - float32, float32 / float32
            t = np.minimum(np.maximum(t, F(0)), F(1))
            q[:, a] = np.minimum((t * F(2097152.0)).astype(np.int64), 2097151)
    keys = np.zeros(c.shape[0], np.uint64)
    for b in range(21):
        for a, shift in ((0, 2), (1, 1), (2, 0)):
            keys |= (((q[:, a] >> b) & 1).astype(np.uint64)) << np.uint64(3 * b + shift)
    return [int(k) for k in keys]


def split(keys, a, b):
    """Last position of the left part of [a, b] (a < b)."""
    if keys[a] != keys[b]:
        bit = (keys[a] ^ keys[b]).bit_length() - 1
        return bisect.bisect_left(keys, ((keys[a] >> bit) | 1) << bit, a, b + 1) - 1     # the first key with that bit set, minus one
    bit = (a ^ b).bit_length() - 1
    return ((b >> bit) << bit) - 1


def build(vertices):
    """vertices: (3 * triangles, 4) float32.  Returns (nodes, tris) as flat uint8 arrays, origins with +0.0 for any zero."""
    v = np.ascontiguousarray(vertices, dtype=np.float32)[:, :3].reshape(-1, 3, 3)
    n = v.shape[0]
    assert n >= 1
    with np.errstate(over="ignore", invalid="ignore"):
        return _build(v, n)


def _build(v, n):
    tmn, tmx = v.min(axis=1), v.max(axis=1)
    centroid = F(0.5) * (tmn + tmx)
    keys = morton_keys(centroid)
    order = sorted(range(n), key=keys.__getitem__)                          # sorted() is stable
    keys = [keys[p] for p in order]
    smn, smx = tmn[order], tmx[order]                                       # boxes by sorted position
    # ---- binary tree.  A reference is a node index >= 0, or ~position for one triangle.
    left, right, first, last = [], [], [], []
    bmn, bmx = np.zeros((max(n - 1, 1), 3), np.float32), np.zeros((max(n - 1, 1), 3), np.float32)

    def box(ref):
        return (smn[~ref], smx[~ref]) if ref < 0 else (bmn[ref], bmx[ref])

    def count(ref):
        return 1 if ref < 0 else last[ref] - first[ref] + 1

    def make(a, b):
        if a == b:
            return ~a
        k = len(left)
        left.append(None), right.append(None), first.append(a), last.append(b)
        g = split(keys, a, b)
        left[k], right[k] = make(a, g), make(g + 1, b)
        (lmn, lmx), (rmn, rmx) = box(left[k]), box(right[k])
        bmn[k], bmx[k] = np.minimum(lmn, rmn), np.maximum(lmx, rmx)        # selections
        return k

    root = make(0, n - 1)
    ext = bmx - bmn
    area = (ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2]) + ext[:, 2] * ext[:, 0]
    sign = np.array([[-1.0 if s & 4 else 1.0, -1.0 if s & 2 else 1.0, -1.0 if s & 1 else 1.0] for s in range(8)], np.float32)
    # ---- wide nodes, breadth first
    wide = [root]                                                           # the binary reference each wide node is made from
    rows_n, rows_t = [], []
    tri_rows = 0
    w = 0
    while w < len(wide):
        r = wide[w]
        w += 1
        child = [r] if count(r) <= 3 else [left[r], right[r]]
        while len(child) < 8:
            best, best_area = -1, None
            for i, c in enumerate(child):
                if count(c) <= 3:
                    continue
                if best < 0 or float(area[c]) > best_area:
                    best, best_area = i, float(area[c])
            if best < 0:
                break
            c = child[best]
            child[best] = left[c]
            child.append(right[c])
        cmn = np.array([box(c)[0] for c in child], np.float32)
        cmx = np.array([box(c)[1] for c in child], np.float32)
        nmn, nmx = cmn.min(axis=0), cmx.max(axis=0)
        centre = (F(0.5) * (cmn + cmx)) - (F(0.5) * (nmn + nmx))            # (count, 3)
        cost = (centre[None, :, 0] * sign[:, None, 0] + centre[None, :, 1] * sign[:, None, 1]) + centre[None, :, 2] * sign[:, None, 2]
        cost = cost.astype(np.float64).tolist()                             # [slot][child], exact
        child_of, slot_of = [-1] * 8, [-1] * len(child)
        for _ in range(len(child)):
            best, bs, bi = INF, -1, -1
            for s in range(8):
                if child_of[s] >= 0:
                    continue
                for i in range(len(child)):
                    if slot_of[i] < 0 and cost[s][i] < best:
                        best, bs, bi = cost[s][i], s, i
            if bs < 0:
                bi, bs = slot_of.index(-1), child_of.index(-1)
            child_of[bs], slot_of[bi] = bi, bs
        # ---- encode
        node = np.zeros(80, np.uint8)
        lo = nmn + F(0.0)                                                   # -0.0 + 0.0 = +0.0: which zero a min returns is not part of the rule
        node[0:12] = lo.view(np.uint8)
        e = [exponent(F(nmx[a]) - F(nmn[a])) for a in range(3)]
        node[12:15] = [x & 255 for x in e]
        inner = [s for s in range(8) if child_of[s] >= 0 and count(child[child_of[s]]) > 3]
        leaves = [s for s in range(8) if child_of[s] >= 0 and count(child[child_of[s]]) <= 3]
        child_base = len(wide) if inner else 0
        tri_base = tri_rows if leaves else 0
        node[16:24] = np.array([child_base, tri_base], np.uint32).view(np.uint8)
        seen = 0
        for s in range(8):
            i = child_of[s]
            if i < 0:
                continue
            for a in range(3):
                cell = F(2.0 ** e[a])
                node[32 + 8 * a + s] = clamp_byte(np.floor((cmn[i, a] - nmn[a]) / cell))
                node[56 + 8 * a + s] = clamp_byte(np.ceil((cmx[i, a] - nmn[a]) / cell))
            c = child[i]
            if count(c) > 3:
                node[15] |= 1 << s
                node[24 + s] = (1 << 5) | (24 + s)
                wide.append(c)
            else:
                k = count(c)
                node[24 + s] = (((1 << k) - 1) << 5) | seen
                p0 = ~c if c < 0 else first[c]
                for p in range(p0, p0 + k):
                    prim = order[p]
                    rec = np.zeros(12, np.float32)
                    rec[0:3] = v[prim, 2] - v[prim, 0]
                    rec[4:7] = v[prim, 1] - v[prim, 0]
                    rec[8:11] = v[prim, 0]
                    rec.view(np.uint32)[11] = prim
                    rows_t.append(rec)
                seen += k
        tri_rows += 3 * seen
        rows_n.append(node)
    return np.concatenate(rows_n), np.concatenate(rows_t).view(np.uint8)


def positive_zero_origins(nodes):
    """A copy of nodes with every origin component -0.0 replaced by +0.0."""
    out = np.array(nodes, dtype=np.uint8, copy=True).reshape(-1, 80)
    lo = out[:, 0:12].copy().view(np.uint32)
    lo[lo == 0x80000000] = 0
    out[:, 0:12] = lo.view(np.uint8)
    return out.reshape(-1)


def _inner_slots(meta):
    return (meta & 0x1F) >= 24


def _leaf_triangles(meta):
    """Triangles per slot for leaf slots, 0 elsewhere: the popcount of the unary count."""
    unary = (meta >> 5).astype(np.int64)
    return np.where(_inner_slots(meta) | (meta == 0), 0, (unary & 1) + ((unary >> 1) & 1) + ((unary >> 2) & 1))


def levels_of(nodes):
    """Breadth-first levels from node 0: a list of arrays of node indices, each node's inner children in slot order."""
    n = np.asarray(nodes, np.uint8).reshape(-1, 80)
    child_base = n[:, 16:20].copy().view(np.uint32)[:, 0].astype(np.int64)
    inner = _inner_slots(n[:, 24:32]).sum(axis=1)
    out, level, seen = [], np.array([0], np.int64), 0
    while level.size:
        out.append(level)
        seen += level.size
        assert seen <= n.shape[0], "the tree has a cycle or a shared child"
        k = inner[level]
        start = np.repeat(child_base[level], k)
        rank = np.arange(k.sum()) - np.repeat(np.cumsum(k) - k, k)
        level = start + rank
        assert ((level >= 0) & (level < n.shape[0])).all(), "child index outside the node array"
    return out


def canonical(nodes, tris):
    """The same tree numbered by the rule: nodes breadth first from node 0 with each node's inner children in slot order, every
    node's triangle rows in that node order, childBase / triBase rewritten, origins -0.0 -> +0.0.  Nothing else changes."""
    n = positive_zero_origins(nodes).reshape(-1, 80)
    t = np.asarray(tris, np.uint8).reshape(-1, 16)
    order = np.concatenate(levels_of(n))
    assert order.size == n.shape[0] and np.array_equal(np.sort(order), np.arange(n.shape[0])), "not every node is reached exactly once"
    out = n[order].copy()
    words = out[:, 16:24].copy().view(np.uint32).astype(np.int64)          # childBase, triBase of the reordered nodes
    inner = _inner_slots(out[:, 24:32]).sum(axis=1)
    rows = 3 * _leaf_triangles(out[:, 24:32]).sum(axis=1)
    new_child = np.where(inner > 0, 1 + np.cumsum(inner) - inner, 0)
    new_tri = np.where(rows > 0, np.cumsum(rows) - rows, 0)
    src = np.repeat(words[:, 1], rows) + np.arange(rows.sum()) - np.repeat(np.cumsum(rows) - rows, rows)
    assert src.size == t.shape[0], "the nodes' leaves do not hold every triangle row"
    out[:, 16:24] = np.stack([new_child, new_tri], axis=1).astype(np.uint32).view(np.uint8)
    return out.reshape(-1), t[src].reshape(-1).copy()


def check_structure(nodes, tris, ntri):
    """What every tree of the builder must satisfy, whatever its boxes (vectorised: it also runs on the 250k-triangle tree)."""
    n = np.asarray(nodes, np.uint8).reshape(-1, 80)
    t = np.frombuffer(np.asarray(tris, np.uint8).tobytes(), np.uint32).reshape(-1, 4)
    count = n.shape[0]
    assert count >= 1 and t.shape[0] == 3 * ntri
    meta, imask = n[:, 24:32], n[:, 15]
    tri_base = n[:, 20:24].copy().view(np.uint32)[:, 0].astype(np.int64)
    empty, inner = meta == 0, _inner_slots(meta)
    leaf = ~empty & ~inner
    slot = np.arange(8, dtype=np.uint8)[None, :]
    # inner slots: the meta byte is exactly (1 << 5) | (24 + s), and imask is exactly their set
    assert np.array_equal(meta[inner], np.broadcast_to((1 << 5) | (24 + slot), meta.shape)[inner])
    assert np.array_equal(imask, (inner.astype(np.uint8) << slot).sum(axis=1).astype(np.uint8))
    # leaf slots: unary count 1, 3 or 7, offset below 24
    assert np.isin(meta[leaf] >> 5, (1, 3, 7)).all() and ((meta[leaf] & 0x1F) < 24).all()
    # every node but the root is the child of exactly one slot, all are reached from the root, the levels are contiguous
    levels = levels_of(n)
    children = np.concatenate(levels[1:]) if len(levels) > 1 else np.zeros(0, np.int64)
    assert inner.sum() == count - 1 and np.array_equal(np.sort(children), np.arange(1, count))
    end = 0
    for level in levels:
        assert np.array_equal(np.sort(level), np.arange(end, end + level.size)), "a level is not a contiguous run of nodes"
        end += level.size
    assert end == count
    # leaf row ranges: disjoint, inside [0, 3 * ntri), covering it
    tcount = _leaf_triangles(meta)
    start = (tri_base[:, None] + 3 * (meta & 0x1F).astype(np.int64))[leaf]
    length = 3 * tcount[leaf]
    by_start = np.argsort(start, kind="stable")
    start, length = start[by_start], length[by_start]
    assert start.size and start[0] == 0 and np.array_equal(start[1:], (start + length)[:-1]) and start[-1] + length[-1] == 3 * ntri
    # triangle records: each primitive once, w of the two edge rows 0
    assert np.array_equal(np.sort(t[2::3, 3]), np.arange(ntri, dtype=np.uint32))
    assert not t[0::3, 3].any() and not t[1::3, 3].any()
    # the quantised bytes of empty slots are 0
    assert not n[:, 32:80].reshape(count, 6, 8)[np.broadcast_to(empty[:, None, :], (count, 6, 8))].any()


def first_difference(got_nodes, want_nodes):
    """None for equal node arrays; otherwise a sentence naming the first differing node, its level and the parts that differ."""
    g, w = (np.asarray(a, np.uint8).reshape(-1, 80) for a in (got_nodes, want_nodes))
    if g.shape != w.shape:
        return f"{g.shape[0]} nodes, the rule gives {w.shape[0]}"
    bad = np.nonzero((g != w).any(axis=1))[0]
    if bad.size == 0:
        return None
    k = int(bad[0])
    level = next(i for i, lv in enumerate(levels_of(w)) if k in lv)
    parts = [name for name, a, b in PARTS if not np.array_equal(g[k, a:b], w[k, a:b])]
    return (f"{bad.size} of {g.shape[0]} nodes differ; the first is node {k} on level {level}: {', '.join(parts)} differ\n"
            f"  got  {g[k].tobytes().hex()}\n  want {w[k].tobytes().hex()}")
