"""tests/lbvh_ref.py, the restated rule of the device CWBVH builder, checked on its own (no GPU): its trees are well formed, are
numbered as canonical() numbers them, are fixed points of the refit rule (refit_ref.py and the host C++ refit), have boxes that
contain their triangles in exact arithmetic, and give the hits of BuildBVH's tree.  tests/test_bvh_builder_gpu.py then holds
PTBuildBVHDevice's bytes against these trees."""
import os

import numpy as np
import pytest

import lbvh_ref
import refit_ref
from test_refit import GOLDEN, _rays, _scene_of, soup
from unity_webgpu_pathtracer_amd import plugin

SOUPS = [1, 2, 3, 4, 5, 9, 33, 63, 64, 65, 255, 256, 257, 1000, 5000]      # 63 ... 65, 255 ... 257: a wave / a 256-thread block partly empty


def _degenerate():
    """The five arrays of test_refit.py::test_degenerate_input."""
    rng = np.random.RandomState(8)
    base = soup(40, 5)
    point = np.zeros_like(base)
    point[:, :3] = (0.25, -1.5, 3.0)
    flat = base.copy()
    flat[:, 1] = 0.75
    huge, tiny = base.copy(), base.copy()
    huge[:, :3] *= np.float32(1e30)
    tiny[:, :3] *= np.float32(1e-30)
    zeros = base.copy()
    zeros[:, 2] = np.where(rng.rand(zeros.shape[0]) < 0.5, np.float32(-0.0), np.float32(0.0))
    zeros[::7, 0] = -0.0
    return [("point", point), ("flat", flat), ("1e30", huge), ("1e-30", tiny), ("signed-zeros", zeros)]


def cases():
    for n in SOUPS:
        yield f"soup{n}", soup(n, 100 + n)
    for name in ("cwbvh_identical20", "cwbvh_flat_grid72", "cwbvh_cornell"):
        yield name, np.ascontiguousarray(np.load(os.path.join(GOLDEN, name + ".npz"))["vertices"], np.float32)
    same = np.zeros((900, 4), np.float32)                                   # 300 identical triangles: equal keys, the positions split
    same[:, :3] = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (300, 1))
    yield "identical300", same
    rng = np.random.RandomState(21)
    line = np.zeros((300, 4), np.float32)                                   # 100 triangles, every centroid on the line x = y = z
    tri = np.array([[-1, 0, 1], [0, 1, -1], [1, -1, 0]], np.float32) * 0.0625       # box centre = its own origin, exactly
    step = (rng.randint(-512, 512, 100) / 64.0).astype(np.float32)          # multiples of 2^-6: every sum below is exact
    line[:, :3] = (step[:, None, None] + tri[None]).reshape(-1, 3)
    yield "line100", line
    yield from _degenerate()


CASES = list(cases())
IDS = [c[0] for c in CASES]
_restated = {}


def restated(name, v):
    """lbvh_ref.build(v), computed once per input and shared (read only)."""
    if name not in _restated:
        nodes, tris = lbvh_ref.build(v)
        nodes.setflags(write=False), tris.setflags(write=False)
        _restated[name] = (nodes, tris)
    return _restated[name]


@pytest.mark.parametrize("name,v", CASES, ids=IDS)
def test_restated_tree(name, v):
    nodes, tris = restated(name, v)
    ntri = v.shape[0] // 3
    lbvh_ref.check_structure(nodes, tris, ntri)
    cn, ct = lbvh_ref.canonical(nodes, tris)
    assert np.array_equal(cn, nodes) and np.array_equal(ct, tris)          # already numbered by the rule
    # a fixed point of the refit rule: restated, and the host's C++ (origin zero signs aside: the refit's min may return -0.0)
    for label, (rn, rt) in (("refit_ref", refit_ref.refit(nodes, tris, v)), ("host refit", plugin.refit_cwbvh((nodes, tris), v))):
        assert np.array_equal(rt, tris), (name, label)
        assert lbvh_ref.first_difference(lbvh_ref.positive_zero_origins(rn), nodes) is None, (name, label, lbvh_ref.first_difference(lbvh_ref.positive_zero_origins(rn), nodes))
    assert refit_ref.decoded_boxes_contain(nodes, tris, v) >= (ntri + 2) // 3


def test_centroids_on_a_line_and_equal_keys():
    """The two inputs made for the key: line100's centroids really lie on x = y = z (so the three axes quantise alike and every
    key has its bits in equal triples), identical300's keys are all 0."""
    by_name = dict(CASES)
    v = by_name["line100"][:, :3].reshape(-1, 3, 3)
    c = np.float32(0.5) * (v.min(axis=1) + v.max(axis=1))
    assert (c[:, 0] == c[:, 1]).all() and (c[:, 1] == c[:, 2]).all() and np.unique(c[:, 0]).size > 50
    for k in lbvh_ref.morton_keys(c):
        assert all(((k >> (3 * b)) & 7) in (0, 7) for b in range(21))
    v = by_name["identical300"][:, :3].reshape(-1, 3, 3)
    assert not any(lbvh_ref.morton_keys(np.float32(0.5) * (v.min(axis=1) + v.max(axis=1))))


def test_key_bit_order():
    """x is the most significant of each bit triple, 21 bits per axis, the top cell is clamped."""
    c = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5], [2.0 ** -21, 0, 0]], np.float32)
    k = lbvh_ref.morton_keys(c)
    top = (1 << 21) - 1
    spread = sum(((top >> b) & 1) << (3 * b) for b in range(21))
    assert k[0] == 0 and k[1] == spread << 2 and k[2] == spread << 1 and k[3] == spread
    assert k[4] == 7 << 60 and k[5] == 1 << 2


def test_split():
    keys = [0b000, 0b001, 0b100, 0b101, 0b101, 0b101, 0b111]
    assert lbvh_ref.split(keys, 0, 6) == 1 and lbvh_ref.split(keys, 2, 6) == 5 and lbvh_ref.split(keys, 2, 5) == 2
    assert lbvh_ref.split(keys, 3, 5) == 3 and lbvh_ref.split(keys, 4, 5) == 4          # equal keys: positions 3 | 4 5, then 4 | 5
    assert lbvh_ref.split([0] * 300, 0, 299) == 255 and lbvh_ref.split([0] * 300, 256, 299) == 287


def _shuffled(nodes, tris, seed):
    """The same tree with the nodes permuted within each level and the nodes' triangle blocks permuted, bases fixed up."""
    rng = np.random.RandomState(seed)
    n = np.array(nodes, np.uint8).reshape(-1, 80)
    t = np.asarray(tris, np.uint8).reshape(-1, 16)
    words = n[:, 16:24].copy().view(np.uint32).astype(np.int64)
    meta = n[:, 24:32]
    inner = ((meta & 0x1F) >= 24).sum(axis=1)
    rows = 3 * np.array([sum(bin(int(m) >> 5).count("1") for m in row if m and (m & 0x1F) < 24) for row in meta])
    new_of = np.arange(n.shape[0])                                          # old node index -> new node index
    for level in lbvh_ref.levels_of(n)[1:]:
        # sibling groups stay consecutive and in slot order (childBase + rank addresses them); the groups trade places
        parents = [p for p in range(n.shape[0]) if inner[p] and level[0] <= words[p, 0] <= level[-1]]
        groups = [np.arange(words[p, 0], words[p, 0] + inner[p]) for p in parents]
        at = int(level[0])
        for g in rng.permutation(len(groups)):
            new_of[groups[g]] = np.arange(at, at + groups[g].size)
            at += groups[g].size
    out = np.zeros_like(n)
    out[new_of] = n
    out_words = np.zeros_like(words)
    out_words[new_of] = words
    has = out_words[:, 0] > 0
    out_words[has, 0] = new_of[out_words[has, 0]]                           # childBase: where the first child went
    # triangle blocks: one per node with leaves, in a random order
    out_t = np.zeros_like(t)
    at = 0
    for k in rng.permutation(n.shape[0]):
        r = int(rows[k])
        if r:
            out_t[at:at + r] = t[words[k, 1]:words[k, 1] + r]
            out_words[new_of[k], 1] = at
            at += r
    out[:, 16:24] = out_words.astype(np.uint32).view(np.uint8)
    return out.reshape(-1), out_t.reshape(-1)


@pytest.mark.parametrize("name", ["soup33", "soup257", "soup5000", "cwbvh_cornell", "signed-zeros"])
def test_canonical_undoes_a_renumbering(name):
    v = dict(CASES)[name]
    nodes, tris = restated(name, v)
    sn, st = _shuffled(nodes, tris, seed=len(name))
    if nodes.size > 50 * 80:
        assert not np.array_equal(sn, nodes) and not np.array_equal(st, tris)
    lbvh_ref.check_structure(sn, st, v.shape[0] // 3)                       # still a well-formed tree
    cn, ct = lbvh_ref.canonical(sn, st)
    assert lbvh_ref.first_difference(cn, nodes) is None, lbvh_ref.first_difference(cn, nodes)
    assert np.array_equal(ct, tris)
    # and -0.0 origins become +0.0, nothing else
    neg = np.array(nodes, np.uint8).reshape(-1, 80)
    lo = neg[:, 0:12].copy().view(np.uint32)
    zeros = lo == 0
    lo[zeros] = 0x80000000
    neg[:, 0:12] = lo.view(np.uint8)
    cn, _ = lbvh_ref.canonical(neg.reshape(-1), tris)
    assert np.array_equal(cn, nodes)
    if name == "signed-zeros":
        assert zeros.any()


def test_check_structure_refuses_broken_trees():
    v = dict(CASES)["soup65"]
    nodes, tris = restated("soup65", v)
    n = np.array(nodes, np.uint8).reshape(-1, 80)
    inner_slot = int(np.nonzero((n[0, 24:32] & 0x1F) >= 24)[0][0])
    leaf_node, leaf_slot = (int(x[0]) for x in np.nonzero((n[:, 24:32] != 0) & ((n[:, 24:32] & 0x1F) < 24)))
    empty_node, empty_slot = (int(x[0]) for x in np.nonzero(n[:, 24:32] == 0))

    def broken(edit_nodes=None, edit_tris=None):
        bn, bt = n.copy(), np.array(tris, np.uint8)
        if edit_nodes:
            edit_nodes(bn)
        if edit_tris:
            edit_tris(bt.view(np.uint32).reshape(-1, 4))
        with pytest.raises(AssertionError):
            lbvh_ref.check_structure(bn.reshape(-1), bt, 65)

    def set_byte(node, byte, value):
        def edit(bn):
            bn[node, byte] = value
        return edit

    lbvh_ref.check_structure(nodes, tris, 65)
    broken(set_byte(0, 15, n[0, 15] ^ (1 << inner_slot)))                   # imask without one of its inner slots
    broken(set_byte(0, 24 + inner_slot, (1 << 5) | (24 + (inner_slot ^ 1))))     # inner meta naming another slot
    broken(set_byte(0, 24 + inner_slot, (3 << 5) | (24 + inner_slot)))      # inner meta with another count
    broken(set_byte(leaf_node, 24 + leaf_slot, (5 << 5) | (n[leaf_node, 24 + leaf_slot] & 0x1F)))      # unary count 5
    broken(set_byte(leaf_node, 24 + leaf_slot, n[leaf_node, 24 + leaf_slot] + 1))                      # leaf rows shifted: overlap / gap
    broken(set_byte(0, 16, n[0, 16] + 1))                                   # childBase off by one: node 1 nobody's child, a level not contiguous
    broken(set_byte(empty_node, 56 + empty_slot, 1))                        # a quantised byte in an empty slot

    def dup_prim(t):
        t[2, 3] = t[5, 3]
    broken(edit_tris=dup_prim)

    def w_set(t):
        t[1, 3] = 1
    broken(edit_tris=w_set)
    with pytest.raises(AssertionError):
        lbvh_ref.check_structure(nodes, tris[:-48], 65)


@pytest.mark.parametrize("ntri,seed", [(300, 400), (5000, 5100)])
def test_hits_equal_buildbvh_tree(oracle, ntri, seed):
    """oracle.trace over the restated tree and over BuildBVH's tree of the same soup: the project's bar for two different trees
    over one soup (test_refit.py::test_hits_on_cornell, test_bvh_builder_gpu.py)."""
    v = soup(ntri, seed)
    s = _scene_of(v)
    nrays = 4096
    rays = _rays(v, nrays, seed + 2)
    t_ref, p_ref, _ = oracle.trace(oracle.SceneBuffers(s, *plugin.build_cwbvh(v)), rays)
    t_own, p_own, steps = oracle.trace(oracle.SceneBuffers(s, *lbvh_ref.build(v)), rays)
    assert (p_ref != 0xFFFFFFFF).sum() > nrays // 10
    tdiff = int((t_ref.view(np.uint32) != t_own.view(np.uint32)).sum())
    differ = int(((t_ref.view(np.uint32) != t_own.view(np.uint32)) | (p_ref != p_own)).sum())
    print(f"[lbvh_ref] soup {ntri}: {differ} of {nrays} rays answered by a different primitive, {tdiff} with another t")
    assert tdiff <= max(2, nrays // 2000) and differ <= nrays // 50


def test_device_builder_looks_at_the_vertices_first():
    """PTBuildBVHDevice refuses a non-finite vertex on the host, before it asks for a device: so this holds without a GPU too."""
    import ctypes as C
    lib = plugin.load_library()
    v = soup(9, 1)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[13, 1] = bad
        assert lib.PTBuildBVHDevice(0, w.ctypes.data_as(C.c_void_p), 9) == -1
        assert b"vertex 13 is not finite" in lib.PTGetBVHBuildError()
    w = v.copy()
    w[13, 3] = np.nan                                                       # the fourth component is not a coordinate
    assert lib.PTBuildBVHDevice(-1, w.ctypes.data_as(C.c_void_p), 9) == -1 and b"device" in lib.PTGetBVHBuildError()
