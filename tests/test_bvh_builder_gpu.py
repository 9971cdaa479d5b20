"""PTBuildBVHDevice: the CWBVH builder that runs on the MI355X (csrc/bvh_builder_gpu.hip: LBVH -> 8-wide collapse -> CWBVH
encode in HIP kernels).  It sits beside BuildBVH, whose bytes must equal the reference plugin's; this one
builds a different tree in the same format.  Its own bar: after renumbering (the kernels claim node and triangle storage with
atomicAdd) the bytes equal tests/lbvh_ref.py, the builder's rule restated in numpy float32.  Beside that, HIT
equality: every ray finds the same closest hit (bit-identical t, same primitive unless another triangle yields the very same
t) as in the reference-built tree, the structure passes PTSetScene's index validation, and a frame rendered on the GPU over
the device-built tree equals the oracle's render over the same bytes bit for bit."""
import ctypes as C

import numpy as np
import pytest

import lbvh_ref
from lbvh_ref import check_structure
from test_lbvh_ref import CASES, IDS, restated
from test_refit import soup
from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import BVHScene, PathTracer

pytestmark = pytest.mark.gpu


def _rays(scene, n, seed):
    rng = np.random.RandomState(seed)
    v = scene.vertices[:, :3]
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    o = (lo - 0.2 * ext + rng.rand(n, 3) * 1.4 * ext).astype(np.float32)
    target = (lo + rng.rand(n, 3) * ext).astype(np.float32)
    d = target - o
    d = (d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    rays = np.zeros(n, dtype=[("origin", "<f4", 3), ("direction", "<f4", 3), ("tmax", "<f4"), ("kind", "<f4")])
    rays["origin"], rays["direction"], rays["tmax"] = o, d, 1e5
    return rays


@pytest.mark.parametrize("name,kw,nrays", [
    ("cornell", {}, 4000), ("zoo", {}, 20000), ("sponza", {"tex_size": 4, "detail": 0.15}, 20000), ("bunny", {}, 20000),
])
def test_device_built_tree_gives_the_same_hits(oracle, name, kw, nrays):
    s = scenes.make_scene(name, **kw)
    ref_nodes, ref_tris = plugin.build_cwbvh(s.vertices)
    tm = {}
    dev_nodes, dev_tris = plugin.build_cwbvh(s.vertices, device=0, timing=tm)
    print(f"[gpu builder] {name}: {s.tri_count} triangles, {dev_nodes.nbytes // 80} nodes (reference tree: {ref_nodes.nbytes // 80}), device build {tm['build_ms']:.2f} ms")
    check_structure(dev_nodes, dev_tris, s.tri_count)
    rays = _rays(s, nrays, seed=11)
    t_ref, p_ref, _ = oracle.trace(oracle.SceneBuffers(s, ref_nodes, ref_tris), rays)
    t_dev, p_dev, _ = oracle.trace(oracle.SceneBuffers(s, dev_nodes, dev_tris), rays)
    assert (p_ref != 0xFFFFFFFF).sum() > nrays // 10
    # Same closest hit.  Two trees cannot agree on MORE than the traversal's own arithmetic defines: where a ray passes through an
    # edge shared by two triangles both are hit, at distances equal or one ulp apart, and a hit that lies exactly on a face of a
    # (quantised, but here grid-aligned) child box can be culled by the rounding of the slab test once the other triangle has
    # shrunk tmax -- in either tree (util/bvh.hlsl:77-124 has no epsilon).  So: bit-identical (t, primitive) for all but a
    # handful of rays, and for those the other tree's answer must be a genuine hit of that very ray within 2 ulp of t.
    differ = np.nonzero((t_ref.view(np.uint32) != t_dev.view(np.uint32)) | (p_ref != p_dev))[0]
    tdiff = np.nonzero(t_ref.view(np.uint32) != t_dev.view(np.uint32))[0]
    print(f"[gpu builder] {name}: {len(differ)} of {nrays} rays answered by a different (tied) primitive, {len(tdiff)} of them with t one or two ulp apart")
    assert len(tdiff) <= max(2, nrays // 2000) and len(differ) <= nrays // 50     # coincident (z-fighting) faces of the procedural scenes tie exactly
    for k in list(tdiff) + list(differ[:40]):
        assert p_dev[k] != 0xFFFFFFFF and p_ref[k] != 0xFFFFFFFF
        assert abs(int(t_ref[k:k + 1].view(np.uint32)[0]) - int(t_dev[k:k + 1].view(np.uint32)[0])) <= 2, (k, t_ref[k], t_dev[k])
        one = scenes.Scene("one", s.vertices[int(p_dev[k]) * 3:int(p_dev[k]) * 3 + 3], s.tri_attrs[:1], s.materials, s.lights, s.texture_data, s.camera)
        n1, t1 = plugin.build_cwbvh(one.vertices)
        tt, _, _ = oracle.trace(oracle.SceneBuffers(one, n1, t1), rays[k:k + 1])
        assert tt[0] == t_dev[k]                                            # the device tree's primitive really is hit at that t


def test_tiny_and_degenerate_inputs(oracle):
    lib = plugin.load_library()
    rng = np.random.RandomState(3)
    for ntri in (1, 2, 3, 4, 5, 9, 33):
        v = np.zeros((ntri * 3, 4), np.float32)
        v[:, :3] = rng.uniform(-2, 2, (ntri, 1, 3)).repeat(3, axis=1).reshape(-1, 3) + rng.normal(0, 0.5, (ntri * 3, 3))
        nodes, tris = plugin.build_cwbvh(v, device=0)
        check_structure(nodes, tris, ntri)
    dup = np.zeros((60, 4), np.float32)                                     # twenty identical triangles: equal Morton codes
    dup[:, :3] = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (20, 1))
    nodes, tris = plugin.build_cwbvh(dup, device=0)
    check_structure(nodes, tris, 20)
    flat = np.zeros((12, 4), np.float32)                                    # zero extent on one axis
    flat[:, :2] = rng.rand(12, 2)
    check_structure(*plugin.build_cwbvh(flat, device=0), 4)
    assert lib.PTBuildBVHDevice(0, None, 5) == -1 and lib.PTBuildBVHDevice(0, dup.ctypes.data_as(C.c_void_p), 0) == -1
    assert lib.PTBuildBVHDevice(99, dup.ctypes.data_as(C.c_void_p), 20) == -1 and b"device" in lib.PTGetBVHBuildError()


def _assert_equals_the_rule(name, v, built):
    want_n, want_t = restated(name, v)
    check_structure(*built, v.shape[0] // 3)
    got_n, got_t = lbvh_ref.canonical(*built)
    diff = lbvh_ref.first_difference(got_n, want_n)
    assert diff is None, f"{name}: {diff}"
    bad = np.nonzero((got_t.reshape(-1, 48) != want_t.reshape(-1, 48)).any(axis=1))[0]
    assert bad.size == 0, f"{name}: {bad.size} triangle records differ, the first is record {bad[0]}"


@pytest.mark.parametrize("name,v", CASES, ids=IDS)
def test_device_tree_equals_the_restated_rule(name, v):
    """canonical(PTBuildBVHDevice's tree) == lbvh_ref.build(v), byte for byte: keys, order, splits, greedy expansion, slots,
    quantised boxes, meta bytes and triangle records are all the rule's.  A mismatch names the first node, its level and the
    part that differs: keys / splits / expansion change the bases and meta of a node near the root, the slot assignment
    permutes meta and bytes within a node, the fit or the encode changes origin, exponents or the low / high bytes alone."""
    _assert_equals_the_rule(name, v, plugin.build_cwbvh(v, device=0))


def test_two_builds_are_one_tree():
    name, v = next(c for c in CASES if c[0] == "soup5000")
    a, b = plugin.build_cwbvh(v, device=0), plugin.build_cwbvh(v, device=0)
    print(f"[gpu builder] two builds of {name}: bytes equal before renumbering: nodes {np.array_equal(a[0], b[0])}, triangles {np.array_equal(a[1], b[1])}")
    ca, cb = lbvh_ref.canonical(*a), lbvh_ref.canonical(*b)
    assert lbvh_ref.first_difference(ca[0], cb[0]) is None, lbvh_ref.first_difference(ca[0], cb[0])
    assert np.array_equal(ca[1], cb[1])


def test_non_finite_vertices_are_refused():
    lib = plugin.load_library()
    name, v = "soup300", soup(300, 400)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[3 * 137 + 1, 2] = bad
        assert lib.PTBuildBVHDevice(0, w.ctypes.data_as(C.c_void_p), 300) == -1 and b"finite" in lib.PTGetBVHBuildError()
        _assert_equals_the_rule(name, v, plugin.build_cwbvh(v, device=0))  # the clean soup right after: builds, and to the rule


def test_frame_over_the_device_built_tree_is_bit_exact(oracle):
    """The render kernels take any valid CWBVH: a frame over the device-built tree equals the oracle's render over the same
    bytes bit for bit (all counters too), PTSetScene's validation accepts it, and the image agrees with the frame over the
    reference-built tree (different traversal order, same hits: only exact-tie pixels may differ)."""
    s = scenes.material_zoo()
    pt = PathTracer(s, width=160, height=100, samplesPerPass=3, build_device=0)
    pt.set_stats_level(1)
    p = pt.params(seed=0xB1D)
    pt.render_pass(p)
    gpu = pt.readback()
    ref, st = oracle.render(oracle.buffers_from_bvhscene(pt._bvhScene), p, shadow_any_hit=True)
    assert np.array_equal(gpu.view(np.uint32), ref.view(np.uint32))
    g, r = pt.stats().as_dict(), st.as_dict()
    assert all(g[k] == r[k] for k in g), {k: (g[k], r[k]) for k in g if g[k] != r[k]}
    pt.close()
    sah = PathTracer(s, width=160, height=100, samplesPerPass=3)
    sah.render_pass(p)
    other = sah.readback()
    sah.close()
    same = (other.view(np.uint32) == gpu.view(np.uint32)).all(axis=-1).mean()
    print(f"[gpu builder] frame over device tree vs reference tree: {100 * same:.3f} % of pixels bit-identical")
    assert same > 0.995


def test_build_time_250k_triangles():
    """The Sponza-class soup (250,752 triangles): device build time next to the CPU builder's (DESIGN.md quotes both)."""
    s = scenes.sponza_atrium(tex_size=4)
    cpu, dev = {}, {}
    plugin.build_cwbvh(s.vertices, timing=cpu)
    plugin.build_cwbvh(s.vertices, device=0, timing=dev)                   # first call: module load + allocation warm-up
    n, t = plugin.build_cwbvh(s.vertices, device=0, timing=dev)
    check_structure(n, t, s.tri_count)
    # the large-scale pin: a refit with the vertices it was built from changes no byte (origin zero signs aside), so every box
    # and every triangle record is the encode rule's for this topology
    rn, rt = plugin.refit_cwbvh((n, t), s.vertices)
    assert np.array_equal(rt, t)
    assert lbvh_ref.first_difference(lbvh_ref.positive_zero_origins(rn), lbvh_ref.positive_zero_origins(n)) is None, \
        lbvh_ref.first_difference(lbvh_ref.positive_zero_origins(rn), lbvh_ref.positive_zero_origins(n))
    print(f"[gpu builder] 250k triangles: CPU binned-SAH BuildBVH {cpu['build_ms']:.1f} ms, PTBuildBVHDevice kernels {dev['build_ms']:.2f} ms, {n.nbytes // 80} nodes")
    assert dev["build_ms"] < cpu["build_ms"]
