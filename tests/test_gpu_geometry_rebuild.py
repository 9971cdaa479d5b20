"""Geometry rebuilds and tree quality (PTRebuildGeometry / PTRebuildGeometryDevice / PTMeasureGeometry, include/ptmi_plugin.h
Part 10) on the MI355X.

The rebuilt tree is checked against the builder's restated rule (tests/lbvh_ref.py) byte for byte after renumbering, everything
rendered or queried after a rebuild against a fresh PTSetScene of the arrays PTReadGeometry returns, bit for bit, and the device
measure against the host twin PTMeasureBVHArrays (itself pinned by tests/test_geometry_quality.py)."""
import ctypes as C

import numpy as np
import pytest

import lbvh_ref
from test_gpu_geometry_update import instance_bounds, new_attrs, render, set_arrays, soup_scene, to_device
from test_refit import deformed, soup
from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer

pytestmark = pytest.mark.gpu

W, H = 64, 64
REL = 1e-9
_rule = {}


def rule(key, w):
    """lbvh_ref.build(w), computed once per key"""
    if key not in _rule:
        _rule[key] = lbvh_ref.build(w)
    return _rule[key]


def rule_count(key, w):
    return rule(key, w)[0].size // 80


def assert_rule_tree(nodes, tris, w, want, label):
    """nodes / tris (one BLAS, exactly its K nodes and 3n rows) hold the rule's tree for w, whatever the numbering"""
    n = w.shape[0] // 3
    lbvh_ref.check_structure(nodes, tris, n)
    got_n, got_t = lbvh_ref.canonical(nodes, tris)
    diff = lbvh_ref.first_difference(got_n, want[0])
    assert diff is None, (label, diff)
    assert np.array_equal(got_t, want[1]), label


def blas_slice(pt, mesh, nodes, tris):
    n0, cap, t0, nt = pt._bvhScene.blas_spans[0 if mesh is None else mesh]
    return nodes[n0 * 80:(n0 + cap) * 80], tris[t0 * 16:t0 * 16 + nt * 48]


def assert_rebuilt(pt, mesh, w, want, label, got=None):
    """The BLAS of the current scene: K = PTMeasureGeometry's nodeCount nodes of the rule's tree, zero nodes behind them"""
    nodes, tris, _ = got or pt.read_geometry()
    bn, bt = blas_slice(pt, mesh, nodes, tris)
    q = pt.geometry_quality(mesh)
    K = q["nodeCount"]
    assert K == want[0].size // 80 and q["nodeCapacity"] == bn.size // 80 and q["triangleCount"] == w.shape[0] // 3, (label, q)
    assert_rule_tree(bn[:K * 80], bt, w, want, label)
    assert not bn[K * 80:].any(), label
    return q


def same_quality(got, want):
    for k in ("nodeCount", "triangleCount", "levels"):
        assert got[k] == want[k], (k, got, want)
    for k in ("rootHalfArea", "sahCost"):
        assert abs(got[k] - want[k]) <= REL * abs(want[k]), (k, got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 1. bytes against the restated rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", [1, 2, 3, 4, 9, 64, 300, 2000])
def test_bytes_equal_the_rule(ntri):
    v = soup(ntri, 40 + ntri)
    poses = [v] + [deformed(v, 11 + step) for step in range(3)]
    counts = [rule_count((ntri, k), w) for k, w in enumerate(poses)]
    if ntri == 2000:
        assert counts == [329, 345, 336, 324]
    if ntri == 300:
        assert counts == [54, 53, 47, 53]
    if ntri == 64:
        assert counts == [9, 9, 8, 9]
    pt = PathTracer(soup_scene(v), width=8, height=8, build_device=0, node_capacity=max(counts))
    assert_rebuilt(pt, None, v, rule((ntri, 0), v), (ntri, "built"))
    attrs = pt._bvhScene.tri_attrs
    for step, device in enumerate((False, True, False)):      # three rebuilds: both generations are written, the first one twice
        w = poses[1 + step]
        give_attrs = step != 2
        if give_attrs:
            attrs = new_attrs(attrs, step)
        if device:
            pt.rebuild_geometry(to_device(pt, w), tri_attrs=to_device(pt, attrs) if give_attrs else None)
        else:
            pt.rebuild_geometry(w, tri_attrs=attrs if give_attrs else None)
        got = pt.read_geometry()
        assert_rebuilt(pt, None, w, rule((ntri, 1 + step), w), (ntri, step), got)
        assert np.array_equal(got[2].view(np.uint8), attrs.view(np.uint8)), (ntri, step)
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. capacity
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity():
    v = soup(2000, 2040)
    small, large = deformed(v, 13), deformed(v, 11)
    counts = [rule_count((2000, k), w) for k, w in ((0, v), (3, small), (1, large))]
    assert counts == [329, 324, 345]                          # the preconditions: a changed rule fails here, not below
    s = soup_scene(v)
    pt = PathTracer(s, width=W, height=H, build_device=0)
    assert pt.geometry_quality()["nodeCapacity"] == 329
    pt.rebuild_geometry(small)
    got = pt.read_geometry()
    assert_rebuilt(pt, None, small, rule((2000, 3), small), "324 of 329", got)
    assert not got[0][324 * 80:].any() and got[0].size == 329 * 80
    frame = render(pt, 2)[0]
    for device in (False, True):
        arg = to_device(pt, large) if device else large
        with pytest.raises(plugin.PluginError) as e:
            pt.rebuild_geometry(arg)
        assert e.value.code == abi.PT_ERR_INVALID_ARG and "345" in str(e.value) and "329" in str(e.value), str(e.value)
        after = pt.read_geometry()
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, after)), device
        assert np.array_equal(render(pt, 2)[0].view(np.uint32), frame.view(np.uint32)), device
    pt.update_geometry(v)                                      # a refit after the refusals: of the tree built for `small`
    want = plugin.refit_cwbvh((got[0][:324 * 80], got[1]), v)
    now = pt.read_geometry()
    assert np.array_equal(now[0][:324 * 80], want[0]) and np.array_equal(now[1], want[1]) and not now[0][324 * 80:].any()
    pt.rebuild_geometry(small)
    assert_rebuilt(pt, None, small, rule((2000, 3), small), "rebuild after a refusal")
    pt.close()
    pt = PathTracer(s, width=8, height=8, build_device=0, node_capacity=1.25)
    assert pt.geometry_quality()["nodeCapacity"] == 412
    pt.rebuild_geometry(large)
    assert_rebuilt(pt, None, large, rule((2000, 1), large), "345 of 412")
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a tree from the CPU builder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", [3, 300, 2000])
def test_rebuild_of_a_cpu_built_tree(ntri):
    v = soup(ntri, 40 + ntri)
    w = deformed(v, 11)
    cpu_count = plugin.build_cwbvh(v)[0].size // 80
    pt = PathTracer(soup_scene(v), width=8, height=8, node_capacity=max(cpu_count, rule_count((ntri, 1), w)))
    assert pt.geometry_quality()["nodeCount"] == cpu_count
    pt.rebuild_geometry(w)
    assert_rebuilt(pt, None, w, rule((ntri, 1), w), ntri)
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. frames, counters, queries, guides against a fresh PTSetScene of the arrays PTReadGeometry returns
# ---------------------------------------------------------------------------------------------------------------------
def queries_and_guides_equal(upd, ref):
    rays = np.stack([upd.camera_ray(x, y) for y in range(0, H, 3) for x in range(0, W, 3)])
    h1, s1 = upd.trace_rays(rays, surface=True)
    h2, s2 = ref.trace_rays(rays, surface=True)
    assert (h1.view(np.uint32)[:, 3] != abi.PT_MISS).sum() > rays.shape[0] // 4
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    for pt in (upd, ref):
        pt.render_guides(4)
    for a, b in zip(upd.guides(), ref.guides()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def flat_case(schedule, oracle=None):
    s = scenes.material_zoo()
    w = deformed(s.vertices, 5, amplitude=0.01)
    cap = max(rule_count("zoo", s.vertices), rule_count("zoo-5", w))
    upd = PathTracer(s, width=W, height=H, schedule=schedule, build_device=0, node_capacity=cap)
    ref = PathTracer(s, width=W, height=H, schedule=schedule, build_device=0, node_capacity=cap)
    render(upd, 1)
    upd.rebuild_geometry(w)
    got, gst = render(upd)
    nodes, tris, attrs = upd.read_geometry()
    assert_rebuilt(upd, None, w, rule("zoo-5", w), schedule, (nodes, tris, attrs))
    set_arrays(ref, nodes, tris, attrs)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), schedule
    assert gst == wst, (gst, wst)
    if schedule == 1:
        queries_and_guides_equal(upd, ref)
    if oracle is not None:
        for pt in (upd, ref):
            pt.Reset()
            pt.reset_stats()
        p = upd.params(seed=0xB1D)
        upd.render_pass(p)
        frame, st = oracle.render(oracle.buffers_from_bvhscene(ref._bvhScene), p, shadow_any_hit=True)
        assert np.array_equal(upd.readback(last_output=False).view(np.uint32), frame.view(np.uint32))
        g, r = upd.stats().as_dict(), st.as_dict()
        assert all(g[k] == r[k] for k in g), {k: (g[k], r[k]) for k in g if g[k] != r[k]}
    upd.close()
    ref.close()


def tlas_case(schedule):
    s = scenes.instanced_scene()
    poses = {mesh: deformed(s.vertices[t0 * 3:(t0 + n) * 3], 6 + mesh, amplitude=0.08) for mesh, (t0, n) in enumerate(s.mesh_ranges) if mesh in (0, 2)}
    caps = [max(rule_count(("inst", m), s.vertices[t0 * 3:(t0 + n) * 3]), rule_count(("inst-6", m), poses[m]) if m in poses else 0)
            for m, (t0, n) in enumerate(s.mesh_ranges)]
    upd = PathTracer(s, width=W, height=H, schedule=schedule, build_device=0, node_capacity=caps)
    ref = PathTracer(s, width=W, height=H, schedule=schedule, build_device=0, node_capacity=caps)
    blas = ref._bvhScene.blas_instances
    render(upd, 1)
    for mesh, w in poses.items():
        upd.rebuild_geometry(w, mesh=mesh)                     # resends the instances' bounds
        blas = instance_bounds(ref, s, mesh, w, blas)
    got, gst = render(upd)
    nodes, tris, attrs = upd.read_geometry()
    for mesh, w in poses.items():
        assert_rebuilt(upd, mesh, w, rule(("inst-6", mesh), w), (schedule, mesh), (nodes, tris, attrs))
    set_arrays(ref, nodes, tris, attrs, blas=blas)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), schedule
    assert gst == wst, (gst, wst)
    if schedule == 1:
        queries_and_guides_equal(upd, ref)
    upd.close()
    ref.close()


@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4])
def test_frames_after_rebuild_flat(schedule):
    flat_case(schedule)


@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4])
def test_frames_after_rebuild_tlas(schedule):
    tlas_case(schedule)


def test_frame_after_rebuild_equals_the_oracle(oracle):
    flat_case(None, oracle)


# ---------------------------------------------------------------------------------------------------------------------
# 5. carry-over between the generations, and the plan a rebuild replaces
# ---------------------------------------------------------------------------------------------------------------------
def test_carry_over_and_refit_after_rebuild():
    s = scenes.instanced_scene(count=5, detail=6)
    local = [s.vertices[t0 * 3:(t0 + n) * 3] for t0, n in s.mesh_ranges]
    steps = (("rebuild", 1), ("refit", 0), ("rebuild", 0), ("refit", 1))
    poses = [deformed(local[mesh], 20 + k, amplitude=0.05) for k, (_, mesh) in enumerate(steps)]
    caps = [rule_count(("carry", m), v) for m, v in enumerate(local)]
    for k, (what, mesh) in enumerate(steps):
        if what == "rebuild":
            caps[mesh] = max(caps[mesh], rule_count(("carry-pose", k), poses[k]))
    pt = PathTracer(s, width=8, height=8, build_device=0, node_capacity=caps)
    spans = pt._bvhScene.blas_spans
    count = {m: pt.geometry_quality(m)["nodeCount"] for m in (0, 1)}
    for k, (what, mesh) in enumerate(steps):
        before = pt.read_geometry()
        w = poses[k]
        if what == "rebuild":
            pt.rebuild_geometry(w, mesh=mesh)
        else:
            pt.update_geometry(w, mesh=mesh)
        after = pt.read_geometry()
        for m, (n0, cap, t0, nt) in enumerate(spans):
            if m != mesh:                                      # untouched BLASes: carried over
                assert np.array_equal(after[0][n0 * 80:(n0 + cap) * 80], before[0][n0 * 80:(n0 + cap) * 80]), (k, m)
                assert np.array_equal(after[1][t0 * 16:t0 * 16 + nt * 48], before[1][t0 * 16:t0 * 16 + nt * 48]), (k, m)
        assert np.array_equal(after[2].view(np.uint8), before[2].view(np.uint8)), k
        if what == "rebuild":
            count[mesh] = assert_rebuilt(pt, mesh, w, rule(("carry-pose", k), w), k, after)["nodeCount"]
        else:                                                  # the refit of the tree that was there, a rebuilt one included
            bn, bt = blas_slice(pt, mesh, before[0], before[1])
            K = count[mesh]
            want_n, want_t = plugin.refit_cwbvh((bn[:K * 80], bt), w)
            an, at = blas_slice(pt, mesh, after[0], after[1])
            assert np.array_equal(an[:K * 80], want_n) and np.array_equal(at, want_t) and not an[K * 80:].any(), k
            assert pt.geometry_quality(mesh)["nodeCount"] == K
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. ordering with passes in flight
# ---------------------------------------------------------------------------------------------------------------------
def test_ordering_with_passes_in_flight():
    """Passes enqueued before a rebuild render the old tree, passes after it the new one, with no host synchronisation of the
    passes between.  The reference context rebuilds the same poses itself: two builds of the same vertices may number their
    nodes differently, but they are the same tree and give the same frame."""
    import torch
    s = scenes.material_zoo()
    states = [None, deformed(s.vertices, 21, amplitude=0.01), deformed(s.vertices, 22, amplitude=0.02)]
    cap = max([rule_count("zoo", s.vertices)] + [rule_count(("zoo-order", k), states[k]) for k in (1, 2)])
    ref = PathTracer(s, width=W, height=H, build_device=0, node_capacity=cap)
    statics = []
    for w in states:
        if w is not None:
            ref.rebuild_geometry(w)
        statics.append(render(ref, 1)[0])
    ref.close()
    assert not np.array_equal(statics[0].view(np.uint32), statics[1].view(np.uint32))
    for host in (False, True):
        pt = PathTracer(s, width=W, height=H, build_device=0, node_capacity=cap)
        pt.set_passes_in_flight(12)
        dev = f"cuda:{pt.device}"
        outs = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in states]
        keep = [to_device(pt, w) for w in states[1:]]
        torch.cuda.synchronize()
        p = pt.params(seed=0x51)
        pt.render_pass_to(p, outs[0].data_ptr())
        for k in (1, 2):
            if host:
                w = states[k].copy()
                plugin.check(pt.lib.PTRebuildGeometry(pt.ctx, 0, 0, 0, w.ctypes.data, w.shape[0] // 3, None))
                w[:] = np.nan                                  # the library copied the array before returning
            else:
                pt.rebuild_geometry(keep[k - 1])
            pt.render_pass_to(p, outs[k].data_ptr())
        pt.synchronize()
        torch.cuda.synchronize()
        for k in range(3):
            assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), statics[k].view(np.uint32)), (host, k)
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. quality on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_device():
    v = soup(2000, 2040)
    w = deformed(v, 3, amplitude=0.2)
    cap = max(rule_count((2000, 0), v), rule_count("quality-pose", w))

    def host_twin(pt):
        nodes, tris, _ = pt.read_geometry()
        return plugin.measure_cwbvh((nodes, tris), 2000)

    pt = PathTracer(soup_scene(v), width=8, height=8, build_device=0, node_capacity=cap)
    built = pt.geometry_quality()                              # before any update
    same_quality(built, host_twin(pt))
    assert built["nodeCapacity"] == cap and built["nodeCount"] == 329 and built["sahCost"] > 1.0
    pt.update_geometry(w)
    refit = pt.geometry_quality()
    same_quality(refit, host_twin(pt))
    pt.rebuild_geometry(to_device(pt, w))
    rebuilt = pt.geometry_quality()
    same_quality(rebuilt, host_twin(pt))
    print(f"[rebuild] soup 2000, amplitude 0.2: sahCost built {built['sahCost']:.3f}, refitted {refit['sahCost']:.3f}, rebuilt {rebuilt['sahCost']:.3f}")
    assert rebuilt["sahCost"] < refit["sahCost"]
    pt.close()
    ratio = refit["sahCost"] / built["sahCost"]
    for r, verdict in ((ratio * (1 - 1e-6), "rebuild"), (ratio * (1 + 1e-6), "refit")):
        pt = PathTracer(soup_scene(v), width=8, height=8, build_device=0, node_capacity=cap)
        assert pt.update_geometry(w, rebuild_above=r) == verdict, (r, ratio)
        q = pt.geometry_quality()
        same_quality(q, rebuilt if verdict == "rebuild" else refit)
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = plugin.load_library()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    buf = np.zeros(4096, np.uint8)
    q = abi.geometry_quality()
    for rc in (lib.PTRebuildGeometry(ctx, 0, 0, 0, buf.ctypes.data, 1, None), lib.PTRebuildGeometryDevice(ctx, 0, 0, 0, buf.ctypes.data, 1, None),
               lib.PTMeasureGeometry(ctx, 0, 0, 0, C.byref(q))):
        assert rc == abi.PT_ERR_NO_SCENE
    lib.PTDestroy(ctx)
    v = soup(9, 2)
    flat = PathTracer(soup_scene(v), width=W, height=H, build_device=0, node_capacity=2.0)
    before = flat.read_geometry()
    frame = render(flat, 1)[0]
    p, n = v.ctypes.data, 9
    dv = to_device(flat, v)
    import torch
    torch.cuda.synchronize()

    def unchanged(label):
        after = flat.read_geometry()
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after)), label
        assert np.array_equal(render(flat, 1)[0].view(np.uint32), frame.view(np.uint32)), label

    for fn, ptr in ((lib.PTRebuildGeometry, p), (lib.PTRebuildGeometryDevice, dv.data_ptr())):
        assert fn(None, 0, 0, 0, ptr, n, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 0, 0, 0, None, n, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 0, 0, 0, ptr, 0, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 0, 0, 0, ptr, n - 1, None) == abi.PT_ERR_INVALID_ARG          # count mismatch
        assert fn(flat.ctx, 0, 0, 0, ptr, n + 1, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 1, 0, 0, ptr, n, None) == abi.PT_ERR_INVALID_ARG              # offsets that name no BLAS
        assert fn(flat.ctx, 0, 3, 0, ptr, n, None) == abi.PT_ERR_INVALID_ARG
        assert fn(flat.ctx, 0, 0, -1, ptr, n, None) == abi.PT_ERR_INVALID_ARG
        unchanged(fn)
        assert fn(flat.ctx, 0, 0, 0, ptr, n, None) == abi.PT_OK                           # ... followed by a successful call
        before = flat.read_geometry()
        frame = render(flat, 1)[0]
    assert lib.PTMeasureGeometry(None, 0, 0, 0, C.byref(q)) == abi.PT_ERR_INVALID_ARG
    assert lib.PTMeasureGeometry(flat.ctx, 0, 0, 0, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTMeasureGeometry(flat.ctx, 1, 0, 0, C.byref(q)) == abi.PT_ERR_INVALID_ARG
    unset = abi.PTGeometryQuality()
    assert lib.PTMeasureGeometry(flat.ctx, 0, 0, 0, C.byref(unset)) == abi.PT_ERR_INVALID_ARG and b"structSize" in lib.PTGetLastError()
    for bad in (np.nan, np.inf, -np.inf):
        w = deformed(v, 4)
        w[5, 2] = bad
        assert lib.PTRebuildGeometry(flat.ctx, 0, 0, 0, w.ctypes.data, n, None) == abi.PT_ERR_INVALID_ARG       # the host looks
        assert b"vertex 5 is not finite" in lib.PTGetLastError()
        dw = to_device(flat, w)
        import torch
        torch.cuda.synchronize()
        assert lib.PTRebuildGeometryDevice(flat.ctx, 0, 0, 0, dw.data_ptr(), n, None) == abi.PT_ERR_INVALID_ARG  # the device looks
        assert b"vertex 5 is not finite" in lib.PTGetLastError()
        unchanged(bad)
    attrs = flat._bvhScene.tri_attrs.copy()
    attrs["materialIndex"][3] = flat._bvhScene.materials.shape[0]          # a flat scene indexes the materials with it
    w = deformed(v, 4)
    assert lib.PTRebuildGeometry(flat.ctx, 0, 0, 0, w.ctypes.data, n, attrs.ctypes.data) == abi.PT_ERR_INVALID_ARG
    assert b"materialIndex" in lib.PTGetLastError()
    unchanged("materialIndex")
    flat.rebuild_geometry(w)                                   # ... and the successful calls after the refusals
    assert_rebuilt(flat, None, w, lbvh_ref.build(w), "after the refusals")
    flat.update_geometry(v)
    flat.rebuild_geometry(to_device(flat, v))
    assert_rebuilt(flat, None, v, lbvh_ref.build(v), "device, after the refusals")
    flat.close()
    s = scenes.instanced_scene(count=5, detail=4)
    pt = PathTracer(s, width=8, height=8, build_device=0, node_capacity=2.0)
    gi = pt._bvhScene.gpu_instances
    k = next(i for i, inst in enumerate(s.instances) if inst[0] == 1)
    off = [int(gi[k][f]) for f in ("bvhOffset", "triOffset", "triAttributeOffset")]
    t0, n = s.mesh_ranges[1]
    w = np.ascontiguousarray(s.vertices[t0 * 3:(t0 + n) * 3])
    assert lib.PTRebuildGeometry(pt.ctx, *off, w.ctypes.data, n - 1, None) == abi.PT_ERR_INVALID_ARG         # not the BLAS's count
    assert lib.PTRebuildGeometry(pt.ctx, off[0], off[1], off[2] + 1, w.ctypes.data, n, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTRebuildGeometry(pt.ctx, off[0] + 1, off[1], off[2], w.ctypes.data, n, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTRebuildGeometry(pt.ctx, *off, w.ctypes.data, n, None) == abi.PT_OK
    assert pt.geometry_quality(1)["triangleCount"] == n
    # PTSetScene discards the rebuild state: the scene's own arrays are current again
    pt._bvhScene.PrepareShader(pt.ctx)
    got = pt.read_geometry()
    assert np.array_equal(got[0], pt._bvhScene.bvh_nodes) and np.array_equal(got[1], pt._bvhScene.bvh_tris)
    same_quality(pt.geometry_quality(1), plugin.measure_cwbvh(blas_slice(pt, 1, got[0], got[1]), n))
    pt.close()
