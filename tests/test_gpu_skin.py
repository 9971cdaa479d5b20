"""Skinned geometry (PTSetSkin / PTSkinGeometry / PTSkinGeometryDevice, include/ptmi_plugin.h Part 11) on the MI355X.

The skin kernels are checked against tests/skin_ref.py (the rule restated in numpy float32) byte for byte: after a skin the nodes
and triangle rows equal the host refit of the restated vertices, the attribute records equal the restated records.  Frames, TLAS
and counters are compared with a second context that was given those vertices through PTUpdateGeometry / PTRebuildGeometry."""
import ctypes as C
import warnings

import numpy as np
import pytest

import skin_cases
import skin_ref
from test_gpu_geometry_update import H, W, compose, mesh_slices, render, soup_scene, to_device
from test_refit import deformed, soup
from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer

pytestmark = pytest.mark.gpu

CASES = [(t, j) for t in (1, 2, 3, 21, 22, 85, 86, 300) for j in (1, 64, 1024)] + [(5000, 64)]


def soup_skin(ntri, joint_count, materials):
    rest = soup(ntri, 40 + ntri)
    joints, weights = skin_cases.skin_of(rest, joint_count, 3 * ntri + joint_count)
    return rest, joints, weights, skin_cases.rest_attrs(ntri, ntri + 1, material_count=materials)


def same_bounds(got, verts):
    assert got.shape == (2, 3) and got.dtype == np.float32
    assert np.array_equal(got[0], verts[:, :3].min(axis=0)) and np.array_equal(got[1], verts[:, :3].max(axis=0)), (got, verts[:, :3].min(axis=0), verts[:, :3].max(axis=0))


def assert_skinned(pt, built, want_v, want_a, label):
    want_n, want_t = plugin.refit_cwbvh(built, want_v)
    got_n, got_t, got_a = pt.read_geometry()
    bad = np.nonzero((got_n.reshape(-1, 80) != want_n.reshape(-1, 80)).any(axis=1))[0]
    assert bad.size == 0, (label, bad[:8], got_n.size // 80)
    assert np.array_equal(got_t, want_t), label
    assert got_a.tobytes() == want_a.tobytes(), label


# ---------------------------------------------------------------------------------------------------------------------
# bytes against the restated rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri,joint_count", CASES)
def test_bytes_equal_the_restatement(ntri, joint_count):
    scene = soup_scene(soup(ntri, 40 + ntri))
    rest, joints, weights, attrs = soup_skin(ntri, joint_count, scene.materials.shape[0])
    pt = PathTracer(scene, width=8, height=8)
    built = (pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris)
    pt.set_skin(rest, joints, weights, rest_attrs=attrs, joint_count=joint_count)
    for step in range(3):                                      # three skins: both generations are written, the first one twice
        pal = skin_cases.palette(joint_count, 100 * step + joint_count)
        bounds = pt.skin_geometry(pal.reshape(-1, 3, 4) if step == 1 else pal)
        want_v, want_a, _ = skin_ref.skin(rest, joints, weights, pal, attrs)
        assert_skinned(pt, built, want_v, want_a, (ntri, joint_count, step))
        same_bounds(bounds, want_v)
    # a second PTSetSkin replaces the skin; without rest attributes the records are not touched
    pt.set_skin(rest[::-1].copy(), joints, weights, joint_count=joint_count)
    pal = skin_cases.palette(joint_count, 7)
    bounds = pt.skin_geometry(pal)
    want_v, _, _ = skin_ref.skin(rest[::-1], joints, weights, pal)
    assert_skinned(pt, built, want_v, want_a, (ntri, joint_count, "replaced"))
    same_bounds(bounds, want_v)
    pt.close()


def test_without_rest_attrs_the_attribute_buffer_is_untouched():
    scene = scenes.material_zoo()
    pt = PathTracer(scene, width=8, height=8)
    joints, weights = skin_cases.skin_of(scene.vertices, 16, 1)
    pt.set_skin(scene.vertices, joints, weights, joint_count=16)
    pt.skin_geometry(skin_cases.palette(16, 2, amplitude=0.02))
    assert pt.read_geometry()[2].tobytes() == np.ascontiguousarray(scene.tri_attrs).tobytes()
    pt.close()


def test_device_palette_gives_the_same_bytes():
    import torch
    ntri, J = 300, 64
    scene = soup_scene(soup(ntri, 40 + ntri))
    rest, joints, weights, attrs = soup_skin(ntri, J, scene.materials.shape[0])
    pal = skin_cases.palette(J, 5)
    out = []
    for device in (False, True):
        pt = PathTracer(scene, width=8, height=8)
        pt.set_skin(rest, joints, weights, rest_attrs=attrs, joint_count=J)
        m = torch.from_numpy(pal.reshape(J, 3, 4).copy()).to(f"cuda:{pt.device}") if device else pal
        bounds = pt.skin_geometry(m)
        out.append([a.tobytes() for a in pt.read_geometry()] + [bounds.tobytes()])
        pt.close()
    assert out[0] == out[1]
    want_v, _, _ = skin_ref.skin(rest, joints, weights, pal)
    same_bounds(np.frombuffer(out[1][3], np.float32).reshape(2, 3), want_v)


# ---------------------------------------------------------------------------------------------------------------------
# rebuild
# ---------------------------------------------------------------------------------------------------------------------
def test_rebuild_equals_a_rebuild_of_the_restated_vertices():
    ntri, J = 300, 64
    scene = soup_scene(soup(ntri, 40 + ntri))
    rest, joints, weights, attrs = soup_skin(ntri, J, scene.materials.shape[0])
    pal = skin_cases.palette(J, 9, amplitude=0.3)
    want_v, want_a, _ = skin_ref.skin(rest, joints, weights, pal, attrs)
    upd = PathTracer(scene, width=W, height=H, build_device=0, node_capacity=2.0)
    ref = PathTracer(scene, width=W, height=H, build_device=0, node_capacity=2.0)
    upd.set_skin(rest, joints, weights, rest_attrs=attrs, joint_count=J)
    render(upd, 1)
    bounds = upd.skin_geometry(pal, rebuild=True)
    same_bounds(bounds, want_v)
    ref.rebuild_geometry(want_v, tri_attrs=want_a)
    got, gst = render(upd)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and gst == wst
    qa, qb = upd.geometry_quality(), ref.geometry_quality()
    assert qa["nodeCount"] == qb["nodeCount"] and qa["levels"] == qb["levels"]
    assert abs(qa["sahCost"] - qb["sahCost"]) <= 1e-9 * qb["sahCost"], (qa, qb)
    ga, gb = upd.read_geometry(), ref.read_geometry()
    rows = [sorted(map(bytes, g[1].reshape(-1, 48))) for g in (ga, gb)]       # the records as a multiset: node numbering is the builder's
    assert rows[0] == rows[1]
    assert ga[2].tobytes() == gb[2].tobytes() == want_a.tobytes()
    # the policy of update_geometry(rebuild_above=) on the same bookkeeping
    assert upd.skin_geometry(pal, rebuild_above=1e9)[1] == "refit"
    assert upd.skin_geometry(pal, rebuild_above=0.0)[1] == "rebuild"
    upd.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# frames against a second context given the restated vertices through PTUpdateGeometry
# ---------------------------------------------------------------------------------------------------------------------
def zoo_skin(scene, J=16):
    joints, weights = skin_cases.skin_of(scene.vertices, J, 77)
    return joints, weights


@pytest.mark.parametrize("schedule", [0, 1])
def test_frames_after_skin_flat(schedule):
    s = scenes.material_zoo()
    J = 16
    joints, weights = zoo_skin(s, J)
    pal = skin_cases.palette(J, 3, amplitude=0.02)
    want_v, want_a, _ = skin_ref.skin(s.vertices, joints, weights, pal, s.tri_attrs)
    upd = PathTracer(s, width=W, height=H, schedule=schedule)
    ref = PathTracer(s, width=W, height=H, schedule=schedule)
    upd.set_skin(s.vertices, joints, weights, rest_attrs=s.tri_attrs, joint_count=J)
    render(upd, 1)
    upd.skin_geometry(pal)
    ref.update_geometry(want_v, tri_attrs=want_a)
    got, gst = render(upd)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), schedule
    assert gst == wst, (gst, wst)
    upd.close()
    ref.close()


@pytest.mark.parametrize("schedule", [0, 1])
def test_frames_after_skin_instanced(schedule):
    s = scenes.instanced_scene()
    upd = PathTracer(s, width=W, height=H, schedule=schedule)
    ref = PathTracer(s, width=W, height=H, schedule=schedule)
    render(upd, 1)
    J = 8
    with warnings.catch_warnings():
        warnings.simplefilter("error")                         # no warning: the bounds come back, the TLAS stays exact
        for mesh in (0, 2):
            t0, n = s.mesh_ranges[mesh]
            rest = np.ascontiguousarray(s.vertices[t0 * 3:(t0 + n) * 3])
            attrs = np.ascontiguousarray(s.tri_attrs[t0:t0 + n])
            joints, weights = skin_cases.skin_of(rest, J, 5 + mesh)
            pal = skin_cases.palette(J, 9 + mesh, amplitude=0.1)
            upd.set_skin(rest, joints, weights, mesh=mesh, rest_attrs=attrs, joint_count=J)
            upd.skin_geometry(pal, mesh=mesh)
            want_v, want_a, _ = skin_ref.skin(rest, joints, weights, pal, attrs)
            ref.update_geometry(want_v, mesh=mesh, tri_attrs=want_a)
    got, gst = render(upd)
    want, wst = render(ref)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), schedule
    assert gst == wst, (gst, wst)
    ta, tb = upd.read_tlas(), ref.read_tlas()
    assert ta[0].tobytes() == tb[0].tobytes() and np.array_equal(ta[1], tb[1])
    upd.close()
    ref.close()


def test_carry_over_between_generations():
    """Mesh 1, then mesh 0, then mesh 1 again, each with its own skin: every skin writes the generation that is not current, so
    what it does not rewrite must have been carried over -- after each step the WHOLE buffers equal the host-side composition."""
    s = scenes.instanced_scene(count=5, detail=6)
    pt = PathTracer(s, width=8, height=8)
    slices = mesh_slices(s)
    nodes, tris, attrs = pt._bvhScene.bvh_nodes.copy(), pt._bvhScene.bvh_tris.copy(), pt._bvhScene.tri_attrs.copy()
    J = 8
    skins = {}
    for mesh in (0, 1):
        t0, n = s.mesh_ranges[mesh]
        rest = np.ascontiguousarray(s.vertices[t0 * 3:(t0 + n) * 3])
        skins[mesh] = (rest,) + skin_cases.skin_of(rest, J, mesh) + (attrs[t0:t0 + n].copy() if mesh == 1 else None,)
        pt.set_skin(*skins[mesh][:3], mesh=mesh, rest_attrs=skins[mesh][3], joint_count=J)
    for step, mesh in enumerate((1, 0, 1)):
        t0, n = s.mesh_ranges[mesh]
        rest, joints, weights, rest_attrs = skins[mesh]
        pal = skin_cases.palette(J, 20 + step, amplitude=0.05)
        pt.skin_geometry(pal, mesh=mesh)
        w, a, _ = skin_ref.skin(rest, joints, weights, pal, rest_attrs)
        if a is not None:                                      # the attribute generations flip less often than the geometry's
            attrs[t0:t0 + n] = a
        nodes, tris = compose(s, slices, nodes, tris, mesh, w)
        got_n, got_t, got_a = pt.read_geometry()
        assert np.array_equal(got_n, nodes) and np.array_equal(got_t, tris), step
        assert got_a.tobytes() == attrs.tobytes(), step
    pt.close()


def test_ordering_with_passes_in_flight():
    """Passes enqueued before a skin see the old geometry, passes after it the new, with no host synchronisation between."""
    import torch
    s = scenes.material_zoo()
    J = 16
    joints, weights = zoo_skin(s, J)
    pals = [skin_cases.palette(J, 21, amplitude=0.01), skin_cases.palette(J, 22, amplitude=0.02)]
    ref = PathTracer(s, width=W, height=H)
    statics = [render(ref, 1)[0]]
    for pal in pals:
        ref.update_geometry(skin_ref.skin(s.vertices, joints, weights, pal)[0])
        statics.append(render(ref, 1)[0])
    ref.close()
    assert not np.array_equal(statics[1], statics[2])
    for host in (False, True):
        pt = PathTracer(s, width=W, height=H)
        pt.set_passes_in_flight(12)
        pt.set_skin(s.vertices, joints, weights, joint_count=J)
        dev = f"cuda:{pt.device}"
        outs = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in statics]
        keep = [torch.from_numpy(p.copy()).to(dev) for p in pals]
        torch.cuda.synchronize()
        p = pt.params(seed=0x51)
        pt.render_pass_to(p, outs[0].data_ptr())
        for k in (1, 2):
            if host:
                m = pals[k - 1].copy()
                plugin.check(pt.lib.PTSkinGeometry(pt.ctx, 0, 0, 0, m.ctypes.data, J, 0, None))       # NULL bounds: no synchronisation
                m[:] = np.nan                                  # the library copied the palette before returning
            else:
                pt.skin_geometry(keep[k - 1])
            pt.render_pass_to(p, outs[k].data_ptr())
        pt.synchronize()
        torch.cuda.synchronize()
        for k in range(3):
            assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), statics[k].view(np.uint32)), (host, k)
        pt.close()


def test_animation():
    s = scenes.material_zoo()
    J = 16
    joints, weights = zoo_skin(s, J)
    pt = PathTracer(s, width=W, height=H)
    ref = PathTracer(s, width=W, height=H)
    pt.set_skin(s.vertices, joints, weights, rest_attrs=s.tri_attrs, joint_count=J)
    for f in range(4):
        pal = skin_cases.palette(J, 50, amplitude=0.008 * (f + 1))             # the same pose, growing
        pt.skin_geometry(pal)
        got, _ = render(pt, 1, seed0=0x77 + f)
        want_v, want_a, _ = skin_ref.skin(s.vertices, joints, weights, pal, s.tri_attrs)
        ref.update_geometry(want_v, tri_attrs=want_a)
        want, _ = render(ref, 1, seed0=0x77 + f)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
    pt.close()
    ref.close()


def test_mixing_with_plain_updates():
    ntri, J = 300, 64
    scene = soup_scene(soup(ntri, 40 + ntri))
    rest, joints, weights, attrs = soup_skin(ntri, J, scene.materials.shape[0])
    pt = PathTracer(scene, width=8, height=8)
    built = (pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris)
    pt.set_skin(rest, joints, weights, rest_attrs=attrs, joint_count=J)
    pal = skin_cases.palette(J, 1)
    pt.skin_geometry(pal)
    want_v, want_a, _ = skin_ref.skin(rest, joints, weights, pal, attrs)
    assert_skinned(pt, built, want_v, want_a, "skin")
    w = deformed(rest, 3)
    pt.update_geometry(w)                                      # Part 9 after a skin: the skinned attributes stay
    assert_skinned(pt, built, w, want_a, "plain update after a skin")
    pt.update_geometry(to_device(pt, rest))
    assert_skinned(pt, built, rest, want_a, "device update after a skin")
    pal = skin_cases.palette(J, 2)
    pt.skin_geometry(pal)                                      # ... and a skin after them
    want_v, want_a, _ = skin_ref.skin(rest, joints, weights, pal, attrs)
    assert_skinned(pt, built, want_v, want_a, "skin after plain updates")
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# errors: each refused call leaves the scene as it was, later calls work
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = plugin.load_library()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    m = np.zeros((4, 12), np.float32)
    d = abi.skin_desc()
    for rc in (lib.PTSetSkin(ctx, 0, 0, 0, 1, C.byref(d)), lib.PTSkinGeometry(ctx, 0, 0, 0, m.ctypes.data, 4, 0, None),
               lib.PTSkinGeometryDevice(ctx, 0, 0, 0, m.ctypes.data, 4, 0, None)):
        assert rc == abi.PT_ERR_NO_SCENE
    lib.PTDestroy(ctx)

    v = soup(2000, 2040)
    large = deformed(v, 11)                                    # the builder's tree has 329 nodes for v and 345 for this pose (test_capacity pins both)
    scene = soup_scene(v)
    pt = PathTracer(scene, width=W, height=H, build_device=0)
    n, J = 2000, 4
    joints, weights = skin_cases.skin_of(v, J, 1)
    pal = skin_cases.palette(J, 2, amplitude=0.01)
    before = pt.read_geometry()
    frame = render(pt, 1)[0]

    def unchanged(label):
        after = pt.read_geometry()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), label
        assert np.array_equal(render(pt, 1)[0].view(np.uint32), frame.view(np.uint32)), label

    def refused(rc, text, label):
        message = lib.PTGetLastError()
        assert rc == abi.PT_ERR_INVALID_ARG and all(t in message for t in text.split(b"|")), (label, rc, message)
        unchanged(label)

    out = (C.c_float * 6)()
    refused(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, pal.ctypes.data, J, 0, out), b"no skin", "skin before PTSetSkin")
    bad = joints.copy()
    bad[-1, 3] = J
    d, ntri, keep = plugin.skin_desc(v, bad, weights, J)
    refused(lib.PTSetSkin(pt.ctx, 0, 0, 0, ntri, C.byref(d)), b"joint index", "a joint index out of range")
    refused(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, pal.ctypes.data, J, 0, out), b"no skin", "the refused skin was not kept")
    d, ntri, keep = plugin.skin_desc(v, joints, weights, J)
    refused(lib.PTSetSkin(pt.ctx, 0, 0, 0, ntri - 1, C.byref(d)), b"triangleCount", "not the BLAS's count")
    refused(lib.PTSetSkin(pt.ctx, 1, 0, 0, ntri, C.byref(d)), b"name no BLAS", "offsets that name no BLAS")
    unset = abi.PTSkinDesc()
    refused(lib.PTSetSkin(pt.ctx, 0, 0, 0, ntri, C.byref(unset)), b"structSize", "structSize not set")
    d.weights = None
    refused(lib.PTSetSkin(pt.ctx, 0, 0, 0, ntri, C.byref(d)), b"NULL", "a NULL array")
    pt.set_skin(v, joints, weights, joint_count=J)
    refused(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, pal.ctypes.data, J + 1, 0, out), b"jointCount", "wrong jointCount")
    refused(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, None, J, 0, out), b"NULL", "NULL palette")
    refused(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, pal.ctypes.data, J, 2, out), b"flags", "unknown flags")
    nan = pal.copy()
    nan[2, 5] = np.nan
    refused(lib.PTSkinGeometry(pt.ctx, 0, 0, 0, nan.ctypes.data, J, 0, out), b"joint matrix 2 is not finite", "a NaN host matrix")
    # rebuild over capacity: a one-joint skin whose rest pose is the pose that needs 345 nodes, under the identity
    one = np.zeros((n * 3, 4), np.float32)
    one[:, 0] = 1.0
    pt.set_skin(large, np.zeros((n * 3, 4), np.uint16), one, joint_count=1)
    eye = np.eye(4, dtype=np.float32)[:3].reshape(1, 12).copy()
    assert np.array_equal(skin_ref.skin(large, np.zeros((n * 3, 4), np.uint16), one, eye)[0][:, :3], large[:, :3])
    rc = lib.PTSkinGeometry(pt.ctx, 0, 0, 0, eye.ctypes.data, 1, abi.PT_SKIN_REBUILD, out)
    refused(rc, b"345|329", "rebuild over capacity")
    # later calls work
    bounds = pt.skin_geometry(eye)
    same_bounds(bounds, large)
    want_n, want_t = plugin.refit_cwbvh((before[0], before[1]), large)
    got = pt.read_geometry()
    assert np.array_equal(got[0], want_n) and np.array_equal(got[1], want_t)
    # a NULL desc removes the skin; PTSetScene discards every skin
    pt.set_skin(None, None, None)
    assert lib.PTSkinGeometry(pt.ctx, 0, 0, 0, eye.ctypes.data, 1, 0, out) == abi.PT_ERR_INVALID_ARG and b"no skin" in lib.PTGetLastError()
    pt.set_skin(v, joints, weights, joint_count=J)
    pt.skin_geometry(pal)
    pt._bvhScene.PrepareShader(pt.ctx)
    assert lib.PTSkinGeometry(pt.ctx, 0, 0, 0, pal.ctypes.data, J, 0, out) == abi.PT_ERR_INVALID_ARG and b"no skin" in lib.PTGetLastError()
    got = pt.read_geometry()
    assert np.array_equal(got[0], pt._bvhScene.bvh_nodes) and np.array_equal(got[1], pt._bvhScene.bvh_tris)
    pt.close()
