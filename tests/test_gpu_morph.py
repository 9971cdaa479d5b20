"""Morph targets (PTSetMorph / PTMorphGeometry / PTMorphGeometryDevice, include/ptmi_plugin.h Part 12) on the MI355X.

The morph kernels are checked against tests/morph_ref.py (the rule restated in numpy float32) byte for byte: after a morph the nodes
and triangle rows equal the host refit of the restated vertices, the attribute records equal the restated records.  Frames, TLAS
and counters are compared with a second context that was given those vertices through PTUpdateGeometry / PTRebuildGeometry."""
import ctypes as C
import warnings

import numpy as np
import pytest

import morph_cases
import morph_ref
import skin_cases
import skin_ref
from test_gpu_geometry_update import H, W, compose, mesh_slices, render, soup_scene, to_device
from test_gpu_skin import assert_skinned, same_bounds
from test_refit import deformed, soup
from unity_webgpu_pathtracer_amd import abi, ingest, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (2, 3), (21, 1), (22, 64), (85, 3), (86, 1024), (300, 64), (5000, 8)]      # 3 T = 63 / 66, 255 / 258: a slice, a workgroup
JOINTS = 16


def soup_morph(ntri, target_count, pattern, materials, scale=0.25):
    """rest, (position, normal, tangent) streams, rest attributes, (joints, weights) of a skin"""
    rest = soup(ntri, 40 + ntri)
    seed = 1000 * ntri + target_count
    streams = [morph_cases.stream(ntri * 3, target_count, pattern, seed + k, s) for k, s in enumerate((scale, 0.5, 0.5))]
    return rest, streams, skin_cases.rest_attrs(ntri, ntri + 1, material_count=materials), skin_cases.skin_of(rest, JOINTS, seed + 5)


# ---------------------------------------------------------------------------------------------------------------------
# bytes against the restated rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", morph_cases.PATTERNS)
@pytest.mark.parametrize("ntri,target_count", CASES)
def test_bytes_equal_the_restatement(ntri, target_count, pattern):
    scene = soup_scene(soup(ntri, 40 + ntri))
    rest, (pos, nrm, tan), attrs, skin = soup_morph(ntri, target_count, pattern, scene.materials.shape[0])
    pt = PathTracer(scene, width=8, height=8)
    built = (pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris)
    pt.set_skin(rest[::-1].copy(), *skin, joint_count=JOINTS)            # the skin's own rest pose is not the morph's, and is not used
    cur_a = np.ascontiguousarray(scene.tri_attrs)
    step = 0
    # every PTSetMorph after the first replaces the morph.  "streams": normal and tangent streams; "records": rest attributes but no
    # stream (copied, or with a palette skinned); "none": no rest attributes, the records are not touched
    for mode in ("streams", "none", "records"):
        n_, t_, a_ = (nrm, tan, attrs) if mode == "streams" else (None, None, attrs if mode == "records" else None)
        pt.set_morph(rest, pos, n_, t_, rest_attrs=a_, target_count=target_count)
        for palette in (False, True):
            for _ in range(3 if step == 0 else 1):                      # three morphs first: both generations are written, the first one twice
                w = morph_cases.weights(target_count, 100 * step + target_count)
                pal = skin_cases.palette(JOINTS, 50 + step) if palette else None
                bounds = pt.morph_geometry(w, pal)
                want_v, want_a, _ = morph_ref.morph(rest, pos, w, n_, t_, a_, skin if palette else None, pal)
                cur_a = cur_a if want_a is None else want_a
                assert_skinned(pt, built, want_v, cur_a, (ntri, target_count, pattern, mode, palette, step))
                same_bounds(bounds, want_v)
                step += 1
    pt.close()


def test_device_weights_and_palette_give_the_same_bytes():
    import torch
    ntri, K = 300, 64
    scene = soup_scene(soup(ntri, 40 + ntri))
    rest, (pos, nrm, tan), attrs, skin = soup_morph(ntri, K, "random", scene.materials.shape[0])
    w, pal = morph_cases.weights(K, 3), skin_cases.palette(JOINTS, 5)
    for palette in (False, True):
        out = []
        for device in (False, True):
            pt = PathTracer(scene, width=8, height=8)
            pt.set_skin(rest, *skin, joint_count=JOINTS)
            pt.set_morph(rest, pos, nrm, tan, rest_attrs=attrs, target_count=K)
            dev = f"cuda:{pt.device}"
            m = None if not palette else torch.from_numpy(pal.reshape(JOINTS, 3, 4).copy()).to(dev) if device else pal
            bounds = pt.morph_geometry(torch.from_numpy(w.copy()).to(dev) if device else w, m)
            out.append([a.tobytes() for a in pt.read_geometry()] + [bounds.tobytes()])
            pt.close()
        assert out[0] == out[1], palette
        want_v, _, _ = morph_ref.morph(rest, pos, w, skin=skin if palette else None, palette=pal if palette else None)
        same_bounds(np.frombuffer(out[1][3], np.float32).reshape(2, 3), want_v)


# ---------------------------------------------------------------------------------------------------------------------
# rebuild
# ---------------------------------------------------------------------------------------------------------------------
def test_rebuild_equals_a_rebuild_of_the_restated_vertices():
    ntri, K = 300, 8
    scene = soup_scene(soup(ntri, 40 + ntri))
    rest, (pos, nrm, tan), attrs, skin = soup_morph(ntri, K, "random", scene.materials.shape[0])
    w, pal = morph_cases.weights(K, 9), skin_cases.palette(JOINTS, 9, amplitude=0.3)
    want_v, want_a, _ = morph_ref.morph(rest, pos, w, nrm, tan, attrs, skin, pal)
    upd = PathTracer(scene, width=W, height=H, build_device=0, node_capacity=2.0)
    ref = PathTracer(scene, width=W, height=H, build_device=0, node_capacity=2.0)
    upd.set_skin(rest, *skin, joint_count=JOINTS)
    upd.set_morph(rest, pos, nrm, tan, rest_attrs=attrs, target_count=K)
    render(upd, 1)
    bounds = upd.morph_geometry(w, pal, rebuild=True)
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
    assert upd.morph_geometry(w, pal, rebuild_above=1e9)[1] == "refit"
    assert upd.morph_geometry(w, rebuild_above=0.0)[1] == "rebuild"
    upd.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# frames against a second context given the restated vertices through PTUpdateGeometry
# ---------------------------------------------------------------------------------------------------------------------
def mesh_morph(rest, ntri, K, seed, scale):
    """Sparse position, normal and tangent streams for a mesh of a scene"""
    return [morph_cases.stream(ntri * 3, K, "random", seed + k, s) for k, s in enumerate((scale, 0.3, 0.3))]


@pytest.mark.parametrize("schedule", [0, 1])
def test_frames_after_morph_flat(schedule):
    s = scenes.material_zoo()
    K = 6
    pos, nrm, tan = mesh_morph(s.vertices, s.tri_count, K, 70, 0.02)
    skin = skin_cases.skin_of(s.vertices, JOINTS, 77)
    w, pal = morph_cases.weights(K, 2), skin_cases.palette(JOINTS, 3, amplitude=0.02)
    upd = PathTracer(s, width=W, height=H, schedule=schedule)
    ref = PathTracer(s, width=W, height=H, schedule=schedule)
    upd.set_skin(s.vertices, *skin, joint_count=JOINTS)
    upd.set_morph(s.vertices, pos, nrm, tan, rest_attrs=s.tri_attrs, target_count=K)
    render(upd, 1)
    for m, sk in ((None, None), (pal, skin)):
        upd.morph_geometry(w, m)
        want_v, want_a, _ = morph_ref.morph(s.vertices, pos, w, nrm, tan, s.tri_attrs, sk, m)
        ref.update_geometry(want_v, tri_attrs=want_a)
        got, gst = render(upd)
        want, wst = render(ref)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (schedule, m is not None)
        assert gst == wst, (gst, wst)
    upd.close()
    ref.close()


@pytest.mark.parametrize("schedule", [0, 1])
def test_frames_after_morph_instanced(schedule):
    s = scenes.instanced_scene()
    upd = PathTracer(s, width=W, height=H, schedule=schedule)
    ref = PathTracer(s, width=W, height=H, schedule=schedule)
    render(upd, 1)
    K = 5
    with warnings.catch_warnings():
        warnings.simplefilter("error")                         # no warning: the bounds come back, the TLAS stays exact
        for mesh in (0, 2):
            t0, n = s.mesh_ranges[mesh]
            rest = np.ascontiguousarray(s.vertices[t0 * 3:(t0 + n) * 3])
            attrs = np.ascontiguousarray(s.tri_attrs[t0:t0 + n])
            pos, nrm, tan = mesh_morph(rest, n, K, 5 + mesh, 0.1)
            w = morph_cases.weights(K, 9 + mesh)
            upd.set_morph(rest, pos, nrm, tan, mesh=mesh, rest_attrs=attrs, target_count=K)
            upd.morph_geometry(w, mesh=mesh)
            want_v, want_a, _ = morph_ref.morph(rest, pos, w, nrm, tan, attrs)
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
    """Mesh 1, then mesh 0, then mesh 1 again, each with its own morph: every morph writes the generation that is not current, so
    what it does not rewrite must have been carried over -- after each step the WHOLE buffers equal the host-side composition."""
    s = scenes.instanced_scene(count=5, detail=6)
    pt = PathTracer(s, width=8, height=8)
    slices = mesh_slices(s)
    nodes, tris, attrs = pt._bvhScene.bvh_nodes.copy(), pt._bvhScene.bvh_tris.copy(), pt._bvhScene.tri_attrs.copy()
    K = 4
    morphs = {}
    for mesh in (0, 1):
        t0, n = s.mesh_ranges[mesh]
        rest = np.ascontiguousarray(s.vertices[t0 * 3:(t0 + n) * 3])
        pos, nrm, tan = mesh_morph(rest, n, K, mesh, 0.05)
        morphs[mesh] = (rest, pos) + ((nrm, tan, attrs[t0:t0 + n].copy()) if mesh == 1 else (None, None, None))
        pt.set_morph(*morphs[mesh][:4], mesh=mesh, rest_attrs=morphs[mesh][4], target_count=K)
    for step, mesh in enumerate((1, 0, 1)):
        t0, n = s.mesh_ranges[mesh]
        rest, pos, nrm, tan, rest_attrs = morphs[mesh]
        w = morph_cases.weights(K, 20 + step)
        pt.morph_geometry(w, mesh=mesh)
        v, a, _ = morph_ref.morph(rest, pos, w, nrm, tan, rest_attrs)
        if a is not None:                                      # the attribute generations flip less often than the geometry's
            attrs[t0:t0 + n] = a
        nodes, tris = compose(s, slices, nodes, tris, mesh, v)
        got_n, got_t, got_a = pt.read_geometry()
        assert np.array_equal(got_n, nodes) and np.array_equal(got_t, tris), step
        assert got_a.tobytes() == attrs.tobytes(), step
    pt.close()


def test_ordering_with_passes_in_flight():
    """Passes enqueued before a morph see the old geometry, passes after it the new, with no host synchronisation between."""
    import torch
    s = scenes.material_zoo()
    K = 6
    pos, _, _ = mesh_morph(s.vertices, s.tri_count, K, 70, 0.02)
    ws = [morph_cases.weights(K, 21), morph_cases.weights(K, 22)]
    ref = PathTracer(s, width=W, height=H)
    statics = [render(ref, 1)[0]]
    for w in ws:
        ref.update_geometry(morph_ref.morph(s.vertices, pos, w)[0])
        statics.append(render(ref, 1)[0])
    ref.close()
    assert not np.array_equal(statics[1], statics[2])
    for host in (False, True):
        pt = PathTracer(s, width=W, height=H)
        pt.set_passes_in_flight(12)
        pt.set_morph(s.vertices, pos, target_count=K)
        dev = f"cuda:{pt.device}"
        outs = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in statics]
        keep = [torch.from_numpy(w.copy()).to(dev) for w in ws]
        torch.cuda.synchronize()
        p = pt.params(seed=0x51)
        pt.render_pass_to(p, outs[0].data_ptr())
        for k in (1, 2):
            if host:
                w = ws[k - 1].copy()
                plugin.check(pt.lib.PTMorphGeometry(pt.ctx, 0, 0, 0, w.ctypes.data, K, None, 0, 0, None))     # NULL bounds: no synchronisation
                w[:] = np.nan                                  # the library copied the weights before returning
            else:
                pt.morph_geometry(keep[k - 1])
            pt.render_pass_to(p, outs[k].data_ptr())
        pt.synchronize()
        torch.cuda.synchronize()
        for k in range(3):
            assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), statics[k].view(np.uint32)), (host, k)
        pt.close()


def test_mixing_with_skins_and_plain_updates():
    ntri, K = 300, 64
    scene = soup_scene(soup(ntri, 40 + ntri))
    rest, (pos, nrm, tan), attrs, skin = soup_morph(ntri, K, "random", scene.materials.shape[0])
    pt = PathTracer(scene, width=8, height=8)
    built = (pt._bvhScene.bvh_nodes, pt._bvhScene.bvh_tris)
    other = deformed(rest, 5)                                  # the skin has its own rest pose and its own rest attributes
    pt.set_skin(other, *skin, rest_attrs=attrs, joint_count=JOINTS)
    pt.set_morph(rest, pos, nrm, tan, rest_attrs=attrs, target_count=K)
    w, pal = morph_cases.weights(K, 1), skin_cases.palette(JOINTS, 1)
    pt.morph_geometry(w)
    want_v, want_a, _ = morph_ref.morph(rest, pos, w, nrm, tan, attrs)
    assert_skinned(pt, built, want_v, want_a, "morph")
    pt.skin_geometry(pal)                                      # Part 11 after a morph: the skin's rest pose, not the morph's
    want_v, want_a, _ = skin_ref.skin(other, *skin, pal, attrs)
    assert_skinned(pt, built, want_v, want_a, "skin after a morph")
    v = deformed(rest, 3)
    pt.update_geometry(v)                                      # Part 9: the attributes stay
    assert_skinned(pt, built, v, want_a, "plain update")
    pt.update_geometry(to_device(pt, rest))
    assert_skinned(pt, built, rest, want_a, "device update")
    pt.morph_geometry(w, pal)                                  # morph + skin after them: the morph's rest pose, the skin's joints
    want_v, want_a, _ = morph_ref.morph(rest, pos, w, nrm, tan, attrs, skin, pal)
    assert_skinned(pt, built, want_v, want_a, "morph + skin after plain updates")
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# errors: each refused call leaves the scene as it was, later calls work
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = plugin.load_library()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    w4 = np.zeros(4, np.float32)
    d = abi.morph_desc()
    for rc in (lib.PTSetMorph(ctx, 0, 0, 0, 1, C.byref(d)), lib.PTMorphGeometry(ctx, 0, 0, 0, w4.ctypes.data, 4, None, 0, 0, None),
               lib.PTMorphGeometryDevice(ctx, 0, 0, 0, w4.ctypes.data, 4, None, 0, 0, None)):
        assert rc == abi.PT_ERR_NO_SCENE
    lib.PTDestroy(ctx)

    ntri, K, J = 300, 4, 4
    v = soup(ntri, 40 + ntri)
    scene = soup_scene(v)
    pt = PathTracer(scene, width=W, height=H)
    pos, nrm, tan = mesh_morph(v, ntri, K, 3, 0.05)
    attrs = skin_cases.rest_attrs(ntri, 1, material_count=scene.materials.shape[0])
    joints, sw = skin_cases.skin_of(v, J, 1)
    w, pal = morph_cases.weights(K, 2), skin_cases.palette(J, 2, amplitude=0.01)
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

    def morph(weights=w, count=K, palette=None, joints_=0, flags=0):
        return lib.PTMorphGeometry(pt.ctx, 0, 0, 0, None if weights is None else weights.ctypes.data, count, None if palette is None else palette.ctypes.data,
                                   joints_, flags, out)

    def set_morph(count=ntri, offsets=(0, 0, 0), **kw):
        args = dict(rest_vertices=v, target_count=K, position=pos, normal=nrm, tangent=tan, rest_attrs=attrs)
        args.update(kw)
        d, _, keep = plugin.morph_desc(**args)
        return lib.PTSetMorph(pt.ctx, *offsets, count, C.byref(d))

    refused(morph(), b"no morph", "morph before PTSetMorph")
    bad = pos[1].copy()
    bad["target"][-1] = K
    refused(set_morph(position=(pos[0], bad)), b"position stream|target 4 >= targetCount", "a target out of range")
    refused(morph(), b"no morph", "the refused morph was not kept")
    refused(set_morph(target_count=0), b"targetCount", "targetCount 0")
    refused(set_morph(target_count=1025), b"targetCount", "targetCount 1025")
    bad = nrm[1].copy()
    bad["dx"][0] = np.nan
    refused(set_morph(normal=(nrm[0], bad)), b"normal stream|not finite", "a NaN delta")
    refused(set_morph(rest_attrs=None), b"needs restAttrs", "a normal stream without restAttrs")
    bad = attrs.copy()
    bad["materialIndex"][7] = scene.materials.shape[0]
    refused(set_morph(rest_attrs=bad), b"materialIndex", "a materialIndex out of range on a flat scene")
    refused(set_morph(count=ntri - 1), b"triangleCount", "not the BLAS's count")
    refused(set_morph(offsets=(1, 0, 0)), b"name no BLAS", "offsets that name no BLAS")
    unset = abi.PTMorphDesc()
    refused(lib.PTSetMorph(pt.ctx, 0, 0, 0, ntri, C.byref(unset)), b"structSize", "structSize not set")
    assert set_morph() == abi.PT_OK
    refused(morph(count=K + 1), b"targetCount", "wrong targetCount")
    refused(morph(weights=None), b"NULL", "NULL weights")
    refused(morph(flags=2), b"flags", "unknown flags")
    nan = w.copy()
    nan[2] = np.inf
    refused(morph(weights=nan), b"morph weight 2 is not finite", "an infinite host weight")
    refused(morph(palette=pal, joints_=J), b"palette needs a skin", "a palette without a skin")
    pt.set_skin(v, joints, sw, joint_count=J)
    refused(morph(palette=pal, joints_=J + 1), b"jointCount", "wrong jointCount")
    nan = pal.copy()
    nan[1, 5] = np.nan
    refused(morph(palette=nan, joints_=J), b"joint matrix 1 is not finite", "a NaN host matrix")
    # later calls work
    bounds = pt.morph_geometry(w, pal)
    want_v, want_a, _ = morph_ref.morph(v, pos, w, nrm, tan, attrs, (joints, sw), pal)
    same_bounds(bounds, want_v)
    assert_skinned(pt, (before[0], before[1]), want_v, want_a, "after the refusals")
    # a NULL desc removes the morph and leaves the skin; PTSetScene discards every morph
    pt.set_morph(None, None)
    assert morph() == abi.PT_ERR_INVALID_ARG and b"no morph" in lib.PTGetLastError()
    pt.skin_geometry(pal)
    assert set_morph() == abi.PT_OK
    pt.morph_geometry(w)
    pt._bvhScene.PrepareShader(pt.ctx)
    assert morph() == abi.PT_ERR_INVALID_ARG and b"no morph" in lib.PTGetLastError()
    got = pt.read_geometry()
    assert np.array_equal(got[0], pt._bvhScene.bvh_nodes) and np.array_equal(got[1], pt._bvhScene.bvh_tris)
    pt.close()


# ---------------------------------------------------------------------------------------------------------------------
# a GLB clip end to end: file -> targets, skin and channels -> weights and palette per frame -> the GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_glb_clip(tmp_path):
    """Two joints, two targets, LINEAR channels, four frames: after every morph_geometry the geometry and the frame equal those of a
    reference context that was given the host twin's vertices."""
    from test_morph import quaternion
    nx = 10
    grid = np.array([[x * 0.1 - 0.5, y * 0.2 + 0.3, 0.05 * np.sin(x)] for x in range(nx) for y in range(3)], np.float32)
    quads = [(x * 3 + y, (x + 1) * 3 + y, (x + 1) * 3 + y + 1, x * 3 + y + 1) for x in range(nx - 1) for y in range(2)]
    idx = np.array([(a, b, c, a, c, d) for a, b, c, d in quads], np.uint16).reshape(-1)
    mesh = ingest.Mesh(positions=grid, normals=None, tangents=None, uvs=None, indices=idx, local_to_world=np.eye(4), material_index=0, name="strip")
    rng = np.random.RandomState(1)
    local = np.tile(np.eye(4), (2, 1, 1))
    local[0, :3, 3], local[1, :3, 3] = (-0.5, 0.3, 0.0), (0.5, 0.0, 0.0)
    world = [local[0], local[0] @ local[1]]
    u = (grid[:, 0] + 0.5)[:, None]                          # along the strip: joint 0 at one end, joint 1 at the other
    weights = np.concatenate([1 - u, u, np.zeros((len(grid), 2))], axis=1).astype(np.float32)
    skin = dict(joints=np.tile(np.array([0, 1, 0, 0], np.uint16), (len(grid), 1)), weights=weights,
                inverse_bind=np.stack([np.linalg.inv(w) for w in world]), parents=np.array([-1, 0], np.int32), local=local)
    deltas = rng.uniform(-0.05, 0.05, (2, len(grid), 3)).astype(np.float32)
    deltas[1, ::2] = 0.0
    times = np.array([0.0, 0.5, 1.0])
    channels = [dict(node=("joint", 0, 1), path="rotation", interpolation="LINEAR", times=times, values=np.stack([quaternion((0, 0, 1), a) for a in (0.0, 0.4, -0.3)])),
                dict(node=("joint", 0, 0), path="translation", interpolation="LINEAR", times=times, values=np.array([[-0.5, 0.3, 0], [-0.45, 0.35, 0.05], [-0.5, 0.25, 0]])),
                dict(node=0, path="weights", interpolation="LINEAR", times=times, values=np.array([[0, 0], [1, 0.5], [0.25, 1]]))]
    path = str(tmp_path / "clip.glb")
    ingest.write_glb(path, [mesh], skins=[skin], morphs=[dict(position=deltas)], animations=[dict(name="clip", channels=channels)])

    meshes, _, _ = ingest.load_glb(path, load_images=False)
    g, m, anim = ingest.load_glb_skins(path)[0], ingest.load_glb_morphs(path)[0], ingest.load_glb_animations(path)[0]
    rest = np.zeros((len(meshes[0].indices), 4), np.float32)
    rest[:, :3] = meshes[0].positions[meshes[0].indices.astype(np.int64)]
    scene = soup_scene(rest)
    pt = PathTracer(scene, width=W, height=H)
    ref = PathTracer(scene, width=W, height=H)
    pt.set_skin(rest, g["joints"], g["weights"], joint_count=2)
    pt.set_morph(rest, m["position"])
    position = plugin.morph_csr(m["position"])
    assert 0 < len(position[1]) < m["position"].shape[0] * m["position"].shape[1]          # the zero rows of target 1 are not listed
    frames = []
    for f, t in enumerate(np.linspace(0.0, anim["duration"], 4)):
        s = ingest.sample_animation(anim, t)
        pal = ingest.joint_matrices(g, s["local"][0])
        w = s["weights"][0].astype(np.float32)
        bounds = pt.morph_geometry(w, pal)
        want_v, _, _ = plugin.morph_vertices(rest, position, w, skin=(g["joints"], g["weights"]), joint_matrices=pal)
        same_bounds(bounds, want_v)
        ref.update_geometry(want_v)
        ga, gb = pt.read_geometry(), ref.read_geometry()
        assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes(), f
        got, _ = render(pt, 1, seed0=0x77 + f)
        want, _ = render(ref, 1, seed0=0x77 + f)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
        frames.append(want_v)
    assert all(not np.array_equal(frames[k], frames[k + 1]) for k in range(3))             # the clip moves
    pt.close()
    ref.close()
