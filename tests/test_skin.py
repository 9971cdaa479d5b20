"""Skinned geometry on the host (PTSkinVerticesHost, include/ptmi_plugin.h Part 11) and GLB skins, no GPU needed.

The host twin's bytes are pinned against tests/skin_ref.py (the rule restated in numpy float32, one operation per line): the
rule is bit-defined, so positions, attribute records and bounds are compared byte for byte."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import skin_cases
import skin_ref
from kernel_resources import resources
from test_refit import soup
from unity_webgpu_pathtracer_amd import abi, ingest, plugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART11 = ("PTSetSkin", "PTSkinGeometry", "PTSkinGeometryDevice", "PTSkinVerticesHost")
TRIANGLES = [1, 2, 21, 22, 85, 86, 300]          # 3 T = 63 / 66 and 255 / 258: around a wave and a workgroup
JOINTS = [1, 2, 64, 1024]


def test_symbols_exported_and_bound():
    lib = plugin.load_library()
    for name in PART11:
        assert hasattr(lib, name), name
        assert name in plugin.EXPORTED_SYMBOLS and getattr(lib, name).argtypes == plugin.sig[name][1]
    assert abi.PT_SKIN_MAX_JOINTS == 1024 and abi.PT_SKIN_REBUILD == 1
    assert abi.skin_desc().structSize == C.sizeof(abi.PTSkinDesc)


def test_desc_size_matches_the_header():
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "ptmi_plugin.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %u %u\n", sizeof(PTSkinDesc), offsetof(PTSkinDesc, jointCount), offsetof(PTSkinDesc, restVertices),
             offsetof(PTSkinDesc, joints), offsetof(PTSkinDesc, weights), offsetof(PTSkinDesc, restAttrs), PT_SKIN_MAX_JOINTS, PT_SKIN_REBUILD);
      return 0; }
    """
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    D = abi.PTSkinDesc
    assert got == [C.sizeof(D), D.jointCount.offset, D.restVertices.offset, D.joints.offset, D.weights.offset, D.restAttrs.offset,
                   abi.PT_SKIN_MAX_JOINTS, abi.PT_SKIN_REBUILD]


@pytest.mark.parametrize("joint_count", JOINTS)
@pytest.mark.parametrize("ntri", TRIANGLES)
def test_host_twin_equals_the_restatement(ntri, joint_count):
    rest = soup(ntri, 300 + ntri)
    joints, weights = skin_cases.skin_of(rest, joint_count, 7 * ntri + joint_count)
    assert (weights == 0).any() or ntri < 3
    attrs = skin_cases.rest_attrs(ntri, ntri, material_count=3)
    pal = skin_cases.palette(joint_count, 11 * joint_count + ntri)
    want_v, want_a, want_b = skin_ref.skin(rest, joints, weights, pal, attrs)
    got_v, got_a, got_b = plugin.skin_vertices(rest, joints, weights, pal.reshape(-1, 3, 4), attrs)
    assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))
    assert got_a.tobytes() == want_a.tobytes()
    assert got_b.tobytes() == want_b.tobytes()
    assert (got_v[:, 3] == 0).all()
    # without rest attributes: the same positions, no records
    v2, a2, b2 = plugin.skin_vertices(rest, joints, weights, pal)
    assert a2 is None and v2.tobytes() == want_v.tobytes() and b2.tobytes() == want_b.tobytes()


def test_one_hot_weights_are_the_rigid_transform():
    rest = soup(50, 5)
    rng = np.random.RandomState(3)
    joints = rng.randint(0, 16, (150, 4)).astype(np.uint16)
    weights = np.zeros((150, 4), np.float32)
    hot = rng.randint(0, 4, 150)
    weights[np.arange(150), hot] = 1.0
    pal = skin_cases.palette(16, 9)
    got, _, _ = plugin.skin_vertices(rest, joints, weights, pal)
    m = pal[joints[np.arange(150), hot]]                 # the one joint's matrix: 1 * m + 0 * the others is m exactly
    want = skin_ref.positions(m, rest)
    assert np.array_equal(got, want)


def test_zero_length_rest_normal_is_kept():
    rest = soup(4, 1)
    joints, weights = skin_cases.skin_of(rest, 8, 2)
    attrs = skin_cases.rest_attrs(4, 3)
    attrs["normal1"][2] = 0.0
    attrs["tangent0"][1] = 0.0
    _, got, _ = plugin.skin_vertices(rest, joints, weights, skin_cases.palette(8, 4), attrs)
    assert (got["normal1"][2] == 0).all() and (got["tangent0"][1] == 0).all()
    others = got.view(np.float32).reshape(-1, 8, 4)[:, :6, :3]
    norms = np.linalg.norm(others.astype(np.float64), axis=2)
    norms[2, 1] = norms[1, 3] = 1.0
    assert np.abs(norms - 1).max() < 1e-6
    for f in ("uv0", "uv1", "uv2", "materialIndex", "pad0", "pad3", "pad6"):
        assert got[f].tobytes() == attrs[f].tobytes(), f


def test_host_twin_refusals():
    rest = soup(10, 1)
    joints, weights = skin_cases.skin_of(rest, 8, 2)
    pal = skin_cases.palette(8, 4)
    plugin.skin_vertices(rest, joints, weights, pal)
    bad = joints.copy()
    bad[17, 2] = 8
    with pytest.raises(plugin.PluginError, match="joint index 8 >= jointCount"):
        plugin.skin_vertices(rest, bad, weights, pal)
    bad = weights.copy()
    bad[5, 1] = np.nan
    with pytest.raises(plugin.PluginError, match="weight"):
        plugin.skin_vertices(rest, joints, bad, pal)
    bad = pal.copy()
    bad[3, 7] = np.nan
    with pytest.raises(plugin.PluginError, match="joint matrix 3 is not finite"):
        plugin.skin_vertices(rest, joints, weights, bad)
    bad = rest.copy()
    bad[4, 0] = np.inf
    with pytest.raises(plugin.PluginError, match="rest vertex 4"):
        plugin.skin_vertices(bad, joints, weights, pal)
    with pytest.raises(plugin.PluginError, match="jointCount"):
        plugin.skin_vertices(rest, np.zeros_like(joints), weights, np.zeros((1025, 12), np.float32))


# ---- GLB skins ----
def glb_case(seed=0):
    """An indexed mesh (a strip of quads along x) with a chain of 5 joints plus a branch, smooth 4-influence weights"""
    rng = np.random.RandomState(seed)
    nx = 12
    grid = np.array([[x * 0.5, y * 0.3, 0.1 * np.sin(x)] for x in range(nx) for y in range(3)], np.float32)
    quads = [(x * 3 + y, (x + 1) * 3 + y, (x + 1) * 3 + y + 1, x * 3 + y + 1) for x in range(nx - 1) for y in range(2)]
    idx = np.array([(a, b, c, a, c, d) for a, b, c, d in quads], np.uint16).reshape(-1)
    parents = np.array([-1, 0, 1, 2, 3, 1], np.int32)
    local = np.tile(np.eye(4), (6, 1, 1))
    for j in range(6):
        local[j, :3, :3] = skin_cases.rotation(rng)
        local[j, :3, 3] = rng.uniform(-1, 1, 3)
    world = [None] * 6
    for j in range(6):
        world[j] = local[j] if parents[j] < 0 else world[parents[j]] @ local[j]
    inverse_bind = np.stack([np.linalg.inv(w) for w in world])
    joints = rng.randint(0, 6, (len(grid), 4)).astype(np.uint16)
    w = rng.uniform(0, 1, (len(grid), 4))
    w[::5, 3] = 0.0
    weights = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    mesh = ingest.Mesh(positions=grid, normals=None, tangents=None, uvs=None, indices=idx, local_to_world=np.eye(4), material_index=0, name="strip")
    return mesh, dict(joints=joints, weights=weights, inverse_bind=inverse_bind, parents=parents, local=local)


def soup_of(mesh):
    v = np.zeros((len(mesh.indices), 4), np.float32)
    v[:, :3] = mesh.positions[mesh.indices.astype(np.int64)]
    return v


def posed(skin, seed):
    rng = np.random.RandomState(seed)
    local = np.array(skin["local"], copy=True)
    for j in range(len(local)):
        local[j, :3, :3] = local[j, :3, :3] @ skin_cases.rotation(rng)
        local[j, :3, 3] += rng.uniform(-0.2, 0.2, 3)
    return local


def test_glb_skin_round_trip(tmp_path):
    mesh, skin = glb_case()
    plain = ingest.Mesh(positions=mesh.positions[::-1].copy(), normals=None, tangents=None, uvs=None, indices=None, local_to_world=np.eye(4), material_index=0, name="plain")
    path = str(tmp_path / "skinned.glb")
    ingest.write_glb(path, [plain, mesh], skins=[None, skin])
    meshes, _, _ = ingest.load_glb(path, unity_handedness=False, load_images=False)
    got = ingest.load_glb_skins(path, unity_handedness=False)
    assert len(got) == len(meshes) == 2 and got[0] is None
    g = got[1]
    ix = mesh.indices.astype(np.int64)
    assert np.array_equal(g["joints"], skin["joints"][ix]) and g["joints"].dtype == np.uint16
    assert np.array_equal(g["weights"], skin["weights"][ix]) and g["weights"].dtype == np.float32
    assert np.array_equal(g["parents"], skin["parents"])
    assert np.allclose(g["inverse_bind"], skin["inverse_bind"], rtol=0, atol=1e-6)      # stored as float32
    assert np.allclose(g["local"], skin["local"], rtol=0, atol=1e-12)
    assert np.array_equal(soup_of(meshes[1]), soup_of(mesh))


def test_write_glb_without_skins_is_unchanged(tmp_path):
    mesh, _ = glb_case()
    a, b, c = (str(tmp_path / n) for n in ("a.glb", "b.glb", "c.glb"))
    ingest.write_glb(a, [mesh])
    ingest.write_glb(b, [mesh], skins=None)
    ingest.write_glb(c, [mesh], skins=[None])
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def test_glb_rest_pose_reproduces_the_rest_vertices(tmp_path):
    mesh, skin = glb_case(1)
    path = str(tmp_path / "skinned.glb")
    ingest.write_glb(path, [mesh], skins=[skin])
    for handed in (False, True):
        meshes, _, _ = ingest.load_glb(path, unity_handedness=handed, load_images=False)
        g = ingest.load_glb_skins(path, unity_handedness=handed)[0]
        rest = soup_of(meshes[0])
        pal = ingest.joint_matrices(g)
        assert pal.shape == (6, 3, 4) and pal.dtype == np.float32
        got, _, _ = plugin.skin_vertices(rest, g["joints"], g["weights"], pal)
        scale = np.abs(rest[:, :3]).max()                  # relative to the mesh's size: a coordinate may itself be 0
        assert np.abs(got[:, :3] - rest[:, :3]).max() <= 1e-6 * scale, np.abs(got[:, :3] - rest[:, :3]).max()


def test_glb_handedness_is_applied_consistently(tmp_path):
    mesh, skin = glb_case(2)
    path = str(tmp_path / "skinned.glb")
    ingest.write_glb(path, [mesh], skins=[skin])
    out = {}
    for handed in (False, True):
        meshes, _, _ = ingest.load_glb(path, unity_handedness=handed, load_images=False)
        g = ingest.load_glb_skins(path, unity_handedness=handed)[0]
        local = posed(g, 5) if not handed else None
        if handed:                                          # the same pose, mirrored as the loader mirrors matrices: M' = F M F
            flip = np.diag([1.0, 1.0, -1.0, 1.0])
            local = flip @ out["local"] @ flip
        else:
            out["local"] = local
        pal = ingest.joint_matrices(g, local)
        out[handed], _, _ = plugin.skin_vertices(soup_of(meshes[0]), g["joints"], g["weights"], pal)
    assert np.abs(out[False][:, :3] - soup_of(mesh)[:, :3]).max() > 0.1        # a non-trivial pose
    want = out[False].reshape(-1, 3, 4)[:, ::-1].reshape(-1, 4) * np.array([1, 1, -1, 1], np.float32)      # mirrored z, reversed winding
    assert np.abs(out[True] - want).max() <= 1e-5 * np.abs(want).max()


# ---- the kernels' resources and the sanitizers ----
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_skin_kernel_resources():
    res = resources("pt_skin.hip")
    kernels = {name: r for k, r in res.items() for name in ("pt_skin_vertices", "pt_skin_bounds_fold", "pt_skin_attrs") if name in k}
    assert len(kernels) == 3 == len(res), list(res)
    for k, r in kernels.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
    assert {k: r["vgprs"] for k, r in kernels.items()} == VGPRS, kernels


VGPRS = {"pt_skin_vertices": 60, "pt_skin_bounds_fold": 18, "pt_skin_attrs": 59}          # what the build shows; 8 waves per SIMD each


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_host_twin_under_sanitizers(tmp_path):
    """`make skin-sanitize`: the host twin and csrc/skin_sanitize_main.cpp (its own main) with -fsanitize=address,undefined, built
    and run -- it skins a generated mesh, checks the result and makes the refusals, and must finish without a report."""
    csrc = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "skin-sanitize", "SKIN_SANITIZE_OUT=" + str(tmp_path / "skin_sanitize")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "skin ok" in out.stdout, out.stdout + out.stderr
