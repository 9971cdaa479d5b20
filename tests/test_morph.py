"""Morph targets on the host (PTMorphVerticesHost, include/ptmi_plugin.h Part 12), the device layout's conversion and
GLB morph targets and animations, no GPU needed.

The host twin's bytes are pinned against tests/morph_ref.py (the rule restated in numpy float32, one operation per line): the rule
is bit-defined, so positions, attribute records and bounds are compared byte for byte."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import morph_cases
import morph_ref
import skin_cases
from kernel_resources import resources
from test_refit import soup
from test_skin import glb_case, soup_of
from unity_webgpu_pathtracer_amd import abi, ingest, plugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART12 = ("PTSetMorph", "PTMorphGeometry", "PTMorphGeometryDevice", "PTMorphVerticesHost", "PTMorphLayoutHost")
TRIANGLES = [1, 2, 21, 22, 85, 86, 300]          # 3 T = 63 / 66 and 255 / 258: around a slice and a workgroup
TARGETS = [1, 3, 64, 1024]
JOINTS = 16


def test_symbols_exported_and_bound():
    lib = plugin.load_library()
    for name in PART12:
        assert hasattr(lib, name), name
        assert name in plugin.EXPORTED_SYMBOLS and getattr(lib, name).argtypes == plugin.sig[name][1]
    assert abi.PT_MORPH_MAX_TARGETS == 1024
    assert abi.morph_desc().structSize == C.sizeof(abi.PTMorphDesc)
    assert lib.PTGetVersion() == (0 << 16) | 2


def test_desc_size_matches_the_header():
    fields = ("targetCount", "restVertices", "restAttrs", "positionOffsets", "positionEntries", "normalOffsets", "normalEntries", "tangentOffsets", "tangentEntries")
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "ptmi_plugin.h"
    int main(void) {
      printf("%zu %zu %zu %u", sizeof(PTMorphDesc), sizeof(PTMorphEntry), offsetof(PTMorphEntry, target), PT_MORPH_MAX_TARGETS);
    """ + "".join(f'  printf(" %zu", offsetof(PTMorphDesc, {f}));\n' for f in fields) + "  return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    D = abi.PTMorphDesc
    assert got[:4] == [72, 16, 12, abi.PT_MORPH_MAX_TARGETS]
    assert C.sizeof(D) == 72 and C.sizeof(abi.PTMorphEntry) == 16 and abi.MORPH_ENTRY.itemsize == 16 and abi.MORPH_ENTRY.fields["target"][1] == 12
    assert got[4:] == [getattr(D, f).offset for f in fields]


def case(ntri, target_count, pattern):
    """rest, the three streams, weights, rest attributes, a skin and a palette for one case"""
    n = ntri * 3
    seed = 1000 * ntri + target_count
    rest = soup(ntri, 300 + ntri)
    streams = [morph_cases.stream(n, target_count, pattern, seed + k, scale) for k, scale in enumerate((0.25, 0.5, 0.5))]
    attrs = skin_cases.rest_attrs(ntri, ntri, material_count=3)
    joints, sw = skin_cases.skin_of(rest, JOINTS, seed + 5)
    return rest, streams, morph_cases.weights(target_count, seed + 7), attrs, (joints, sw), skin_cases.palette(JOINTS, seed + 9)


@pytest.mark.parametrize("pattern", morph_cases.PATTERNS)
@pytest.mark.parametrize("target_count", TARGETS)
@pytest.mark.parametrize("ntri", TRIANGLES)
def test_host_twin_equals_the_restatement(ntri, target_count, pattern):
    rest, (pos, nrm, tan), w, attrs, skin, pal = case(ntri, target_count, pattern)
    for skinned in (False, True):
        sk, m = (skin, pal) if skinned else (None, None)
        want_v, want_a, want_b = morph_ref.morph(rest, pos, w, nrm, tan, attrs, sk, m)
        got_v, got_a, got_b = plugin.morph_vertices(rest, pos, w, nrm, tan, attrs, sk, m)
        assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), skinned
        assert got_a.tobytes() == want_a.tobytes(), skinned
        assert got_b.tobytes() == want_b.tobytes(), skinned
        assert (got_v[:, 3] == 0).all()
        if pattern == "empty" and not skinned:               # nothing listed, no palette: the rest bytes (w = 0 apart)
            assert got_v[:, :3].tobytes() == rest[:, :3].tobytes() and got_a.tobytes() == attrs.tobytes()
        # a position stream alone, no rest attributes: the same positions, no records
        v2, a2, b2 = plugin.morph_vertices(rest, pos, w, skin=sk, joint_matrices=m)
        assert a2 is None and v2.tobytes() == want_v.tobytes() and b2.tobytes() == want_b.tobytes()
    # a skin without a palette is a plain morph
    v3, _, _ = plugin.morph_vertices(rest, pos, w, skin=skin)
    assert v3.tobytes() == morph_ref.morph(rest, pos, w)[0].tobytes()


def test_only_one_of_the_attribute_streams():
    rest, (pos, nrm, tan), w, attrs, skin, pal = case(22, 3, "random")
    for n_, t_ in ((nrm, None), (None, tan)):
        want = morph_ref.morph(rest, pos, w, n_, t_, attrs)
        got = plugin.morph_vertices(rest, pos, w, n_, t_, attrs)
        assert got[1].tobytes() == want[1].tobytes()
        untouched = slice(12, 24) if t_ is None else slice(0, 12)            # the rows of the stream that is absent
        assert got[1].view(np.float32).reshape(-1, 32)[:, untouched].tobytes() == attrs.view(np.float32).reshape(-1, 32)[:, untouched].tobytes()


def test_a_direction_that_cannot_be_normalised_keeps_the_rest_vector():
    rest, (pos, _, _), w, attrs, skin, pal = case(4, 3, "dense")
    n = 12
    off = np.zeros(n + 1, np.uint32)
    off[3:] = 1                                              # corner 2 alone lists target 1: the delta that cancels its normal
    ent = np.zeros(1, abi.MORPH_ENTRY)
    w = np.array([0.5, 1.0, 0.25], np.float32)
    rows = attrs.view(np.float32).reshape(-1, 8, 4)
    rows[0, 2, :3] = (0.5, -0.25, 0.125)                    # exact in binary32: rest + 1 * (-rest) is +0
    ent["dx"], ent["dy"], ent["dz"], ent["target"] = -0.5, 0.25, -0.125, 1
    for sk, m in ((None, None), (skin, pal)):
        got = plugin.morph_vertices(rest, pos, w, (off, ent), None, attrs, sk, m)[1]
        assert got.view(np.float32).reshape(-1, 8, 4)[0, 2, :3].tobytes() == rows[0, 2, :3].tobytes(), m is not None
        assert got.tobytes() == morph_ref.morph(rest, pos, w, (off, ent), None, attrs, sk, m)[1].tobytes()


# ---- dense deltas to CSR ----
def test_dense_to_csr_drops_exact_positive_zero_triples_only():
    d = np.zeros((3, 6, 3), np.float32)
    d[0, 0] = (1, 0, 0)
    d[2, 0] = (0, 0, 2)
    d[1, 1] = (0, -0.0, 0)                                   # a -0 component: listed
    d[1, 2] = (np.nan, 0, 0)
    d[0, 4] = (0, 0, 0)                                      # dropped
    d[2, 5] = (0, 3, 0)
    off, ent = plugin.morph_csr(d)
    assert off.tolist() == [0, 2, 3, 4, 4, 4, 5] and off.dtype == np.uint32 and ent.dtype == abi.MORPH_ENTRY
    assert ent["target"].tolist() == [0, 2, 1, 1, 2]
    assert ent["dz"][1] == 2 and np.signbit(ent["dy"][2]) and np.isnan(ent["dx"][3]) and ent["dy"][4] == 3
    back = morph_cases.dense((off, ent), 3)
    assert np.array_equal(back.view(np.uint32), d.view(np.uint32))        # what was dropped was +0 in every bit


def test_all_zero_weights_on_a_dense_morph():
    """Zero weights give the rest POSITIONS: acc + 0 * d is acc for finite d (a rest coordinate of -0 apart: -0 + +0 is +0, and the
    soup has none).  They do not give the rest BYTES of a normal that is not unit length: a corner that lists an entry is
    renormalised, m * (1 / sqrt(dot(m, m))), whatever the weights are -- only a corner that lists nothing is copied."""
    ntri, K = 22, 3
    rest = soup(ntri, 9)
    rng = np.random.RandomState(4)
    dense_p = rng.uniform(-1, 1, (K, ntri * 3, 3)).astype(np.float32)
    dense_n = rng.uniform(-1, 1, (K, ntri * 3, 3)).astype(np.float32)
    attrs = skin_cases.rest_attrs(ntri, 2)
    rows = attrs.view(np.float32).reshape(-1, 8, 4)
    rows[:, :3, :3] *= np.float32(3.0)                       # normals of length 3
    w = np.zeros(K, np.float32)
    got_v, got_a, _ = plugin.morph_vertices(rest, dense_p, w, dense_n, None, attrs)
    assert got_v[:, :3].tobytes() == rest[:, :3].tobytes()
    out = got_a.view(np.float32).reshape(-1, 8, 4)
    assert not np.array_equal(out[:, :3, :3], rows[:, :3, :3])
    assert np.abs(np.linalg.norm(out[:, :3, :3].astype(np.float64), axis=2) - 1).max() < 1e-6
    assert got_a.tobytes() == morph_ref.morph(rest, plugin.morph_csr(dense_p), w, plugin.morph_csr(dense_n), None, attrs)[1].tobytes()
    # ... and the tangents, whose stream is absent, are the rest bytes
    assert out[:, 3:].tobytes() == rows[:, 3:].tobytes()


# ---- the device layout ----
@pytest.mark.parametrize("pattern", morph_cases.PATTERNS)
@pytest.mark.parametrize("ntri,target_count", [(1, 1), (21, 3), (22, 64), (86, 5), (300, 64)])
def test_layout_round_trips_and_never_reads_padding(ntri, target_count, pattern):
    n = ntri * 3
    off, ent = morph_cases.stream(n, target_count, pattern, 5 * ntri + target_count)
    ent["target"] += 1                                       # no listed entry is all zero bytes: padding can be told apart
    count, base, stored = plugin.morph_layout(off, ent)
    slices = (n + 63) // 64
    assert count.tolist() == np.diff(off.astype(np.int64)).tolist() and base.shape == (slices + 1,) and base[0] == 0 and base[-1] == len(stored)
    longest = [int(count[k * 64:(k + 1) * 64].max()) for k in range(slices)]
    assert np.diff(base.astype(np.int64)).tolist() == [64 * m for m in longest]
    if pattern == "dense":
        assert len(stored) == 64 * target_count * slices     # only the last slice's missing corners are padding
    # what a lane reads under the rule s < count: the CSR it came from, in order
    back, used = [], np.zeros(len(stored), bool)
    for c in range(n):
        idx = int(base[c // 64]) + 64 * np.arange(int(count[c])) + c % 64
        assert (idx < int(base[c // 64 + 1])).all()
        used[idx] = True
        back.append(stored[idx])
    assert np.concatenate(back).tobytes() == ent.tobytes()
    assert used.sum() == len(ent) and not stored[~used].view(np.uint32).any()        # every other slot is padding, all zero


# ---- refusals, one test each ----
def refusal_case():
    rest, (pos, nrm, tan), w, attrs, skin, pal = case(10, 4, "random")
    return rest, pos, nrm, w, attrs, skin, pal


def listed_corner(stream, at_least=1):
    return int(np.nonzero(np.diff(stream[0].astype(np.int64)) >= at_least)[0][0])


@pytest.mark.parametrize("target_count", [0, 1025])
def test_refused_target_count(target_count):
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    empty = (np.zeros(31, np.uint32), np.zeros(0, abi.MORPH_ENTRY))
    with pytest.raises(plugin.PluginError, match="targetCount"):
        plugin.morph_vertices(rest, empty, np.zeros(target_count, np.float32), target_count=target_count)


def test_refused_target_out_of_range():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    ent = pos[1].copy()
    ent["target"][-1] = 4
    with pytest.raises(plugin.PluginError, match="target 4 >= targetCount"):
        plugin.morph_vertices(rest, (pos[0], ent), w)


def test_refused_targets_not_ascending():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    c = listed_corner(pos, 2)
    ent = pos[1].copy()
    ent["target"][pos[0][c] + 1] = ent["target"][pos[0][c]]              # equal is not strictly ascending
    with pytest.raises(plugin.PluginError, match="ascending"):
        plugin.morph_vertices(rest, (pos[0], ent), w)


def test_refused_offsets_decreasing():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    off = pos[0].copy()
    c = listed_corner(pos)
    off[c + 1], off[c] = off[c], off[c + 1]
    with pytest.raises(plugin.PluginError, match="offsets decrease"):
        plugin.morph_vertices(rest, (off, pos[1]), w)


def test_refused_first_offset_not_zero():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    off = pos[0].copy()
    off[0] = 1
    with pytest.raises(plugin.PluginError, match=r"offsets\[0\] != 0"):
        plugin.morph_vertices(rest, (off, pos[1]), w)


def test_refused_non_finite_delta():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    ent = nrm[1].copy()
    ent["dz"][2] = np.inf
    with pytest.raises(plugin.PluginError, match="normal stream: the delta of entry 2 is not finite"):
        plugin.morph_vertices(rest, pos, w, (nrm[0], ent), None, attrs)


def test_refused_non_finite_weight():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    bad = w.copy()
    bad[3] = np.nan
    with pytest.raises(plugin.PluginError, match="morph weight 3 is not finite"):
        plugin.morph_vertices(rest, pos, bad)


def test_refused_non_finite_matrix():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    bad = pal.copy()
    bad[3, 7] = np.nan
    with pytest.raises(plugin.PluginError, match="joint matrix 3 is not finite"):
        plugin.morph_vertices(rest, pos, w, skin=skin, joint_matrices=bad)
    with pytest.raises(plugin.PluginError, match="a palette needs a skin"):
        plugin.morph_vertices(rest, pos, w, joint_matrices=pal)


def test_refused_non_finite_rest_vertex():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    bad = rest.copy()
    bad[4, 0] = np.inf
    with pytest.raises(plugin.PluginError, match="rest vertex 4"):
        plugin.morph_vertices(bad, pos, w)


def test_refused_normal_stream_without_rest_attrs():
    rest, pos, nrm, w, attrs, skin, pal = refusal_case()
    with pytest.raises(plugin.PluginError, match="needs restAttrs"):
        plugin.morph_vertices(rest, pos, w, nrm)
    plugin.morph_vertices(rest, pos, w, nrm, None, attrs)


# ---- GLB morph targets and animations ----
def glb_morph(mesh, K=3, seed=0, sparse=False):
    """Per-vertex targets for a test_skin.glb_case mesh: POSITION, NORMAL and TANGENT deltas, most rows of the later targets zero"""
    rng = np.random.RandomState(seed)
    n = len(mesh.positions)
    out = {}
    for key in ("position", "normal", "tangent"):
        d = rng.uniform(-0.3, 0.3, (K, n, 3)).astype(np.float32)
        d[1:, rng.uniform(size=n) < 0.7] = 0.0
        out[key] = d
    out["weights"] = np.linspace(0.25, 0.75, K).astype(np.float32)
    out["sparse"] = sparse
    return out


@pytest.mark.parametrize("sparse", [False, True])
def test_glb_morph_round_trip(tmp_path, sparse):
    mesh, skin = glb_case()
    plain = ingest.Mesh(positions=mesh.positions[::-1].copy(), normals=None, tangents=None, uvs=None, indices=None, local_to_world=np.eye(4), material_index=0, name="plain")
    morph = glb_morph(mesh, sparse=sparse)
    path = str(tmp_path / "morphed.glb")
    ingest.write_glb(path, [plain, mesh], skins=[None, skin], morphs=[None, morph])
    meshes, _, _ = ingest.load_glb(path, unity_handedness=False, load_images=False)
    got = ingest.load_glb_morphs(path, unity_handedness=False)
    assert len(got) == len(meshes) == 2 and got[0] is None
    ix = mesh.indices.astype(np.int64)
    for key in ("position", "normal", "tangent"):
        assert got[1][key].dtype == np.float32 and np.array_equal(got[1][key], morph[key][:, ix]), key
    assert np.array_equal(got[1]["weights"], morph["weights"]) and got[1]["weights"].dtype == np.float32
    assert np.array_equal(soup_of(meshes[1]), soup_of(mesh))
    # the skin of the same file is read as before
    assert np.array_equal(ingest.load_glb_skins(path, unity_handedness=False)[1]["joints"], skin["joints"][ix])
    if sparse:
        import json
        import struct
        raw = open(path, "rb").read()
        doc = json.loads(raw[20:20 + struct.unpack_from("<I", raw, 12)[0]])
        target = [doc["accessors"][a] for t in doc["meshes"][1]["primitives"][0]["targets"] for a in t.values()]
        assert all("bufferView" not in a for a in target) and all(a["sparse"]["count"] < a["count"] for a in target[3:])


def test_glb_morph_defaults(tmp_path):
    """Only POSITION targets and no mesh weights: normal / tangent are None, the default weights are zeros"""
    mesh, _ = glb_case()
    morph = {"position": glb_morph(mesh)["position"]}
    path = str(tmp_path / "morphed.glb")
    ingest.write_glb(path, [mesh], morphs=[morph])
    got = ingest.load_glb_morphs(path)[0]
    assert got["normal"] is None and got["tangent"] is None and got["position"].shape == (3, len(mesh.indices), 3)
    assert np.array_equal(got["weights"], np.zeros(3, np.float32))


def test_write_glb_without_morphs_or_animations_is_unchanged(tmp_path):
    mesh, skin = glb_case()
    a, b, c = (str(tmp_path / n) for n in ("a.glb", "b.glb", "c.glb"))
    ingest.write_glb(a, [mesh], skins=[skin])
    ingest.write_glb(b, [mesh], skins=[skin], morphs=None, animations=None)
    ingest.write_glb(c, [mesh], skins=[skin], morphs=[None], animations=[])
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def test_glb_morph_handedness_is_applied_consistently(tmp_path):
    """The morphed mesh of the mirrored arrays is the mirror image, with reversed winding, of the right-handed result"""
    mesh, _ = glb_case(2)
    morph = glb_morph(mesh, seed=3)
    path = str(tmp_path / "morphed.glb")
    ingest.write_glb(path, [mesh], morphs=[morph])
    w = np.array([0.7, -0.3, 1.2], np.float32)
    out = {}
    for handed in (False, True):
        meshes, _, _ = ingest.load_glb(path, unity_handedness=handed, load_images=False)
        g = ingest.load_glb_morphs(path, unity_handedness=handed)[0]
        out[handed], _, _ = plugin.morph_vertices(soup_of(meshes[0]), g["position"], w)
        listed = len(plugin.morph_csr(g["position"])[1])
        assert 0 < listed == int((morph["position"][:, mesh.indices.astype(np.int64)] != 0).any(axis=2).sum())      # a zero row stays unlisted under the mirror
    assert np.abs(out[False][:, :3] - soup_of(mesh)[:, :3]).max() > 0.1        # a non-trivial morph
    want = out[False].reshape(-1, 3, 4)[:, ::-1].reshape(-1, 4) * np.array([1, 1, -1, 1], np.float32)      # mirrored z, reversed winding
    assert np.array_equal(out[True], want)                   # negating one component commutes with every operation of the rule


def quaternion(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])


def multiply(a, b):
    """The quaternion product a b, (x, y, z, w)"""
    av, bv = a[:3], b[:3]
    return np.concatenate([a[3] * bv + b[3] * av + np.cross(av, bv), [a[3] * b[3] - np.dot(av, bv)]])


def rotation_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def clip_case():
    """glb_case with two targets and one animation: joint 1 turns about a fixed axis (LINEAR), joint 2 moves (LINEAR), joint 3 is
    scaled (STEP), the mesh's weights are keyed (LINEAR).  Times 0.5, 1, 2; float32-exact values where the test compares exactly."""
    mesh, skin = glb_case(4)
    morph = glb_morph(mesh, K=2, seed=6)
    times = np.array([0.5, 1.0, 2.0])
    axis = np.array([1.0, 2.0, -0.5])
    q = np.stack([quaternion(axis, a) for a in (0.2, 1.1, 2.6)])
    channels = [dict(node=("joint", 0, 1), path="rotation", interpolation="LINEAR", times=times, values=q),
                dict(node=("joint", 0, 2), path="translation", interpolation="LINEAR", times=times, values=np.array([[0, 0, 0], [1, 2, 4], [3, -2, 0.5]])),
                dict(node=("joint", 0, 3), path="scale", interpolation="STEP", times=times, values=np.array([[1, 1, 1], [2, 2, 2], [0.5, 0.5, 0.5]])),
                dict(node=0, path="weights", interpolation="LINEAR", times=times, values=np.array([[0, 1], [0.5, 0.25], [1, 0]]))]
    return mesh, skin, morph, dict(name="clip", channels=channels), axis


def test_glb_animation_round_trip(tmp_path):
    mesh, skin, morph, anim, _ = clip_case()
    path = str(tmp_path / "clip.glb")
    ingest.write_glb(path, [mesh], skins=[skin], morphs=[morph], animations=[anim])
    got = ingest.load_glb_animations(path, unity_handedness=False)
    assert len(got) == 1 and got[0]["name"] == "clip" and got[0]["duration"] == 2.0
    first = 1                                                # node 0 is the mesh, the six joints follow
    assert [(c["node"], c["path"], c["interpolation"]) for c in got[0]["channels"]] == \
        [(first + 1, "rotation", "LINEAR"), (first + 2, "translation", "LINEAR"), (first + 3, "scale", "STEP"), (0, "weights", "LINEAR")]
    for c, want in zip(got[0]["channels"], anim["channels"]):
        assert np.array_equal(c["times"], want["times"]) and c["values"].dtype == np.float64
        assert np.array_equal(c["values"], np.asarray(want["values"], np.float32).astype(np.float64))         # stored as float32
    assert got[0]["primitives"][0]["joints"] == list(range(first, first + 6)) and np.array_equal(got[0]["primitives"][0]["weights"], morph["weights"].astype(np.float64))
    # the rest pose comes back: a joint written as translation / rotation / scale is its matrix
    rest = ingest.load_glb_skins(path, unity_handedness=False)[0]
    assert np.allclose(rest["local"], skin["local"], rtol=0, atol=1e-12)


def test_sample_animation(tmp_path):
    mesh, skin, morph, anim, axis = clip_case()
    path = str(tmp_path / "clip.glb")
    ingest.write_glb(path, [mesh], skins=[skin], morphs=[morph], animations=[anim])
    a = ingest.load_glb_animations(path, unity_handedness=False)[0]
    g = ingest.load_glb_skins(path, unity_handedness=False)[0]
    q = a["channels"][0]["values"]                           # as stored (float32): what the sampler interpolates
    q = q / np.linalg.norm(q, axis=1, keepdims=True)

    def expect(rot, trans, scale):
        """the six joints' local matrices with joints 1, 2 and 3 animated"""
        local = np.array(g["local"], copy=True)
        s1 = np.linalg.norm(local[1, :3, :3], axis=0)
        local[1, :3, :3] = rotation_of(rot) * s1[None, :]
        local[2, :3, 3] = trans
        r3 = local[3, :3, :3] / np.linalg.norm(local[3, :3, :3], axis=0)
        local[3, :3, :3] = r3 * np.asarray(scale)[None, :]
        return local

    def close(got, want):
        assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()

    # at the keyframes
    for k, t in enumerate((0.5, 1.0, 2.0)):
        s = ingest.sample_animation(a, t)
        close(s["local"][0], expect(q[k], anim["channels"][1]["values"][k], anim["channels"][2]["values"][k]))
        assert np.array_equal(s["weights"][0], anim["channels"][3]["values"][k])
    # at the midpoints: slerp against the closed form q0 (q0^-1 q1)^u -- the relative rotation's angle scaled by u, about its own axis
    for k, t in ((0, 0.75), (1, 1.5)):
        s = ingest.sample_animation(a, t)
        rel = multiply(q[k] * np.array([-1, -1, -1, 1.0]), q[k + 1])
        rel = -rel if rel[3] < 0 else rel
        mid = multiply(q[k], quaternion(rel[:3], 0.5 * 2 * np.arctan2(np.linalg.norm(rel[:3]), rel[3])))
        values = [np.asarray(c["values"], np.float64) for c in anim["channels"]]
        close(s["local"][0], expect(mid, 0.5 * (values[1][k] + values[1][k + 1]), values[2][k]))              # STEP: the earlier key
        close(s["weights"][0], 0.5 * (values[3][k] + values[3][k + 1]))
    # outside the clip: clamped
    for t, k in ((-1.0, 0), (0.0, 0), (2.5, 2), (1e9, 2)):
        s = ingest.sample_animation(a, t)
        close(s["local"][0], expect(q[k], anim["channels"][1]["values"][k], anim["channels"][2]["values"][k]))
        assert np.array_equal(s["weights"][0], anim["channels"][3]["values"][k])
    # what joint_matrices takes: the palette of the sampled pose moves the mesh
    pal = ingest.joint_matrices(g, ingest.sample_animation(a, 1.5)["local"][0])
    assert pal.shape == (6, 3, 4) and pal.dtype == np.float32
    # mirrored: M' = F M F, the weights are the same
    h = ingest.load_glb_animations(path, unity_handedness=True)[0]
    flip = np.diag([1.0, 1.0, -1.0, 1.0])
    sh, sr = ingest.sample_animation(h, 1.5), ingest.sample_animation(a, 1.5)
    close(sh["local"][0], flip @ sr["local"][0] @ flip)
    assert np.array_equal(sh["weights"][0], sr["weights"][0])


def test_slerp_takes_the_shorter_arc():
    a, b = quaternion((0, 0, 1), 0.4), -quaternion((0, 0, 1), 1.0)          # -q is the same rotation as q
    ch = dict(path="rotation", interpolation="LINEAR", times=np.array([0.0, 1.0]), values=np.stack([a, b]))
    got = ingest._sample_channel(ch, 0.25)
    assert np.abs(got - quaternion((0, 0, 1), 0.55)).max() <= 1e-12


def test_cubicspline_raises(tmp_path):
    mesh, skin, morph, anim, _ = clip_case()
    ch = anim["channels"][1]
    ch["interpolation"] = "CUBICSPLINE"
    ch["values"] = np.repeat(ch["values"], 3, axis=0)        # in-tangent, value, out-tangent per key
    path = str(tmp_path / "clip.glb")
    ingest.write_glb(path, [mesh], skins=[skin], morphs=[morph], animations=[anim])
    a = ingest.load_glb_animations(path)[0]                  # read as data
    assert a["channels"][1]["interpolation"] == "CUBICSPLINE" and a["channels"][1]["values"].shape == (9, 3)
    with pytest.raises(NotImplementedError, match="CUBICSPLINE"):
        ingest.sample_animation(a, 1.0)


# ---- the kernels' resources and the sanitizers ----
VGPRS = {"pt_morph_verticesILb0": 36, "pt_morph_verticesILb1": 64, "pt_morph_attrsILb0": 38, "pt_morph_attrsILb1": 67}      # what the build shows


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_morph_kernel_resources():
    res = resources("pt_morph.hip")
    kernels = {name: r for k, r in res.items() for name in VGPRS if name in k}
    assert len(kernels) == 4 == len(res), list(res)
    for k, r in kernels.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
    assert {k: r["vgprs"] for k, r in kernels.items()} == VGPRS, kernels


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_host_twin_under_sanitizers(tmp_path):
    """`make morph-sanitize`: the host twin and csrc/morph_sanitize_main.cpp (its own main) with -fsanitize=address,undefined, built
    and run -- it morphs and skins a generated mesh, checks the result and the device layout and makes the refusals, and must
    finish without a report."""
    csrc = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "morph-sanitize", "MORPH_SANITIZE_OUT=" + str(tmp_path / "morph_sanitize")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "morph ok" in out.stdout, out.stdout + out.stderr
