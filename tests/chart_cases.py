"""Meshes, charts and scenes for the lightmap tests (test_lightmap.py, test_gpu_lightmap.py): the unit quad, a zoo of about 60
triangles with everything the rasterisation rule has a sentence for, an instance matrix, and the scenes that carry them."""
from dataclasses import replace

import numpy as np

from unity_webgpu_pathtracer_amd import abi, plugin, scenes

F = np.float32
QUAD_SIZES = [(1, 1), (7, 5), (64, 64), (130, 67)]
ZOO_SIZES = [(37, 23), (64, 64)]
WRAP_SEED = 0xFFFFFFF0

# the floor quad origin + u * eu + v * ev of extent 2
QUAD_ORIGIN, QUAD_EU, QUAD_EV, QUAD_NORMAL = (-1.0, 0.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.0, 1.0, 0.0)


def quad_mesh():
    """(vertices (6, 4) float32, attrs (2,) abi.TRI_ATTR): two triangles whose UVs are the whole unit square"""
    sb = scenes.SoupBuilder()
    sb.quad(QUAD_ORIGIN, QUAD_EU, QUAD_EV, QUAD_NORMAL, 1, 1, 0)
    return sb.finish()


# primitive numbers of the zoo's special triangles
OVER_A, OVER_B = 0, 1                   # two overlapping triangles: the lowest primitive numbers, so 0 owns every shared texel
ZERO_AREA_UV, FLAT_IN_SPACE, NAN_UV, PARTLY_OUT, WHOLLY_OUT, TOO_FAR, SUB_TEXEL, ZERO_NORMAL = 2, 3, 4, 5, 6, 7, 8, 9
GRID0 = 10                              # then 5 x 5 cells of two triangles
BIG = GRID0 + 50                        # the last one: it fills what the others leave of the half u + v < 0.9
ZOO_TRIANGLES = BIG + 1


def _surface(uv):
    """a wavy sheet over the unit square: position of a UV"""
    u, v = uv[..., 0], uv[..., 1]
    return np.stack([2.0 * u - 1.0, 0.3 * np.sin(3.0 * u) * np.cos(2.0 * v), 2.0 * v - 1.0], axis=-1)


def zoo_mesh(seed=11):
    """-> (vertices (3T, 4) float32, attrs (T,) abi.TRI_ATTR with the chart in uv0 .. uv2, caller_uvs (T, 6) float32).  The attribute
    UVs are all finite (a scene takes them); the caller's UVs are the same chart with u and v swapped -- every winding mirrored --
    and a NaN in triangle NAN_UV."""
    rng = np.random.RandomState(seed)
    T = ZOO_TRIANGLES
    uv = np.zeros((T, 3, 2))
    uv[OVER_A] = [(0.56, 0.06), (0.96, 0.08), (0.58, 0.46)]
    uv[OVER_B] = [(0.60, 0.04), (0.98, 0.10), (0.57, 0.44)]
    uv[ZERO_AREA_UV] = [(0.1, 0.1), (0.2, 0.2), (0.3, 0.3)]
    uv[FLAT_IN_SPACE] = [(0.1, 0.6), (0.3, 0.6), (0.2, 0.8)]
    uv[NAN_UV] = [(0.05, 0.9), (0.15, 0.9), (0.1, 0.97)]
    uv[PARTLY_OUT] = [(-0.2, 0.3), (0.1, 0.35), (-0.1, 0.5)]
    uv[WHOLLY_OUT] = [(1.5, 1.5), (1.8, 1.5), (1.6, 1.9)]
    uv[TOO_FAR] = [(0.3, 0.3), (5000.0, 0.3), (0.3, 0.4)]
    uv[SUB_TEXEL] = [(0.0005, 0.0005), (0.002, 0.0006), (0.001, 0.002)]
    uv[ZERO_NORMAL] = [(0.88, 0.55), (0.99, 0.6), (0.9, 0.7)]
    k = GRID0
    for i in range(5):
        for j in range(5):
            c = np.array([0.05 + 0.16 * i, 0.05 + 0.16 * j])
            q = [c, c + (0.16, 0.0), c + (0.16, 0.16), c + (0.0, 0.16)]
            jit = rng.uniform(-0.004, 0.004, 2)                         # the shared diagonal moves with both triangles
            q[0], q[2] = q[0] + jit, q[2] - jit
            for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                uv[k] = tri if k % 3 else tri[::-1]                     # every third one mirrored
                k += 1
    uv[BIG] = [(-0.1, -0.1), (1.0, -0.1), (-0.1, 1.0)]
    pos = _surface(uv)
    pos[FLAT_IN_SPACE, 2] = pos[FLAT_IN_SPACE, 1]                       # two corners at one point: no area in space
    verts = np.zeros((T * 3, 4), F)
    verts[:, :3] = pos.reshape(-1, 3)
    attrs = np.zeros(T, abi.TRI_ATTR)
    for c in range(3):
        n = rng.normal(size=(T, 3)) * 0.4 + (0.0, 1.0, 0.0)
        attrs[f"normal{c}"] = n / np.linalg.norm(n, axis=1, keepdims=True)
        attrs[f"tangent{c}"] = (1.0, 0.0, 0.0)
        attrs[f"uv{c}"] = uv[:, c]
    for c in range(3):
        attrs[f"normal{c}"][ZERO_NORMAL] = 0.0
    caller = uv[:, :, ::-1].astype(F).reshape(T, 6).copy()
    caller[NAN_UV, 2] = np.nan
    return verts, attrs, caller


def instance_matrix():
    """localToWorld with a rotation about two axes and a non-uniform scale, and its inverse: (l2w, w2l) as 16 float32 each in
    PTGpuInstance's memory order (element (r, c) at c * 4 + r)"""
    m = scenes._trs((0.5, 1.0, -0.3), 40.0, 25.0, (1.3, 0.7, 0.9))
    return m.T.reshape(16).astype(F), np.linalg.inv(m).T.reshape(16).astype(F), m


def blas_of(vertices):
    """the triangle rows of BuildBVH's CWBVH over the vertices: the records in the tree's order, each with its primIdx"""
    return plugin.build_cwbvh(vertices)[1]


def flat_scene(vertices, attrs, lights=(), name="chart_flat"):
    """One mesh as a flat scene: one white material, a black constant sky"""
    mats = np.stack([scenes.pack_material(color=(0.8, 0.8, 0.8, 1.0), roughness=1.0)])
    L = np.stack(lights).astype(F) if len(lights) else np.zeros((0, 16), F)
    return scenes.Scene(name, vertices, attrs, mats, L, np.zeros(0, np.uint32), scenes.Camera(eye=(0.0, 3.0, -4.0), target=(0.0, 0.0, 0.0)),
                        environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0), environment_intensity=0.0)


def instanced_with(meshes):
    """scenes.instanced_scene() with the meshes [(vertices, attrs), ...] appended, each with one rotated and non-uniformly scaled
    instance (instance_matrix).  -> (scene, [(mesh index, instance index), ...])"""
    base = scenes.instanced_scene(count=5, detail=4)
    verts, attrs = [base.vertices], [base.tri_attrs]
    ranges, instances, where = list(base.mesh_ranges), list(base.instances), []
    start = base.vertices.shape[0] // 3
    for v, a in meshes:
        a = a.copy()
        a["materialIndex"] = 0
        ranges.append((start, len(a)))
        start += len(a)
        instances.append((len(ranges) - 1, instance_matrix()[2], 0))
        where.append((len(ranges) - 1, len(instances) - 1))
        verts.append(v)
        attrs.append(a)
    return replace(base, vertices=np.concatenate(verts), tri_attrs=np.concatenate(attrs), mesh_ranges=ranges, instances=instances), where


def lit_box(emission=(6.0, 5.0, 3.0)):
    """A closed Cornell shell with a 1.2 x 1.2 emissive ceiling patch (an emissive material, no analytic light), every material of
    roughness 1, a black sky.  Its first two triangles are the floor quad, with the whole unit square as their UVs."""
    sb, mats = scenes.SoupBuilder(), []
    scenes._cornell_shell(sb, mats)
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1), 1, 1, 0)
    mats.append(scenes.pack_material(color=(0.5, 0.5, 0.5, 1.0), roughness=1.0, emission=emission))
    sb.quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0), 1, 1, 0)
    sb.quad((-0.6, 1.98, -0.6), (1.2, 0, 0), (0, 0, 1.2), (0, -1, 0), 1, 1, 3)
    verts, attrs = sb.finish()
    return scenes.Scene("chart_box", verts, attrs, np.stack(mats), np.zeros((0, 16), F), np.zeros(0, np.uint32),
                        scenes.Camera(eye=(0.0, 1.0, -0.9), target=(0.0, 1.0, 0.0)), environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0),
                        environment_intensity=0.0)


# Off centre in x and in z: a transposed or flipped axis moves the brightest texel.  High enough for every line from the floor
# through the light to leave by the open top (the render's shadow rays have no far end: one that reaches a wall behind the light
# is occluded): from the farthest texel centre the line passes the wall plane at 1.7 * 1.9375 / 1.3875 = 2.37 > 2.
LIGHT_POS = (0.45, 1.7, -0.35)


def open_box():
    """The same shell with its top open and one off-centre point light"""
    sb, mats = scenes.SoupBuilder(), []
    scenes._cornell_shell(sb, mats)
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1), 1, 1, 0)
    verts, attrs = sb.finish()
    light = scenes.pack_point_light(LIGHT_POS, (1.0, 0.8, 0.6), intensity=5.0, rng=10.0)
    return scenes.Scene("chart_open_box", verts, attrs, np.stack(mats), np.stack([light]).astype(F), np.zeros(0, np.uint32),
                        scenes.Camera(eye=(0.0, 1.0, -0.9), target=(0.0, 1.0, 0.0)), environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0),
                        environment_intensity=0.0), light


def floor_only_uvs(triangle_count):
    """caller UVs that keep the first two triangles (the floor quad's chart) and exclude every other triangle with a NaN"""
    uv = np.full((triangle_count, 6), np.nan, F)
    uv[0] = (0, 0, 1, 0, 1, 1)
    uv[1] = (0, 0, 1, 1, 0, 1)
    return uv
