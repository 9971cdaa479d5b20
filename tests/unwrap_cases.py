"""Meshes for the unwrap tests (include/ptmi_plugin.h Part 23): every case is (vertices, scene_vertices, charts) -- (3T, 4) float32
in primitive order as the caller's vertex array takes them, the same mesh with whatever a BVH builder cannot take (a NaN, a lone
degenerate triangle) replaced, for the tests that build a scene, and the number of charts the vertex form must find (None: not
stated).  records() makes triangle rows from vertices the way a builder stores them, in a shuffled record order."""
import numpy as np

from unity_webgpu_pathtracer_amd import scenes

F = np.float32


def _mesh(tris):
    v = np.zeros((len(tris) * 3, 4), F)
    v[:, :3] = np.asarray(tris, F).reshape(-1, 3)
    return v


def records(vertices, seed=3):
    """(3T, 4) float32 rows e2, e1, v0 + primIdx per record, the records in a fixed random order"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3, 4)
    T = len(v)
    order = np.random.default_rng(seed).permutation(T)
    rows = np.zeros((T, 3, 4), F)
    with np.errstate(all="ignore"):
        rows[:, 0, :3] = v[order, 2, :3] - v[order, 0, :3]
        rows[:, 1, :3] = v[order, 1, :3] - v[order, 0, :3]
    rows[:, 2, :3] = v[order, 0, :3]
    rows[:, 2, 3] = order.astype(np.uint32).view(F)
    return rows.reshape(-1, 4)


def _quad(o, du, dv):
    o, du, dv = (np.asarray(x, np.float64) for x in (o, du, dv))
    return [(o, o + du, o + du + dv), (o, o + du + dv, o + dv)]


def cube():
    t = []
    t += _quad((0, 0, 0), (0, 2, 0), (2, 0, 0)) + _quad((0, 0, 2), (2, 0, 0), (0, 2, 0))          # -z, +z
    t += _quad((0, 0, 0), (2, 0, 0), (0, 0, 2)) + _quad((0, 2, 0), (0, 0, 2), (2, 0, 0))          # -y, +y
    t += _quad((0, 0, 0), (0, 0, 2), (0, 2, 0)) + _quad((2, 0, 0), (0, 2, 0), (0, 0, 2))          # -x, +x
    return _mesh(t)


def grid(nx, ny, step=0.37, cut=None, tilt=0.3):
    """a tessellated quad of 2 nx ny triangles in a tilted plane (one class), cut to `cut` triangles: one chart"""
    pt = lambda i, j: (i * step, j * step, tilt * (i * step) + 0.1 * (j * step))          # one value per grid point, whoever uses it
    t = []
    for j in range(ny):
        for i in range(nx):
            t += [(pt(i, j), pt(i + 1, j), pt(i + 1, j + 1)), (pt(i, j), pt(i + 1, j + 1), pt(i, j + 1))]
    return _mesh(t[:cut])


def strip(n, permute_seed=None):
    """n triangles in a row, each linked to the next only; with a seed the primitives are a fixed random permutation"""
    t = []
    for i in range(n):
        x = i // 2
        a, b, c, d = (x, 0, 1), (x + 1, 0, 1), (x + 1, 1, 1), (x, 1, 1)
        t.append((a, b, d) if i % 2 == 0 else (b, c, d))
    v = _mesh(t).reshape(n, 3, 4)
    if permute_seed is not None:
        v = v[np.random.default_rng(permute_seed).permutation(n)]
    return v.reshape(-1, 4).copy()


def fan(n):
    """n triangles around one vertex, in one plane"""
    ang = np.linspace(0.0, 1.9 * np.pi, n + 1)
    rim = [(np.cos(a), 0.25, np.sin(a)) for a in ang]
    return _mesh([((0, 0.25, 0), rim[i + 1], rim[i]) for i in range(n)])


def instanced_mesh(mesh=0):
    s = scenes.instanced_scene()
    t0, nt = s.mesh_ranges[mesh]
    return s.vertices[t0 * 3:(t0 + nt) * 3].copy()


def small_cases():
    """name -> (vertices, scene_vertices, charts)"""
    one = _mesh([((0, 0, 0), (1, 0, 0), (0, 1, 0))])
    degenerate = _mesh([((0, 0, 0), (1, 0, 0), (1, 0, 0))])
    nan = one.copy()
    nan[1, 1] = np.nan
    # two triangles on the edge (0,0,0)-(1,0,0): in one plane, and folded by 90 degrees
    a, b = (0, 0, 0), (1, 0, 0)
    same = [(a, b, (0, 1, 0)), (b, a, (1, -1, 0))]
    folded = [(a, b, (0, 1, 0)), (b, a, (1, 0, 1))]
    flip = lambda t: (t[0], t[2], t[1])
    # three on one edge: two of a class, the odd one between them in primitive order
    three = [(a, b, (0, 1, 0)), (b, a, (1, 0, 1)), (b, a, (1, -1, 0))]
    zero = _mesh(same)
    zero[0, 1] = F(-0.0)                                                # corner a of the first triangle: y = -0
    zero[4, 2] = F(-0.0)                                                # corner a of the second: z = -0
    out = {
        "one": (one, one, 1),
        "degenerate": (degenerate, one, 0),
        "nan-corner": (nan, one, 0),
        "pair-same-class": (_mesh(same), None, 1),
        "pair-two-classes": (_mesh(folded), None, 2),
        "pair-same-class-opposite-winding": (_mesh([same[0], flip(same[1])]), None, 2),
        "pair-two-classes-opposite-winding": (_mesh([folded[0], flip(folded[1])]), None, 2),
        "three-on-an-edge": (_mesh(three), None, 2),
        "signed-zero": (zero, None, 1),
        "cube": (cube(), None, 6),
        "strip-300": (strip(300), None, 1),
        "fan-65": (fan(65), None, 1),
        "strip-4096-permuted": (strip(4096, permute_seed=11), None, 1),
    }
    return {k: (v, v if sv is None else sv, n) for k, (v, sv, n) in out.items()}


def scene_cases():
    zoo = scenes.material_zoo().vertices
    inst = instanced_mesh(0)
    return {"material-zoo": (zoo, zoo, 54), "instanced-mesh-0": (inst, inst, None)}


CUT_SIZES = (63, 64, 65, 256, 257)


def cut_cases():
    return {f"grid-{n}": (grid(16, 9, cut=n), grid(16, 9, cut=n), 1) for n in CUT_SIZES}
