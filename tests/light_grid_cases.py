"""The scenes, lights, grids and hand-made entries of the light-grid tests (include/ptmi_plugin.h Part 25), built here with
nothing from outside.  tests/test_light_grid.py and tests/test_gpu_light_grid.py import it the way the direct-light tests import
direct_cases.py.

The scene: an 8 x 8 floor at y = 0 over [0, 8]^2 with three boxes on it; 48 lights on a 6 x 8 lattice 1.2 above the floor with a
range of 1.5 -- point, spot pointing down, rectangle of 0.4 x 0.4 facing down, in turn, so that rectangle lights lie between the
lights a wave visits --, and among them one light without emission, one with a NaN position and one with an infinite range.  The
same lights, moved by (-4, 0, -4), stand over the floor of the instanced (HAS_TLAS) test scene."""
import numpy as np

from unity_webgpu_pathtracer_amd import scenes

F = np.float32
U = np.uint32
SPOT, DIRECTIONAL, POINT, RECTANGLE = 0, 1, 2, 3
W, H = 48, 32
RANGE = 1.5
HEIGHT = 1.2
DARK, NAN_P, INF_R = 10, 21, 32             # where the three special lights stand in the array

BOXES = (((1.2, 0.0, 1.4), (1.3, 0.8, 1.1)), ((4.1, 0.0, 4.6), (0.9, 1.6, 1.5)), ((5.6, 0.0, 1.1), (1.7, 0.5, 0.8)))     # (corner, size)


def lights(shift=(0.0, 0.0, 0.0), special=True):
    """(51, 16) float32 PTLight records; special=False: the three special lights are ordinary ones (what a bake can be made with)"""
    out, k = [], 0
    for iz in range(8):
        for ix in range(6):
            p = ((ix + 0.5) * 8.0 / 6.0, HEIGHT, iz + 0.5)
            colour = (6.0 + (k % 5), 5.0 + (k % 3), 4.0 + (k % 7))
            if k % 3 == 0:
                out.append(scenes.pack_point_light(p, colour, rng=RANGE))
            elif k % 3 == 1:
                out.append(scenes.pack_spot_light(p, (0.0, -1.0, 0.0), 120.0, 90.0, colour, intensity=2.0, rng=RANGE))
            else:
                out.append(scenes.pack_rect_light(center=p, right=(1, 0, 0), up=(0, 0, 1), size=(0.4, 0.4), color=colour, intensity=8.0, rng=RANGE))
            k += 1
    dark = scenes.pack_point_light((4.0, HEIGHT, 4.0), (0.0, 0.0, 0.0) if special else (1.0, 1.0, 1.0), rng=RANGE)
    nan_p = scenes.pack_point_light((np.nan if special else 1.0, HEIGHT, 3.0), (5.0, 5.0, 5.0), rng=RANGE)
    inf_r = scenes.pack_rect_light(center=(2.0, 2.5, 6.0), right=(1, 0, 0), up=(0, 0, 1), size=(0.4, 0.4), color=(0.4, 0.5, 0.6), rng=np.inf if special else RANGE)
    for at, rec in ((DARK, dark), (NAN_P, nan_p), (INF_R, inf_r)):
        out.insert(at, rec)
    L = np.stack(out).astype(F)
    L[:, 0:3] += np.asarray(shift, F)[None]
    return L


def grids(shift=(0.0, 0.0, 0.0)):
    """name -> (origin, cell size, dims): the grid over the floor, one over half of it (the rest takes the overflow cell), one cell"""
    s = np.asarray(shift, F)
    return {"full": (s + F(0), 1.0, (8, 2, 8)), "half": (s + np.array([0, 0, 0], F), 1.0, (4, 2, 8)), "one": (s + np.array([-0.5, -0.5, -0.5], F), 9.0, (1, 1, 1))}


INSTANCED_SHIFT = (-4.0, 0.0, -4.0)


def scene(special=True):
    sb = scenes.SoupBuilder()
    sb.quad((0, 0, 0), (0, 0, 8), (8, 0, 0), (0, 1, 0), 8, 8, 0)
    for m, ((x, y, z), (sx, sy, sz)) in enumerate(BOXES):
        sb.quad((x, y + sy, z), (0, 0, sz), (sx, 0, 0), (0, 1, 0), 2, 2, 1 + m)                   # top
        sb.quad((x, y, z), (sx, 0, 0), (0, sy, 0), (0, 0, -1), 2, 2, 1 + m)
        sb.quad((x, y, z + sz), (sx, 0, 0), (0, sy, 0), (0, 0, 1), 2, 2, 1 + m)
        sb.quad((x, y, z), (0, 0, sz), (0, sy, 0), (-1, 0, 0), 2, 2, 1 + m)
        sb.quad((x + sx, y, z), (0, 0, sz), (0, sy, 0), (1, 0, 0), 2, 2, 1 + m)
    verts, attrs = sb.finish()
    mats = np.stack([scenes.pack_material(color=(0.8, 0.75, 0.7, 1.0), roughness=0.7), scenes.pack_material(color=(0.8, 0.2, 0.2, 1.0), roughness=0.4),
                     scenes.pack_material(color=(0.8, 0.75, 0.3, 1.0), roughness=0.25, metallic=1.0), scenes.pack_material(color=(0.2, 0.4, 0.8, 1.0), roughness=0.6)])
    return scenes.Scene("light_lattice", verts, attrs, mats, lights(special=special), np.zeros(0, dtype=np.uint32),
                        scenes.Camera(eye=(4.0, 5.0, -4.5), target=(4.0, 0.2, 3.6), vfov_deg=55.0),
                        environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0), environment_intensity=0.0)


def instanced_scene(special=True):
    s = scenes.instanced_scene()
    s.lights = lights(INSTANCED_SHIFT, special=special)
    return s


def entries(n=1536, seed=23, shift=(0.0, 0.0, 0.0)):
    """(rays (n, 8), terms (n, 12), receivers (n, 8)) float32, hand-made as direct_cases.entries makes them: points on the floor,
    on the boxes' tops and sides and a few above and beside the grids, normals tilted off the surface's, every material random;
    every 11th entry is a miss"""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 3), F)
    P[:, 0], P[:, 2] = rng.uniform(0, 8, n), rng.uniform(0, 8, n)
    N = np.zeros((n, 3), F)
    N[:, 1] = 1
    for k, ((x, y, z), (sx, sy, sz)) in enumerate(BOXES):                    # a sixth of the entries on each box
        on = np.arange(n) % 6 == k
        top = on & (rng.uniform(size=n) < 0.5)
        P[on, 0], P[on, 2] = rng.uniform(x, x + sx, on.sum()), rng.uniform(z, z + sz, on.sum())
        P[top, 1] = y + sy
        side = on & ~top
        P[side, 0], P[side, 1] = x + sx, rng.uniform(y, y + sy, side.sum())
        N[side] = (1, 0, 0)
    out = np.arange(n) % 37 == 5                                                # outside every grid
    P[out, 1] = rng.uniform(2.05, 3.0, out.sum())
    edge = np.arange(n) % 41 == 7                                               # on the grids' faces
    P[edge, 0] = rng.integers(0, 9, edge.sum())
    N = (N + rng.normal(size=(n, 3)) * 0.2).astype(F)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    P += np.asarray(shift, F)[None]
    eye = np.array([4.0, 5.0, -4.5], F) + np.asarray(shift, F)
    D = ((P - eye) * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = eye, D, 1e30
    length = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
    Vd = (-D) / length[:, None]
    d = (N[:, 0] * Vd[:, 0] + N[:, 1] * Vd[:, 1]) + N[:, 2] * Vd[:, 2]
    terms = np.zeros((n, 12), F)
    metallic = rng.uniform(0, 1, n).astype(F)
    base = rng.uniform(0.05, 1, (n, 3)).astype(F)
    terms[:, 0:3] = base * (F(1) - metallic)[:, None]
    terms[:, 3] = np.sqrt(np.maximum(rng.uniform(0, 1, n) ** 2, 0.001)).astype(F)
    terms[:, 4:7] = F(0.04) + metallic[:, None] * (base - F(0.04))
    terms[:, 7] = np.maximum(d, F(1e-4))
    terms[:, 11] = 1
    miss = np.arange(n) % 11 == 4
    terms[miss] = 0
    recv = np.zeros((n, 8), F)
    recv[:, 0:3], recv[:, 4:7] = P, N
    recv[miss] = 0
    return rays, terms, recv
