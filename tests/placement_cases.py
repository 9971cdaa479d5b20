"""The scene of the probe-placement tests in closed form, for tests/test_probe_placement.py and tests/test_gpu_probe_placement.py:
the closed Cornell box of tests/test_gpu_probe_volume.py (x, z in [-1, 1], y in [0, 2], normals into the room, the 1.2 x 1.2
ceiling patch at y = 1.98) with a closed cube of side 0.4 centred at (0, 0.5, 0) whose normals point out of it.  trace() is the
closest-hit query of that scene by plane distances in float64, in the rows PTTraceRays returns; place() runs the host twin over
it as PTProbePlace runs the kernels over the GPU's trace.  No GPU involved."""
import numpy as np

from unity_webgpu_pathtracer_amd import plugin

F = np.float32
U = np.uint32
CUBE_LO, CUBE_HI = np.array([-0.2, 0.3, -0.2]), np.array([0.2, 0.7, 0.2])

# (axis, plane value, normal sign on that axis, lower corner, upper corner): axis-aligned rectangles
_RECTS = [(1, 0.0, 1.0, (-1, 0, -1), (1, 0, 1)), (1, 2.0, -1.0, (-1, 2, -1), (1, 2, 1)), (1, 1.98, -1.0, (-0.6, 1.98, -0.6), (0.6, 1.98, 0.6)),
          (0, -1.0, 1.0, (-1, 0, -1), (-1, 2, 1)), (0, 1.0, -1.0, (1, 0, -1), (1, 2, 1)),
          (2, -1.0, 1.0, (-1, 0, -1), (1, 2, -1)), (2, 1.0, -1.0, (-1, 0, 1), (1, 2, 1))]
for _a in range(3):
    for _v, _s in ((CUBE_LO[_a], -1.0), (CUBE_HI[_a], 1.0)):
        _lo, _hi = CUBE_LO.copy(), CUBE_HI.copy()
        _lo[_a] = _hi[_a] = _v
        _RECTS.append((_a, float(_v), _s, tuple(_lo), tuple(_hi)))

# the probes of the composition case: inside the cube, 0.03 above the floor, free at the room's centre, 0.04 from two walls, outside
# the shell
PROBES = np.array([(0.12, 0.5, 0.0), (0.5, 0.03, 0.5), (0.0, 1.0, 0.0), (0.96, 1.0, 0.96), (1.3, 1.0, 0.0)], F)
SEEDS = (np.arange(5, dtype=np.uint32) * 7919 + 0x1234).astype(np.uint32)


def in_cube(p):
    p = np.asarray(p, np.float64)
    return bool(((p > CUBE_LO) & (p < CUBE_HI)).all())


def trace(origins, directions, tmax):
    """(n, 3) origins and directions -> (hits (n, 4), surfaces (n, 12)) float32 rows: t (tmax on a miss), prim bits (the rectangle's
    index; 0xFFFFFFFF on a miss), and on a hit the surface record's t and normal"""
    O, W = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    n = O.shape[0]
    best, prim = np.full(n, float(F(tmax))), np.full(n, 0xFFFFFFFF, np.int64)
    normal = np.zeros((n, 3))
    for k, (a, v, s, lo, hi) in enumerate(_RECTS):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (v - O[:, a]) / W[:, a]
        p = O + t[:, None] * W
        ok = np.isfinite(t) & (t > 1e-4) & (t < best)
        for b in range(3):
            if b != a:
                ok &= (p[:, b] >= lo[b]) & (p[:, b] <= hi[b])
        best[ok], prim[ok] = t[ok], k
        normal[ok] = 0.0
        normal[ok, a] = s
    hits, surf = np.zeros((n, 4), F), np.zeros((n, 12), F)
    hits[:, 0] = best
    hits[:, 3] = prim.astype(U).view(F)
    hit = prim != 0xFFFFFFFF
    surf[hit, 3], surf[hit, 4:7] = hits[hit, 0], normal[hit]
    return hits, surf


def place(positions, seeds, samples, params, first_sample=0, tracer=trace):
    """PTProbePlace by its definition: params.iterations relocation steps and one that classifies, each the host twin
    (plugin.probe_place_step) over tracer(origins, directions, maxDistance) of the rays {P + o, w_j}.  Returns (offsets, states, stats)."""
    pos = np.asarray(positions, F)
    n = pos.shape[0]
    w = plugin.probe_directions(pos, samples, first_sample=first_sample, seeds=seeds)[:, 3:6]
    o = np.zeros((n, 3), F)
    for step in range(params.iterations + 1):
        origins = np.repeat((pos + o).astype(F), samples, axis=0)
        hits, surf = tracer(origins, w, params.maxDistance)
        o, states, stats = plugin.probe_place_step(pos, hits, surf, params, move=step < params.iterations, offsets=o, first_sample=first_sample, seeds=seeds)
    return o, states, stats
