"""Hand-made inputs for the direct-light rule (include/ptmi_plugin.h Part 24): terms, receivers and rays of a floor seen from
above with the special entries the rule names, and the light sets.  tests/test_direct.py and tests/test_gpu_direct.py import it
the way the shading tests import shade_cases.py.  F64_MEASURED is the largest relative deviation of the host twins from a
float64 evaluation of the same formula over these cases, as test_direct.py measures (and prints) it."""
import numpy as np

F = np.float32
SPOT, DIRECTIONAL, POINT, RECTANGLE = 0, 1, 2, 3

# measured by test_direct.py::test_twins_against_float64 over every case below; the cap is four times it.
# The median pair deviates by 2e-7; the largest figure is the spot light on an entry at the render's smallest alpha (0.001, rho
# 0.0316) near its highlight, where t = (nh * nh) * (a2 - 1) + 1 cancels to a few float32 ulps of 1.
F64_MEASURED = 2.53e-4
F64_CAP = 4 * F64_MEASURED

MISS, BACK, FAR, NAN_P, GLOSSY = 3, 4, 5, 6, 7          # the special entries' indices


def light(kind, position, emission=(10.0, 8.0, 6.0), rng=20.0, u=(0, 0, 0), v=(0, 0, 0), area=0.0):
    r = np.zeros(16, F)
    r[0:3], r[4:7], r[7] = position, emission, rng
    r[8:11], r[11], r[12:15] = u, area, v
    r[3:4].view(np.uint32)[0] = kind
    return r


def light_sets():
    """name -> (k, 16) float32 PTLight records.  The spot points down with cos(outer) = 0.7 and cos(inner) = 0.9: the floor has
    entries outside, between and inside the two cones.  The rectangle faces down (cross(u, v) = (0, -1, 0)); `rect_back` lies
    under the floor and shows the entries its back."""
    point = light(POINT, (0.3, 2.5, -0.2))
    spot = light(SPOT, (-0.4, 3.0, 0.5), (20.0, 18.0, 12.0), u=(0.1, -1.0, 0.05), v=(0.7, 0.9, 0.0))
    rect = light(RECTANGLE, (-0.5, 2.0, -0.75), (6.0, 7.0, 9.0), u=(1.0, 0, 0), v=(0, 0, 1.5), area=1.5)
    sun = light(DIRECTIONAL, (0, 10, 0), u=(0, -1, 0))
    return {
        "none": np.zeros((0, 16), F),
        "point": point[None],
        "spot": spot[None],
        "rect": rect[None],
        "directional": sun[None],
        "all": np.stack([rect, sun, point, spot]),
        "rect_back": light(RECTANGLE, (-0.5, -2.0, -0.75), u=(1.0, 0, 0), v=(0, 0, 1.5), area=1.5)[None],
        "short_range": light(POINT, (0.3, 2.5, -0.2), rng=2.6)[None],
        "dark": np.stack([light(POINT, (0.3, 2.5, -0.2), emission=(0, 0, 0)), rect]),
        "two_rects": np.stack([light(RECTANGLE, (1.0, 1.5, 1.0), u=(0.5, 0, 0), v=(0, 0, 0.5), area=0.25), rect]),
    }


def entries(n=160, seed=11):
    """(rays (n, 8), terms (n, 12), receivers (n, 8)) float32: a floor at y = 0 within [-3, 3]^2 seen from an eye above it, every
    material random; entry MISS is a miss, BACK faces away from every light, FAR lies 40 units off, NAN_P has a NaN position,
    GLOSSY has rho = 0.03"""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 3), F)
    P[:, 0], P[:, 2] = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    N = np.zeros((n, 3), F)
    N[:, 1] = 1
    tilt = rng.normal(size=(n, 3)) * 0.2
    N = (N + tilt).astype(F)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    P[FAR] = (40.0, 0.0, 0.0)
    N[BACK] = (0.0, -1.0, 0.0)
    eye = np.array([0.5, 4.0, -3.0], F)
    D = ((P - eye) * rng.uniform(0.5, 2.0, (n, 1))).astype(F)                 # not of unit length
    D[BACK] = -D[BACK]                                                          # seen from below: N . Vd > 0 there too
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
    terms[GLOSSY, 3] = 0.03
    terms[MISS] = 0
    recv = np.zeros((n, 8), F)
    recv[:, 0:3], recv[:, 4:7] = P, N
    recv[MISS] = 0
    recv[NAN_P, 0] = np.nan
    return rays, terms, recv
