"""Inputs of the baked-light shading tests (tests/test_shade_baked.py, tests/test_gpu_shade_baked.py): material, ray and surface
rows for the terms, probe and box sets for the probe choice, terms and looked-up light for the compose step.  Deterministic; the
sanitizer program (csrc/shade_sanitize_main.cpp) walks the same shapes."""
import numpy as np

F = np.float32
TERM_CASES = 4096


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def term_rows(n=TERM_CASES, seed=21):
    """materials (n, 12), rays (n, 8), surfaces (n, 12): random hits inside [-1, 1]^3, then the named edge cases in the first rows"""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, 12), F)
    M[:, 0:3] = rng.random((n, 3))
    M[:, 3] = rng.random(n)
    M[:, 4:7] = rng.random((n, 3)) * (rng.random((n, 1)) < 0.2)
    M[:, 7] = np.maximum(rng.random(n) ** 2, 0.001)
    M[:, 8] = 1.0 - 0.5 * rng.random(n) * (rng.random(n) < 0.5)
    M[:, 9] = 1.0
    M.view(np.uint32)[:, 10] = rng.integers(0, 8, n)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    rays[:, 3:6] = _unit(rng.normal(size=(n, 3)))
    rays[:, 6] = 1e30
    S = np.zeros((n, 12), F)
    S[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    S[:, 3] = rng.random(n) * 3
    S[:, 4:7] = _unit(rng.normal(size=(n, 3)))                # about half face away from the viewer
    S.view(np.uint32)[:, 7] = M.view(np.uint32)[:, 10]
    S[:, 8:10] = rng.random((n, 2))
    S.view(np.uint32)[:, 10] = 0xFFFFFFFF
    S.view(np.uint32)[:, 11] = rng.integers(0, 1000, n)
    # 0: a back-facing normal; 1: the same, front-facing
    rays[0:2, 3:6] = (0, 0, -1)
    S[0, 4:7] = (0, 0, -1)
    S[1, 4:7] = (0, 0, 1)
    # 2, 3: directions of length 4 and 0.25
    rays[2, 3:6] *= 4
    rays[3, 3:6] *= 0.25
    # 4 ... 7: metallic 0 and 1, roughness 0.001 and 1
    M[4, 3], M[5, 3], M[6, 7], M[7, 7] = 0, 1, 0.001, 1
    # 8: grazing (N.V = 0 exactly -> nDotV 1e-4); 9: a miss
    rays[8, 3:6] = (1, 0, 0)
    S[8, 4:7] = (0, 0, 1)
    M[9] = 0
    M.view(np.uint32)[9, 10:12] = (0xFFFFFFFF, 1)
    return M, rays, S


def box_rows(lo, hi):
    lo = np.asarray(lo, F).reshape(-1, 3)
    rows = np.zeros((lo.shape[0], 8), F)
    rows[:, 0:3], rows[:, 4:7] = lo, np.asarray(hi, F).reshape(-1, 3)
    return rows


def probe_sets():
    """name -> (probe positions (k, 3) or None, box rows (k, 8) or None) for points inside [-1, 1]^3"""
    five = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0, 0.5, 0.5], [0, 0, -0.75], [0.5, 0.5, 0.5]], F)
    tie = np.array([[0.25, 0, 0], [-0.25, 0, 0], [0.25, 0, 0]], F)          # 0 and 2 coincide: every point is a tie between them
    return {
        "none": (None, None),
        "one": (five[:1], None),
        "five": (five, None),
        "five-boxes-none": (five, box_rows(five + 5, five + 6)),                          # no box holds a point
        "five-boxes-all": (five, box_rows(np.full((5, 3), -2), np.full((5, 3), 2))),      # every box holds every point
        "five-boxes-overlap": (five, box_rows(five - 0.75, five + 0.75)),                 # some points in none, one or several
        "tie": (tie, None),
        "tie-boxes": (tie, box_rows(np.full((3, 3), -2), np.full((3, 3), 2))),
    }


def compose_rows(res, seed=22):
    """terms (n, 12), irradiance (n, 4), reflection (n, 4): the table's corners and edges -- nDotV and rho at 1e-4, 0, 1, at the
    first and last entry centres and between -- times random colours; the last row is a miss"""
    rng = np.random.default_rng(seed)
    c = [0.0, 1e-4, 0.5 / res, 1.0 / res, 0.37, 1.0 - 1.0 / res, 1.0 - 0.5 / res, 1.0]
    nv, rho = np.meshgrid(np.array(c, F), np.array(c, F))
    nv, rho = nv.ravel(), rho.ravel()
    keep = nv > 0                                         # nDotV = 0 is the miss's
    nv, rho = nv[keep], rho[keep]
    n = nv.shape[0] + 1
    T = np.zeros((n, 12), F)
    T[:, 0:3] = rng.random((n, 3))
    T[:-1, 3] = rho
    T[:, 4:7] = rng.random((n, 3))
    T[:-1, 7] = nv
    T[:, 8:11] = rng.random((n, 3)) * (rng.random((n, 1)) < 0.3)
    T[:, 11] = rng.random(n)
    T[-1] = 0
    E = (rng.random((n, 4)) * 4).astype(F)
    R = (rng.random((n, 4)) * 4).astype(F)
    return T, E, R
