"""The SH-probe rule (include/ptmi_plugin.h Part 15) restated in numpy float32, for tests/test_probe.py and tests/test_gpu_probe.py:
the basis, a lane's partial sums, the fold tree, the scaling, the delta-light add and the evaluation.  Written from the header's
text, not from sh_rule.h; every operation is one float32 operation in the rule's order.  The seed rule and the closed form of a
point or spot light are gather_ref's (Part 13's)."""
import numpy as np

from gather_ref import F, direct_irradiance, luminance, sample_seed  # noqa: F401  (re-exported for the tests)

LANES = 64
FOUR_PI = F(12.566371)
BAND_A = [F(3.14159265)] + [F(2.09439510)] * 3 + [F(0.78539816)] * 5
C0, C1, C2, C3, C4 = F(0.28209479), F(0.48860251), F(1.09254843), F(0.31539157), F(0.54627422)


def basis(w):
    """Y_0 ... Y_8 of (..., 3) float32 directions -> (..., 9) float32, as the header's expression trees"""
    w = np.asarray(w, F)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    Y = np.empty(w.shape[:-1] + (9,), F)
    Y[..., 0] = C0
    Y[..., 1] = C1 * y
    Y[..., 2] = C1 * z
    Y[..., 3] = C1 * x
    Y[..., 4] = C2 * (x * y)
    Y[..., 5] = C2 * (y * z)
    Y[..., 6] = C3 * (F(3.0) * (z * z) - F(1.0))
    Y[..., 7] = C2 * (x * z)
    Y[..., 8] = C4 * (x * x - y * y)
    return Y


def project(directions, colours):
    """directions, colours: (n, samples, 3) float32 -> sh (n, 9, 3), m2 (n,): lane l sums its samples j = l, l + 64, ... in
    ascending j from +0.0f, the 64 partials are folded by the tree, the coefficients are scaled"""
    d, c = np.asarray(directions, F), np.asarray(colours, F)
    n, samples = d.shape[0], d.shape[1]
    Y = basis(d)                                                 # (n, samples, 9)
    term = (c[:, :, None, :] * Y[:, :, :, None]).astype(F)       # L_j[c] * Y_k: (n, samples, 9, 3)
    lum = luminance(c)
    sq = (lum * lum).astype(F)
    acc = np.zeros((n, LANES, 9, 3), F)
    m2 = np.zeros((n, LANES), F)
    for first in range(0, samples, LANES):                       # ascending j within every lane
        k = min(LANES, samples - first)
        acc[:, :k] = acc[:, :k] + term[:, first:first + k]
        m2[:, :k] = m2[:, :k] + sq[:, first:first + k]
    h = LANES // 2
    while h >= 1:
        acc[:, :h] = acc[:, :h] + acc[:, h:2 * h]
        m2[:, :h] = m2[:, :h] + m2[:, h:2 * h]
        h //= 2
    sh = ((acc[:, 0] * FOUR_PI) / F(samples)).astype(F)
    return sh, m2[:, 0].copy()


def add_delta(sh, Li, direction):
    """one visible point or spot light into one probe's (9, 3) coefficients: sh[k][c] + Li[c] * Y_k(direction)"""
    Y = basis(np.asarray(direction, F))
    return (np.asarray(sh, F) + np.asarray(Li, F)[None, :] * Y[:, None]).astype(F)


def irradiance(sh, normal):
    """E(N) of one probe's (9, 3) coefficients: ascending k from +0.0f, (A_k * sh[k][c]) * Y_k(N)"""
    sh = np.asarray(sh, F)
    Y = basis(np.asarray(normal, F))
    e = np.zeros(3, F)
    for k in range(9):
        e = e + (BAND_A[k] * sh[k]) * Y[k]
    return e.astype(F)
