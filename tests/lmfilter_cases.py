"""Inputs of the lightmap denoiser's tests (tests/test_lightmap_denoise.py without a GPU, tests/test_gpu_lightmap_denoise.py on it):
a synthetic 64 x 64 atlas of four charts whose neighbours in the atlas are no neighbours in the world, and generated lists over
smaller atlases.  Everything is a function of its arguments: the two test files see the same bytes."""
import numpy as np

F = np.float32
SAMPLES = 16
ITERATIONS = (0, 1, 3, 5, 8)
# 1 x 1; 7 x 5; 17 x 16: a second 16 x 16 tile one texel wide; 33 x 20; 130 x 67: steps larger than the image, halos outside it on
# every side (the 64 x 64 atlas below is the sixth)
SIZES = [(1, 1), (7, 5), (17, 16), (33, 20), (130, 67)]

# ---- the 64 x 64 atlas: chart ids per texel
W64 = H64 = 64
TEXEL = 0.1                       # world size of a texel
FLOOR, PATCH, DARK, WALL = 1, 2, 3, 4
LEVEL = {PATCH: 15.0, DARK: 0.05, WALL: 4.0}      # the constant charts; the floor's values are 0.3 ... 1.5
TINT = np.array([1.0, 0.9, 0.8], F)


def atlas64():
    """chart (64, 64) uint8 (0 = uncovered), positions and normals (64, 64, 3) float32, the true irradiance (64, 64) float32.
    1. FLOOR: columns 0 ... 29, y = 0, a smooth gradient along x and a hard shadow edge between rows 39 and 40.
    2. PATCH: columns 30 ... 33 of rows 0 ... 7 (the rest of those columns is a gap): coplanar with the floor, 50 units away, 10
       times as bright.
    3. DARK: columns 34 ... 63 of rows 0 ... 31: the floor of another room, 100 units away.
    4. WALL: columns 34 ... 63 of rows 32 ... 63: it continues DARK upwards across a 90 degree fold that runs between rows 31 and 32."""
    ys, xs = np.mgrid[0:H64, 0:W64]
    chart = np.zeros((H64, W64), np.uint8)
    chart[:, 0:30] = FLOOR
    chart[0:8, 30:34] = PATCH
    chart[0:32, 34:64] = DARK
    chart[32:64, 34:64] = WALL
    u, v = (xs + 0.5) * TEXEL, (ys + 0.5) * TEXEL
    P, N = np.zeros((H64, W64, 3)), np.zeros((H64, W64, 3))
    flat = chart != WALL
    P[..., 0] = u + np.where(chart == PATCH, 50.0, 0.0) + np.where((chart == DARK) | (chart == WALL), 100.0, 0.0)
    P[..., 1] = np.where(flat, 0.0, v - 32 * TEXEL)
    P[..., 2] = np.where(flat, v, 32 * TEXEL)
    N[..., 1] = np.where(flat, 1.0, 0.0)
    N[..., 2] = np.where(flat, 0.0, -1.0)
    E = (1.0 + 0.5 * xs / 30.0) * np.where(ys >= 40, 0.3, 1.0)
    for c, level in LEVEL.items():
        E = np.where(chart == c, level, E)
    E = np.where(chart == 0, 0.0, E)
    return chart, P.astype(F), N.astype(F), E.astype(F)


def receivers(texels, P, N):
    """(n, 8) float32 PTReceiver rows of the texels of (h, w, 3) position and normal images; the seed is the texel index"""
    texels = np.asarray(texels, np.uint32)
    recv = np.zeros((len(texels), 8), F)
    recv[:, 0:3], recv[:, 4:7] = P.reshape(-1, 3)[texels], N.reshape(-1, 3)[texels]
    recv[:, 3] = texels.view(F)
    return recv


def exact_rows(E, v0=0.01, samples=SAMPLES):
    """(n, 4) PTIrradiance rows without noise: rgb = E * TINT, and an m2 that gives step 1 the variance v0 (up to rounding)"""
    E = np.asarray(E, np.float64).reshape(-1)
    rgb = (E[:, None] * TINT[None, :].astype(np.float64)).astype(F)
    l = (rgb[:, 0].astype(np.float64) * 0.299 + rgb[:, 1] * 0.587) + rgb[:, 2] * 0.114
    m2 = samples * l * l + (samples - 1) * samples * v0
    return np.concatenate([rgb, m2[:, None].astype(F)], axis=1)


def noisy_rows(E, seed, samples=SAMPLES):
    """(n, 4) PTIrradiance rows of `samples` Gaussian samples per texel around E, sigma = 0.6 E + 0.05: rgb = the mean * TINT, m2 =
    the sum of the samples' squared luminance, as a gather leaves them"""
    E = np.asarray(E, np.float64).reshape(-1)
    rng = np.random.RandomState(seed)
    s = E[:, None] + rng.standard_normal((len(E), samples)) * (0.6 * E + 0.05)[:, None]
    tint = TINT.astype(np.float64)
    lum = s * (tint[0] * 0.299 + tint[1] * 0.587 + tint[2] * 0.114)
    rgb = s.mean(axis=1)[:, None] * tint[None, :]
    return np.concatenate([rgb, (lum * lum).sum(axis=1)[:, None]], axis=1).astype(F)


def atlas64_list(noise_seed=None):
    """texels ascending, receivers, irradiance rows (noise-free with a constant variance, or noisy), the true E per entry, chart per entry"""
    chart, P, N, E = atlas64()
    texels = np.nonzero(chart.reshape(-1))[0].astype(np.uint32)
    truth = E.reshape(-1)[texels]
    irr = exact_rows(truth) if noise_seed is None else noisy_rows(truth, noise_seed)
    return texels, receivers(texels, P, N), irr, truth, chart.reshape(-1)[texels]


BAD_KINDS = ["nan_rgb", "inf_m2", "inf_position", "nan_normal"]


def generated_list(width, height, seed, cover=1.0, bad=True, isolated=True):
    """A floor below a wall (the fold between rows height // 2 - 1 and height // 2) with noisy values.  cover < 1 leaves texels out
    at random; isolated: a lone covered texel inside an emptied 5 x 5 block where the atlas has room for one; bad: one entry of
    every kind of BAD_KINDS where the list has room.  Returns texels (ascending), receivers, irradiance, and a dict of the entries
    made bad and the texel made isolated (or None)."""
    rng = np.random.RandomState(seed)
    w, h = int(width), int(height)
    ys, xs = np.mgrid[0:h, 0:w]
    covered = rng.uniform(size=(h, w)) < cover
    lone = None
    if isolated and w >= 7 and h >= 7:
        cx, cy = w // 2, max(2, h // 4)
        covered[cy - 2:cy + 3, cx - 2:cx + 3] = False
        covered[cy, cx] = True
        lone = cy * w + cx
    wall = ys >= max(h // 2, 1)
    u, v = (xs + 0.5) * TEXEL, (ys + 0.5) * TEXEL
    fold = max(h // 2, 1) * TEXEL
    P, N = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    P[..., 0], P[..., 1], P[..., 2] = u, np.where(wall, v - fold, 0.0), np.where(wall, fold, v)
    N[..., 1], N[..., 2] = np.where(wall, 0.0, 1.0), np.where(wall, -1.0, 0.0)
    # normals a little off the axes, so that the normal weight is neither 0 nor 1
    N = N + rng.uniform(-0.05, 0.05, N.shape)
    N = N / np.linalg.norm(N, axis=-1, keepdims=True)
    E = np.where(wall, 2.0, 0.5) * (1.0 + 0.3 * np.sin(xs * 0.7) * np.cos(ys * 0.45))
    texels = np.nonzero(covered.reshape(-1))[0].astype(np.uint32)
    recv = receivers(texels, P.astype(F), N.astype(F))
    irr = noisy_rows(E.reshape(-1)[texels], seed + 1)
    made = {}
    if bad and len(texels) >= 12:
        picks = rng.choice(np.nonzero(texels != (lone if lone is not None else -1))[0], len(BAD_KINDS), replace=False)
        for kind, k in zip(BAD_KINDS, picks):
            made[kind] = int(k)
        irr[made["nan_rgb"], 1] = np.nan
        irr[made["inf_m2"], 3] = np.inf
        recv[made["inf_position"], 2] = -np.inf
        recv[made["nan_normal"], 4] = np.nan
    return texels, recv, irr, {"bad": made, "lone": lone}
