"""Lists and a scene for the adaptive gather's tests (test_adaptive_gather.py, test_gpu_adaptive_gather.py): accumulated entries whose
fate under step 2 is known by construction, in every survivor pattern the compaction has to get right, the special entries the rule
has a sentence for, and a box whose floor is half in the shadow of an occluder."""
import numpy as np

from unity_webgpu_pathtracer_amd import scenes
import chart_cases

F = np.float32
# 1 ... 257 straddle a wave and a 256-entry block; 262,145 needs more than 1,024 block counts, so a scan thread's run is longer than one
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 262145]
PATTERNS = ["none", "all", "alternating", "last", "first", "random30"]
# the parameters of the generated lists
N, ADD, MAX, THRESHOLD, DARK_FLOOR = 16, 8, 64, 0.05, 0.01
ACTIVE, BY_THRESHOLD, BY_MAX_SAMPLES, NON_FINITE = 0, 1, 2, 3


def pattern_mask(count, pattern, seed=0):
    """which entries of a list of `count` go on"""
    keep = np.zeros(count, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "alternating":
        keep[::2] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "random30":
        keep = np.random.RandomState(seed).uniform(size=count) < 0.3
    else:
        assert pattern == "none", pattern
    return keep


def receivers(count, seed=0):
    """(count, 8) float32 PTReceiver rows, every one different: position, seed bits, unit normal, 0"""
    rng = np.random.RandomState(seed + 77)
    recv = np.zeros((count, 8), F)
    recv[:, 0:3] = rng.uniform(-1.0, 1.0, (count, 3))
    recv[:, 3] = (np.arange(count, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed)).view(F)
    n = rng.normal(size=(count, 3))
    recv[:, 4:7] = n / np.linalg.norm(n, axis=1, keepdims=True)
    return recv


def generated_list(count, pattern, seed=0, n=N):
    """(acc (count, 4) float32 of n samples each, recv (count, 8), keep (count,) bool): an entry that goes on has a relative variance
    of the mean of about 2 / (n - 1) -- forty times THRESHOLD^2 at n = 16 --, one that stops about 1e-4 / (n - 1)"""
    rng = np.random.RandomState(seed)
    keep = pattern_mask(count, pattern, seed)
    e = (0.5 + rng.uniform(size=count)).astype(F)
    acc = np.zeros((count, 4), F)
    acc[:, 0], acc[:, 1], acc[:, 2] = e, e * F(0.5), e * F(0.25)
    l = ((acc[:, 0] * F(0.299) + acc[:, 1] * F(0.587)) + acc[:, 2] * F(0.114)).astype(np.float64)
    spread = np.where(keep, 2.0 + rng.uniform(size=count), 1e-4 * rng.uniform(size=count))
    acc[:, 3] = (n * l * l * (1.0 + spread)).astype(F)
    return acc, receivers(count, seed), keep


def fresh_rows(count, seed, m=ADD):
    """(count, 4) float32: what a gather of m samples might return"""
    rng = np.random.RandomState(seed + 1000)
    e = (0.5 + rng.uniform(size=count)).astype(F)
    out = np.zeros((count, 4), F)
    out[:, 0], out[:, 1], out[:, 2] = e, e * F(0.45), e * F(0.3)
    out[:, 3] = (m * (e.astype(np.float64) * 0.65) ** 2 * (1.0 + rng.uniform(size=count))).astype(F)
    return out


def special_entries():
    """(acc rows of N samples, what step 2 makes of each under (N, ADD, MAX, THRESHOLD, DARK_FLOOR), a word on each)"""
    nan, inf = np.nan, np.inf
    noisy = [1.0, 0.5, 0.25, N * 0.621 ** 2 * 3.0]
    rows = [([nan, 0.5, 0.25, 10.0], NON_FINITE, "NaN in rgb"),
            ([1.0, inf, 0.25, 10.0], NON_FINITE, "Inf in rgb"),
            ([1.0, 0.5, -inf, 10.0], NON_FINITE, "-Inf in rgb"),
            ([1.0, 0.5, 0.25, nan], NON_FINITE, "NaN in m2"),
            ([1.0, 0.5, 0.25, inf], NON_FINITE, "Inf in m2"),
            (noisy, ACTIVE, "a plain noisy entry"),
            ([1.0, 0.5, 0.25, N * 0.621 ** 2], BY_THRESHOLD, "no spread at all"),
            ([1.0, 0.5, 0.25, 0.0], BY_THRESHOLD, "m2 below S l l: the variance clamps to 0"),
            ([0.0, 0.0, 0.0, 0.0], BY_THRESHOLD, "l == 0 and m2 == 0: v = 0 is not above 0"),
            # l == 0 with m2 = 1: v = 1 / 240, the bound is THRESHOLD^2 DARK_FLOOR^2 = 2.5e-7
            ([0.0, 0.0, 0.0, 1.0], ACTIVE, "l == 0, m2 > 0: measured against the floor"),
            # l = 0.001, v / l^2 = 0.1 (forty times THRESHOLD^2), but v = 1e-7 is below THRESHOLD^2 DARK_FLOOR^2 = 2.5e-7
            ([0.001 / 0.621, 0.0005 / 0.621, 0.00025 / 0.621, N * 1e-6 + 1e-7 * N * (N - 1)], BY_THRESHOLD, "l below darkFloor: the floor decides")]
    return np.array([r[0] for r in rows], F), np.array([r[1] for r in rows]), [r[2] for r in rows]


def bound_entries():
    """Two entries of n = 2 samples under threshold = 1, darkFloor = 0.  With q = fl(l * l): S l l = 2 q and the bound is 1 * q, both
    exact.  m2 = 4 q gives (4 q - 2 q) / 1 = 2 q, v = q EXACTLY at the bound: the comparison is >, so it stops.  The next float32
    above 4 q gives v = q + ulp: it goes on.  -> (acc (2, 4), n, threshold, dark_floor, [BY_THRESHOLD, ACTIVE])"""
    rgb = np.array([0.7, 0.9, 0.3], F)
    l = (rgb[0] * F(0.299) + rgb[1] * F(0.587)) + rgb[2] * F(0.114)
    q = F(l * l)
    m2 = F(4.0) * q
    acc = np.array([[*rgb, m2], [*rgb, np.nextafter(m2, F(np.inf))]], F)
    return acc, 2, 1.0, 0.0, [BY_THRESHOLD, ACTIVE]


def counts_for(count, seed, samples_eq=MAX):
    """(count,) uint32 counts on the rounds' grid N + k * ADD up to MAX, every fourth entry at samples_eq"""
    rng = np.random.RandomState(seed + 5)
    c = (N + ADD * rng.randint(0, (MAX - N) // ADD + 1, count)).astype(np.uint32)
    c[::4] = samples_eq
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# a scene that is heterogeneous on purpose
# ---------------------------------------------------------------------------------------------------------------------------
SHADOW_X = -0.05            # floor receivers with x below this lie in the occluder's shadow, those above -SHADOW_X in plain view of the light


def shadowed_box():
    """chart_cases.open_box()'s shell and point light plus a white quad half way up that shadows the floor's half x < 0: the light
    sits at (0.45, 1.7, -0.35), the quad at y = 0.85 spans x -0.4 ... 0.225 and z -0.8 ... 0.45, so its shadow on the floor is twice
    as large about (0.45, -0.35): x -1.25 ... 0, z -1.25 ... 1.25.  Lit texels get the light's direct term, the same for every
    sample; shadowed ones only indirect light.  The first two triangles are the floor quad, as in open_box()."""
    sb, mats = scenes.SoupBuilder(), []
    scenes._cornell_shell(sb, mats)
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1), 1, 1, 0)
    sb.quad((-0.4, 0.85, -0.8), (0.625, 0, 0), (0, 0, 1.25), (0, -1, 0), 1, 1, 0)
    verts, attrs = sb.finish()
    light = scenes.pack_point_light(chart_cases.LIGHT_POS, (1.0, 0.8, 0.6), intensity=5.0, rng=10.0)
    return scenes.Scene("adaptive_shadowed_box", verts, attrs, np.stack(mats), np.stack([light]).astype(F), np.zeros(0, np.uint32),
                        scenes.Camera(eye=(0.0, 1.0, -0.9), target=(0.0, 1.0, 0.0)), environment_mode=1, environment_color=(0.0, 0.0, 0.0, 1.0),
                        environment_intensity=0.0)
