"""Inputs of the lightmap lookup tests (tests/test_lightmap_shade.py, tests/test_gpu_lightmap_shade.py): synthetic images, a small
table of attribute records, hit lists with the named edge cases in their first rows, and binding tables.  Deterministic; the
sanitizer program (csrc/lightmap_shade_sanitize_main.cpp) walks the same shapes."""
import numpy as np

from unity_webgpu_pathtracer_amd import abi

F = np.float32
NONE = 0xFFFFFFFF
PRIMS = 80                  # 64 ordinary primitives, then 16 whose first corner carries a special UV
MATERIALS = 5
SIZES = [(1, 1), (2, 2), (8, 8), (24, 8)]             # width, height
KINDS = ["full", "checker", "single", "empty", "w-values"]
# first-corner coordinates that, at size 8, put x exactly on -1, on the width, on a texel centre (3), on a texel edge (3.5), then a
# NaN, the first and last half texel, and just outside
SPECIAL = [-0.0625, 1.0625, 0.4375, 0.5, np.nan, 0.0, 1.0, -0.07]
W_VALUES = [1.0, 0.5, 0.0, -1.0, np.nan]


def image(kind, width, height, seed=0, poison=False, constant=None, ramp=None):
    """(height, width, 4) float32.  kind: "full", "checker" (every other texel cleared), "single" (one filled texel), "empty", "w-values"
    (w runs through 1.0, 0.5, 0.0, -1.0, NaN).  poison: the rgb of every texel that is not valid is NaN.  constant: one rgb for every
    texel; ramp: (a, bx, by) per channel, texel (x, y) = a + bx * x + by * y."""
    rng = np.random.default_rng(1000 + seed)
    img = np.zeros((height, width, 4), F)
    img[..., 0:3] = rng.random((height, width, 3)) * 4
    if constant is not None:
        img[..., 0:3] = np.asarray(constant, F)
    if ramp is not None:
        ys, xs = np.mgrid[0:height, 0:width]
        for c in range(3):
            img[..., c] = (ramp[c][0] + ramp[c][1] * xs + ramp[c][2] * ys).astype(F)
    ys, xs = np.mgrid[0:height, 0:width]
    if kind == "full":
        img[..., 3] = 1.0
    elif kind == "checker":
        img[..., 3] = np.where((xs + ys) % 2 == 0, 1.0, 0.0)
    elif kind == "single":
        img[height // 2, width // 2, 3] = 1.0
    elif kind == "empty":
        pass
    elif kind == "w-values":
        img[..., 3] = np.asarray(W_VALUES, F)[(xs + 2 * ys) % len(W_VALUES)]
    else:
        raise ValueError(kind)
    if poison:
        with np.errstate(invalid="ignore"):
            img[~(img[..., 3] > 0), 0:3] = np.nan
    return img


def tri_attrs(seed=7):
    """PRIMS attribute records: random UVs inside the unit square; primitives 64 ... 71 have SPECIAL[k] as their first corner's u
    (v on a texel centre), 72 ... 79 as its v"""
    rng = np.random.default_rng(seed)
    a = np.zeros(PRIMS, abi.TRI_ATTR)
    for name in ("uv0", "uv1", "uv2"):
        a[name] = rng.uniform(0.02, 0.98, (PRIMS, 2))
    for k, s in enumerate(SPECIAL):
        a["uv0"][64 + k] = (s, 0.4375)
        a["uv0"][72 + k] = (0.4375, s)
    return a


def uvs_of(attrs, first, count):
    """the (count, 6) array PTRasterizeChart takes, from the records"""
    a = attrs[first:first + count]
    return np.concatenate([a["uv0"], a["uv1"], a["uv2"]], axis=1).astype(F)


def entries(n=1024, seed=3, prims=PRIMS, materials=MATERIALS):
    """rays (n, 8), hits (n, 4), surfaces (n, 12).  Rows 0 ... 15 hit the special primitives at their first corner (both
    barycentrics 0), seen from the front; rows 16 ... 19 hit primitives 9, 10, 19 and 20 (around the span [10, 20)); from row 20 on:
    random hits, about half seen from behind, instances 0 ... 2 or none, a miss every seventh row (its surface record is never
    written: NaN words), a materialIndex just out of range and one of 0xFFFFFFFF every fiftieth."""
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    rays[:, 6] = 1e30
    hits = np.zeros((n, 4), F)
    hits[:, 0] = rng.random(n) * 3
    b = rng.random((n, 2))
    flip = b.sum(axis=1) > 1
    b[flip] = 1 - b[flip]
    hits[:, 1:3] = b
    hits.view(np.uint32)[:, 3] = rng.integers(0, min(prims, 64), n)
    S = np.zeros((n, 12), F)
    S[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    S[:, 3] = hits[:, 0]
    nrm = rng.normal(size=(n, 3))
    S[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    S.view(np.uint32)[:, 7] = rng.integers(0, materials, n)
    S[:, 8:10] = rng.random((n, 2))
    S.view(np.uint32)[:, 10] = np.array([0, 1, 2, NONE], np.uint32)[rng.integers(0, 4, n)]
    S.view(np.uint32)[:, 11] = hits.view(np.uint32)[:, 3]
    i = np.arange(n)
    if prims >= PRIMS:
        hits.view(np.uint32)[0:16, 3] = np.arange(64, 80)
        hits[0:16, 1:3] = 0
    hits.view(np.uint32)[16:20, 3] = (9, 10, 19, 20)
    S[0:20, 4:7] = -rays[0:20, 3:6] / np.linalg.norm(rays[0:20, 3:6], axis=1, keepdims=True)       # seen from the front
    S.view(np.uint32)[0:20, 7] = 0
    S.view(np.uint32)[0:20, 10] = NONE
    S.view(np.uint32)[(i >= 20) & (i % 50 == 25), 7] = materials
    S.view(np.uint32)[(i >= 20) & (i % 50 == 26), 7] = NONE
    miss = (i >= 20) & (i % 7 == 3)
    hits.view(np.uint32)[miss, 3] = NONE
    hits[miss, 1:3] = 0
    hits[miss, 0] = 1e30
    S.view(np.uint32)[miss] = NONE
    return rays, hits, S


def binding(img, first=0, count=PRIMS, instance=None, uvs=None, two_sided=False):
    return {"image": img, "first_prim": first, "prim_count": count, "instance": instance, "uvs": uvs, "two_sided": two_sided}


def tables(attrs, prims=PRIMS, poison=False):
    """name -> binding list over `prims` primitives whose records are attrs"""
    t = {"none": []}
    for k, (w, h) in enumerate(SIZES):
        for j, kind in enumerate(KINDS):
            img = image(kind, w, h, seed=10 * k + j, poison=poison)
            # UVs from the records and, every other table, from an array of their values; two-sided every third
            uvs = uvs_of(attrs, 0, prims) if (k + j) % 2 else None
            t[f"{w}x{h}-{kind}"] = [binding(img, 0, prims, uvs=uvs, two_sided=(k + j) % 3 == 0)]
    full = [image("full", w, h, seed=50 + k, poison=poison) for k, (w, h) in enumerate(SIZES)]
    t["three"] = [binding(full[2], 0, 10), binding(full[3], 10, 10, two_sided=True), binding(full[1], 20, prims - 20, uvs=uvs_of(attrs, 20, prims - 20))]
    t["span-10-20"] = [binding(full[2], 10, 10, two_sided=True)]
    t["overlap"] = [binding(full[2], 0, 40, two_sided=True), binding(full[3], 20, 40, two_sided=True)]                  # 20 ... 39: the lower index wins
    t["instances"] = [binding(full[2], 0, prims, instance=1, two_sided=True), binding(full[3], 0, prims, instance=2, two_sided=True)]
    t["instance-then-any"] = [binding(full[2], 0, prims, instance=0), binding(full[1], 0, prims, two_sided=True)]
    t["one-sided-then-two"] = [binding(full[2], 0, prims), binding(full[3], 0, prims, two_sided=True)]                  # a back face falls through to 1
    t["one-sided"] = [binding(full[2], 0, prims)]
    # 64 bindings: one primitive each, sizes and kinds in turn
    t["sixty-four"] = [binding(image(KINDS[k % 3], *SIZES[k % 4], seed=100 + k, poison=poison), k, 1, two_sided=k % 2 == 0) for k in range(64)]
    return t
