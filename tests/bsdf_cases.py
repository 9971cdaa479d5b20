"""The materials, textures and inputs of the tests that pin the material fetch and the Disney BSDF at their edges: tests/test_bsdf.py
(the oracle, on the CPU) and tests/test_gpu_bsdf.py (pt_device.h's functions inside a kernel, and whole frames, against the oracle).
Everything is deterministic (fixed seeds); importing this module needs neither the GPU nor the oracle (the draws of what 5 that sit on
a lobe boundary are built from the oracle's own lobe probabilities, when inputs(5, .) is first asked for).

MATERIALS: (name, pack_material arguments, {float index: raw value} written over the packed record).  TEXTURES: name -> (H, W, 4) bytes.
inputs(what, mi) is everything `what` of the BSDF probe (csrc/bsdf_probe.hip, oracle_bsdf_probe) is evaluated on for material mi --
for what 1 texture mi, for what 2 helper mi -- as (n, PER_IN[what]) float32, n <= 2^16."""
import functools

import numpy as np

import math_cases as mc

F32, F64, U32 = np.float32, np.float64, np.uint32
N_MAX = 1 << 16
PER_IN = {0: 9, 1: 3, 2: 8, 3: 10, 4: 14, 5: 11}
PER_OUT = {0: 51, 1: 20, 2: 9, 3: 15, 4: 4, 5: 8}
MATERIAL_FIELDS = ("baseColor.x", "baseColor.y", "baseColor.z", "opacity", "emission.x", "emission.y", "emission.z", "alphaMode",
                   "alphaCutoff", "anisotropic", "metallic", "roughness", "subsurface", "specularTint", "sheen", "sheenTint", "clearcoat",
                   "clearcoatRoughness", "specTrans", "ior", "ax", "ay", "eta", "occlusion")
NAN, INF = float("nan"), float("inf")
TWO24 = 16777216.0

# ---- textures ------------------------------------------------------------------------------------------------------------------
TEXTURE_NAMES = ("w1h1", "w1h7", "w7h1", "w2h2", "w5h3", "w16h16")
TEX = {n: i for i, n in enumerate(TEXTURE_NAMES)}


@functools.lru_cache(None)
def texture_bytes():
    """name -> (H, W, 4) uint8.  Every texture but the 1 x 1 holds 0 and 255 in every channel; the 1 x 1 is (255, 0, 128, 77)."""
    out = {}
    for i, name in enumerate(TEXTURE_NAMES):
        w, h = (int(v) for v in name[1:].split("h"))
        t = np.random.RandomState(300 + i).randint(0, 256, (h, w, 4)).astype(np.uint8)
        if w * h == 1:
            t[0, 0] = (255, 0, 128, 77)
        else:
            t.reshape(-1, 4)[0] = 0
            t.reshape(-1, 4)[-1] = 255
        t.setflags(write=False)
        out[name] = t
    return out


@functools.lru_cache(None)
def texture_data():
    """TextureData of all six, through scenes.pack_textures ((uint)(texel * 255) truncates: + 0.25 keeps every byte)"""
    from unity_webgpu_pathtracer_amd import scenes
    tex = scenes.pack_textures([(texture_bytes()[n].astype(F32) + F32(0.25)) / F32(255.0) for n in TEXTURE_NAMES])
    for i, n in enumerate(TEXTURE_NAMES):
        h, w = texture_bytes()[n].shape[:2]
        off = int(tex[4 * i + 2])
        assert np.array_equal(tex[off:off + w * h].view(np.uint8).reshape(h, w, 4), texture_bytes()[n])
    tex.setflags(write=False)
    return tex


# ---- materials -----------------------------------------------------------------------------------------------------------------
POINTWISE = [          # tests/test_oracle_analytic.py _POINTWISE_MATERIALS (tests/test_bsdf.py checks that the two lists are one)
    dict(color=(0.8, 0.6, 0.4, 1), roughness=0.7),
    dict(color=(0.8, 0.6, 0.4, 1), roughness=0.3, ior=1.6, specular_tint=0.7),
    dict(color=(0.9, 0.8, 0.7, 1), roughness=0.4, metallic=1.0),
    dict(color=(0.9, 0.8, 0.7, 1), roughness=0.5, metallic=1.0, anisotropic=0.7),
    dict(color=(0.5, 0.7, 0.9, 1), roughness=0.45, metallic=0.5, anisotropic=-0.5),
    dict(color=(0.7, 0.2, 0.2, 1), roughness=0.6, clearcoat=1.0, clearcoat_gloss=0.6),
    dict(color=(0.8, 0.5, 0.4, 1), roughness=0.8, sheen=0.9, sheen_tint=0.4, subsurface=0.6),
    dict(color=(0.9, 0.95, 1.0, 0.2), roughness=0.3, ior=1.5),
    dict(color=(0.9, 0.95, 1.0, 0.0), roughness=0.15, ior=1.33),
    dict(color=(0.6, 0.6, 0.6, 0.5), roughness=0.5, metallic=0.3, clearcoat=0.5, clearcoat_gloss=0.2, ior=1.8, sheen=0.3),
]
_IOR = dict(color=(0.8, 0.6, 0.4, 0.4), roughness=0.3)                    # 60 % glass: every lobe but the coat has weight
_ANISO = dict(color=(0.9, 0.8, 0.7, 1), roughness=0.4, metallic=1.0)
_OPAC = dict(roughness=0.35, ior=1.5, metallic=0.25)
_TEXD = dict(color=(0.9, 0.8, 0.7, 1), roughness=0.5, metallic=0.3, ior=1.4, emission=(0.1, 0.2, 0.3))
MATERIALS = [(f"pointwise{i}", kw, {}) for i, kw in enumerate(POINTWISE)] + [
    ("rough0", dict(color=(0.8, 0.6, 0.4, 0.7), roughness=0.0, metallic=0.4), {}),
    ("rough0.001", dict(color=(0.8, 0.6, 0.4, 0.7), roughness=0.001, metallic=0.4), {}),
    ("rough1", dict(color=(0.8, 0.6, 0.4, 0.7), roughness=1.0, metallic=0.4), {}),
    ("ior0.5", dict(ior=0.5, **_IOR), {}), ("ior1.0", dict(ior=1.0, **_IOR), {}), ("ior1.001", dict(ior=1.001, **_IOR), {}),
    ("ior2.0", dict(ior=2.0, **_IOR), {}), ("ior2.5", dict(ior=2.5, **_IOR), {}),
    ("aniso-1", dict(anisotropic=-1.0, **_ANISO), {}), ("aniso-0.9", dict(anisotropic=-0.9, **_ANISO), {}),
    ("aniso0.9", dict(anisotropic=0.9, **_ANISO), {}), ("aniso1", dict(anisotropic=1.0, **_ANISO), {}),
    ("opacity-0.5", dict(color=(0.7, 0.8, 0.9, -0.5), **_OPAC), {}), ("opacity0", dict(color=(0.7, 0.8, 0.9, 0.0), **_OPAC), {}),
    ("opacity1", dict(color=(0.7, 0.8, 0.9, 1.0), **_OPAC), {}), ("opacity1.5", dict(color=(0.7, 0.8, 0.9, 1.5), **_OPAC), {}),
    ("black_base", dict(color=(0.0, 0.0, 0.0, 1), roughness=0.5, specular_tint=0.6, sheen=0.5, sheen_tint=0.7), {}),      # luminance 0: ctint = 1
    ("base_above_1", dict(color=(1.5, 1.2, 0.3, 1), roughness=0.5, metallic=0.5), {}),
    ("metallic0", dict(color=(0.6, 0.7, 0.8, 1), roughness=0.4, metallic=0.0, specular_tint=0.5), {}),
    ("metallic1", dict(color=(0.6, 0.7, 0.8, 1), roughness=0.4, metallic=1.0), {}),
    ("coat_alone", dict(color=(0.0, 0.0, 0.0, 1), roughness=0.5, metallic=1.0, clearcoat=1.0, clearcoat_gloss=0.5), {}),   # black metal: at V.z = 1 only the coat
    ("coat_gloss0", dict(color=(0.7, 0.2, 0.2, 1), roughness=0.6, clearcoat=1.0, clearcoat_gloss=0.0), {}),
    ("coat_gloss1", dict(color=(0.7, 0.2, 0.2, 1), roughness=0.6, clearcoat=1.0, clearcoat_gloss=1.0), {}),
    ("sheen1_subsurface1", dict(color=(0.8, 0.5, 0.4, 1), roughness=0.8, sheen=1.0, subsurface=1.0), {}),
    ("tints1", dict(color=(0.8, 0.5, 0.2, 1), roughness=0.5, ior=1.7, specular_tint=1.0, sheen=0.5, sheen_tint=1.0), {}),
    ("alpha_blend", dict(color=(0.8, 0.8, 0.8, 0.6), roughness=0.5, alpha_mode=1), {}),
    ("alpha_mask", dict(color=(0.8, 0.8, 0.8, 0.3), roughness=0.5, alpha_mode=2, alpha_cutoff=0.5), {}),
    ("nan_roughness", dict(color=(0.8, 0.6, 0.4, 0.8), metallic=0.3), {9: NAN}),
    ("inf_sheen", dict(color=(0.8, 0.6, 0.4, 1), roughness=0.5), {16: INF}),
    ("tex_base", dict(tex_base=TEX["w5h3"], **_TEXD), {}),
    ("tex_mr", dict(tex_mr=TEX["w16h16"], **_TEXD), {}),
    ("tex_emission", dict(tex_emission=TEX["w2h2"], **_TEXD), {}),
    ("tex_occlusion", dict(tex_occlusion=TEX["w5h3"], **_TEXD), {}),
    ("tex_all_four", dict(tex_base=TEX["w1h7"], tex_mr=TEX["w7h1"], tex_emission=TEX["w1h1"], tex_occlusion=TEX["w2h2"], uv_scale=(1.5, -2.0), uv_offset=(0.25, 0.5), **_TEXD), {}),
    ("uv_to_0", dict(tex_base=TEX["w5h3"], uv_scale=(0.0, 0.0), uv_offset=(0.0, 0.0), **_TEXD), {}),
    ("uv_to_1", dict(tex_base=TEX["w5h3"], uv_scale=(0.0, 0.0), uv_offset=(1.0, 1.0), **_TEXD), {}),
    ("uv_below_0", dict(tex_base=TEX["w5h3"], uv_scale=(1.0, 1.0), uv_offset=(-1.5, -3.25), **_TEXD), {}),
    ("uv_above_2", dict(tex_base=TEX["w5h3"], uv_scale=(1.0, 1.0), uv_offset=(2.25, 5.0), **_TEXD), {}),
    ("uv_past_2^24", dict(tex_base=TEX["w5h3"], uv_scale=(1.0, 4.0 * TWO24), uv_offset=(2.0 * TWO24, 0.0), **_TEXD), {}),
]
MATERIAL_NAMES = tuple(m[0] for m in MATERIALS)
MI = {n: i for i, n in enumerate(MATERIAL_NAMES)}
TEXTURED = tuple(n for n, kw, _ in MATERIALS if any(k.startswith("tex_") for k in kw))
# materials the float64 transcription of tests/test_oracle_analytic.py is applied to: finite, in range, roughness >= 0.15, no texture
TRANSCRIBED = ("rough1", "ior2.0", "aniso-0.9", "aniso0.9", "opacity0", "opacity1", "black_base", "base_above_1", "metallic0", "metallic1",
               "coat_alone", "coat_gloss0", "coat_gloss1", "sheen1_subsurface1", "tints1", "alpha_blend", "alpha_mask")


@functools.lru_cache(None)
def materials():
    """(M, 32) float32 MaterialData"""
    from unity_webgpu_pathtracer_amd import scenes
    rows = []
    for _, kw, raw in MATERIALS:
        m = scenes.pack_material(**kw)
        for k, v in raw.items():
            m[k] = v
        rows.append(m)
    out = np.stack(rows).astype(F32)
    out.setflags(write=False)
    return out


# ---- uv ------------------------------------------------------------------------------------------------------------------------
def _neighbours(v):
    v = np.asarray(v, dtype=F32)
    with np.errstate(all="ignore"):
        return np.concatenate([v, np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))])


@functools.lru_cache(None)
def uv_values():
    """0, -0, 1 and its neighbours; k / (W - 1) for every texture extent with the float on each side; values the wrap moves"""
    exact = np.unique(np.concatenate([np.arange(w) / F64(w - 1) for w in (2, 3, 5, 7, 16)]).astype(F32))
    odd = np.array([0.0, -0.0, 1.0, -0.25, -1.0, 3.5, 1e-45, TWO24, -TWO24, INF, -INF, NAN], dtype=F32)
    v = np.concatenate([_neighbours(exact), odd])
    v.setflags(write=False)
    return v


@functools.lru_cache(None)
def uv_pairs():
    """every (u, v) of uv_values() squared"""
    v = uv_values()
    p = np.stack([np.repeat(v, v.size), np.tile(v, v.size)], -1)
    p.setflags(write=False)
    return p


# ---- directions and normals ------------------------------------------------------------------------------------------------------
Z_VALUES = (1.0, 0.5, 1e-3, 1e-7, 0.0, -0.0, -1e-7, -1e-3, -0.5, -1.0)
AZIMUTHS = (0.0, 0.5 * np.pi, 0.25 * np.pi, 3.5)          # the two axes among them


@functools.lru_cache(None)
def local_directions():
    """(n, 3) float32 about +z: every z of Z_VALUES at four azimuths (z = +-1 once), one non-unit vector, the zero vector"""
    d = []
    for z in Z_VALUES:
        s = np.sqrt(1.0 - z * z)
        for a in AZIMUTHS if abs(z) != 1.0 else AZIMUTHS[:1]:
            x, y = (s, 0.0) if a == 0.0 else (0.0, s) if a == AZIMUTHS[1] else (s * np.cos(a), s * np.sin(a))
            d.append((x, y, z))
    d += [(0.3, -0.4, 1.2), (0.0, 0.0, 0.0)]
    out = np.array(d, dtype=F32)
    out.setflags(write=False)
    return out


NORMAL_NAMES = ("+z", "-z", "near -z", "zero", "non-unit", "generic a", "generic b", "generic c")
AXIS_NORMALS = (0, 1)                                     # local z is +-world z exactly under these two


@functools.lru_cache(None)
def normals():
    g = [np.array(v, dtype=F64) / np.linalg.norm(v) for v in ((0.3, -0.5, 0.8), (-0.2, 0.9, -0.4), (0.7, 0.1, -0.7))]
    nz = np.array((1e-4, 0.0, -1.0)) / np.linalg.norm((1e-4, 0.0, -1.0))
    out = np.array([(0, 0, 1), (0, 0, -1), nz, (0, 0, 0), (0.0, 1.5, 2.0)] + g, dtype=F32)
    out.setflags(write=False)
    return out


def _frame64(n):
    """a float64 orthonormal frame about n (the zero normal: the world axes)"""
    n = n.astype(F64)
    if not n.any():
        return np.eye(3)
    z = n / np.linalg.norm(n)
    x = np.cross((0.0, 1.0, 0.0) if abs(z[1]) < 0.9 else (1.0, 0.0, 0.0), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


@functools.lru_cache(None)
def directions_about(ni):
    """local_directions() in the world: as they are under the first five normals (so 0, -0 and +-1 arrive exactly), turned into the
    normal's frame under the generic ones"""
    d = local_directions()
    if ni >= 5:
        d = (d.astype(F64) @ _frame64(normals()[ni])).astype(F32)
    return d


@functools.lru_cache(None)
def pairs():
    """every (V, normal): (n, 6) float32 and the index of the normal.  The last row is a V with a NaN under the zero normal: the dot
    product is NaN, `<= 0` fails and ffnormal = -normal = (-0, -0, -0) -- the one way normal and ffnormal differ in the sign of zero
    components only, which onb_of_normal's `==` calls equal."""
    rows, idx = [], []
    for ni in range(len(normals())):
        for v in directions_about(ni):
            rows.append(np.concatenate([v, normals()[ni]]))
            idx.append(ni)
    rows.append(np.array([NAN, 0.0, 1.0, 0.0, 0.0, 0.0]))
    idx.append(3)
    return np.array(rows, dtype=F32), np.array(idx)


UV_SHADE = np.array([(0.3, 0.6), (0.0, 1.0), (-0.25, 3.5), (0.5, 0.5)], dtype=F32)       # what 3 to 5: the uv of element i is UV_SHADE[i % 4]
FLOORS = np.array([0.0, 1.0, 0.0, 0.5, 0.0], dtype=F32)                                  # ... and its roughness floor FLOORS[i % 5]


def _shade_head(mi, vn):
    """columns 0 to 9 of what 3 to 5 over the (V, normal) rows vn"""
    n = len(vn)
    i = np.arange(n)
    return np.concatenate([np.full((n, 1), mi, F32), UV_SHADE[i % 4], vn, FLOORS[i % 5][:, None]], axis=1).astype(F32)


# ---- RNG -----------------------------------------------------------------------------------------------------------------------
def pcg_next(s):
    """one step of util/random.hlsl:5-16 over a uint32 array (the recurrence of test_oracle_analytic._pcg_chain, vectorised)"""
    s = np.asarray(s, dtype=np.uint64)
    old = (s + 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((old >> ((old >> 28) + 4)) ^ old) * 277803737) & 0xFFFFFFFF
    return (((word >> 22) ^ word) & 0xFFFFFFFF).astype(U32)


def pcg_previous(states):
    """the states pcg_next maps onto `states`"""
    from env_cases import rng_preimages
    return rng_preimages(states)


def third_draw(states):
    s = np.asarray(states, dtype=U32)
    for _ in range(3):
        s = pcg_next(s)
    return (s.astype(F32) / F32(4294967296.0)).astype(F32), s


@functools.lru_cache(None)
def plain_states():
    s = np.concatenate([np.array(mc.KNOWN_SEEDS, dtype=U32), mc.random_bits(252, 55)])
    s.setflags(write=False)
    return s


# the (V, normal) rows the boundary draws are built for: V at z = 0.5, at the normal itself (sample_ggx_vndf: lensq == 0), grazing; from
# outside (+z) and from inside (-z: eta = ior, total internal reflection at grazing V)
BOUNDARY_PAIRS = np.array([(0.6123724, 0.6123724, 0.5, 0, 0, 1), (0, 0, 1, 0, 0, 1), (0.6123724, 0.6123724, 0.5, 0, 0, -1),
                           (0.999999, 0, 1e-3, 0, 0, -1), (0.8, 0, 0.6, 0, 0, -1)], dtype=F32)


def boundary_states(lobes):
    """lobes: (k, 8) the oracle's Lobes of the k BOUNDARY_PAIRS at floor 0.  Returns (pair index, state) rows whose THIRD draw is
    cdf0, cdf2 or cdf3 of that pair, or the float on either side of it."""
    rows = []
    for p, w in enumerate(np.asarray(lobes, dtype=F32)):
        cdf0 = w[3]
        cdf1 = F32(cdf0 + w[4])
        cdf2 = F32(cdf1 + w[5])
        cdf3 = F32(cdf2 + w[6])
        for c in (cdf0, cdf2, cdf3):
            if not (np.isfinite(c) and 0.0 < c <= 1.0):
                continue
            for r in _neighbours([c]):
                target = int(F64(r) * 4294967296.0)
                if not 0 <= target <= 0xFFFFFFFF:
                    target = 0xFFFFFFFF
                s = np.array([target], dtype=U32)
                assert third_draw(pcg_previous(pcg_previous(pcg_previous(s))))[1][0] == s[0]
                rows.append((p, int(pcg_previous(pcg_previous(pcg_previous(s)))[0])))
    return rows


# ---- helpers (what 2) ------------------------------------------------------------------------------------------------------------
HELPERS = ("gtr1", "sample_gtr1", "sample_ggx_vndf", "gtr2_aniso", "smith_g", "smith_g_aniso", "schlick_weight", "dielectric_fresnel",
           "cosine_sample_hemisphere", "power_heuristic", "reflect3", "refract3", "make_onb", "luminance3")
ARITY = dict(gtr1=2, sample_gtr1=3, sample_ggx_vndf=7, gtr2_aniso=5, smith_g=2, smith_g_aniso=5, schlick_weight=1, dielectric_fresnel=2,
             cosine_sample_hemisphere=2, power_heuristic=2, reflect3=6, refract3=7, make_onb=3, luminance3=3)
RESULTS = dict(sample_gtr1=3, sample_ggx_vndf=3, cosine_sample_hemisphere=3, reflect3=3, refract3=3, make_onb=9)
DOMAIN_N = 4096


def _unit(r, n):
    d = r.normal(0, 1, (n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@functools.lru_cache(None)
def helper_domain(name):
    """(DOMAIN_N, arity) float32: finite operands the shader calls the helper with, away from its branch points (the float64
    restatement of tests/test_bsdf.py is held on these)"""
    r = np.random.RandomState(4000 + HELPERS.index(name))
    n, u = DOMAIN_N, r.uniform
    if name == "gtr1":
        c = [u(0, 0.95, n), u(0.001, 0.5, n)]          # the coat's roughness is lerp(0.1, 0.001, gloss); at NDotH -> 1 and a -> 0 the denominator cancels
    elif name == "sample_gtr1":
        c = [u(0.002, 0.5, n), u(0, 1, n), u(0.05, 0.95, n)]
    elif name == "sample_ggx_vndf":
        v = _unit(r, n); v[:, 2] = np.abs(v[:, 2])
        c = [v[:, 0], v[:, 1], v[:, 2], u(0.05, 1, n), u(0.05, 1, n), u(0.01, 0.99, n), u(0, 1, n)]
    elif name == "gtr2_aniso":
        h = _unit(r, n)
        c = [np.abs(h[:, 2]), h[:, 0], h[:, 1], u(0.01, 1, n), u(0.01, 1, n)]
    elif name == "smith_g":
        c = [u(0.01, 1, n), u(0.01, 1, n)]
    elif name == "smith_g_aniso":
        v = _unit(r, n)
        c = [np.abs(v[:, 2]) + 0.01, v[:, 0], v[:, 1], u(0.01, 1, n), u(0.01, 1, n)]
    elif name == "schlick_weight":
        c = [u(0.0, 0.95, n)]
    elif name == "dielectric_fresnel":
        eta = np.where(r.rand(n) < 0.5, u(1.2, 2.0, n), 1.0 / u(1.2, 2.0, n))      # towards eta = 1 F is a difference of nearly equal terms
        cos = u(0.05, 1, n)
        keep = np.abs(eta * eta * (1 - cos * cos) - 1.0) > 0.05          # away from the critical angle
        c = [np.where(keep, cos, 1.0), eta]
    elif name == "cosine_sample_hemisphere":
        c = [u(0, 0.9, n), u(0, 1, n)]
    elif name == "power_heuristic":
        c = [np.exp2(u(-10, 10, n)), np.exp2(u(-10, 10, n))]
    elif name == "reflect3":
        a, b = _unit(r, n), _unit(r, n)
        c = [a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]]
    elif name == "refract3":
        a, b = _unit(r, n), _unit(r, n)
        eta = np.where(r.rand(n) < 0.5, u(1.001, 2.0, n), 1.0 / u(1.001, 2.0, n))
        d = (a * b).sum(1)
        keep = (1.0 - eta * eta * (1.0 - d * d)) > 0.05
        c = [a[:, 0], a[:, 1], a[:, 2], np.where(keep, b[:, 0], a[:, 0]), np.where(keep, b[:, 1], a[:, 1]), np.where(keep, b[:, 2], a[:, 2]), eta]
    elif name == "make_onb":
        a = _unit(r, n)
        a[:, 2] = np.where(a[:, 2] < -0.9, -a[:, 2], a[:, 2])            # away from z = -1, where 1 + z cancels and k is clamped
        a = a * u(0.5, 2.0, (n, 1))
        c = [a[:, 0], a[:, 1], a[:, 2]]
    else:
        c = [u(0, 2, n), u(0, 2, n), u(0, 2, n)]
    out = np.stack(c, -1).astype(F32)
    out.setflags(write=False)
    return out


def _helper_edges(name):
    """operand rows on the boundaries the helper branches on"""
    one = mc.floats(mc.neighbourhood(1.0, 2))
    e = []
    if name == "gtr1":                                   # a >= 1
        e = [(h, a) for h in (0.0, 0.5, 1.0) for a in one] + [(0.5, 0.0), (1.0, 1e-30)]
    elif name == "sample_gtr1":                          # max(0.001, rgh); a2 == 1
        e = [(g, r1, r2) for g in (0.0, 0.001, 0.1, 1.0, 2.0) for r1 in (0.0, 0.5, 1.0) for r2 in (0.0, 0.5, 1.0)]
    elif name == "sample_ggx_vndf":                      # lensq == 0 (V along the normal, or ax V.x underflows)
        e = [(x, y, z, ax, ay, r1, r2) for (x, y, z) in ((0, 0, 1), (0, 0, -1), (-0.0, 0.0, 1), (1e-30, 0, 1), (1e-23, 1e-23, 1), (1, 0, 0), (0, 0, 0))
             for ax, ay in ((0.001, 0.001), (0.5, 0.2), (1.0, 1.0)) for r1 in (0.0, 0.3, 1.0) for r2 in (0.0, 0.25, 0.6, 1.0)]
    elif name == "dielectric_fresnel":                   # sinThetaTSq > 1
        for eta in (2.0, 1.5, 1.001, 0.5, 1.0):
            crit = np.sqrt(max(1.0 - 1.0 / (eta * eta), 0.0))
            e += [(c, eta) for c in mc.floats(mc.neighbourhood(crit, 3)) if c >= 0] + [(0.0, eta), (1.0, eta), (-0.0, eta)]
    elif name == "refract3":                             # k < 0
        for eta in (2.0, 1.5, 0.5, 1.0):
            crit = np.sqrt(max(1.0 - 1.0 / (eta * eta), 0.0))
            for c in list(mc.floats(mc.neighbourhood(crit, 3))) + [0.0, 1.0]:
                s = np.sqrt(max(1.0 - float(c) ** 2, 0.0))
                e.append((s, 0.0, -abs(float(c)), 0, 0, 1, eta))
    elif name == "make_onb":                             # lenSq == 0; the clamp of k at z = -1
        e = [(0, 0, 0), (-0.0, -0.0, -0.0), (1e-30, 0, 0), (1e-23, 0, 1e-23), (0, 0, 1), (0, 0, -1), (0, 0, -2.5), (1e-4, 0, -1), (0, 1e-3, -1),
             (3e-3, 4e-3, -1), (1, 0, 0), (0, 1, 0), (0, -1, 0), (3e38, 3e38, 0)]
    elif name == "schlick_weight":
        e = [(v,) for v in (0.0, 1.0, -0.0, 2.0, -1.0)] + [(v,) for v in one]
    elif name in ("smith_g", "smith_g_aniso", "gtr2_aniso"):
        e = [tuple([0.0] * ARITY[name]), tuple([1.0] * ARITY[name])]
    return np.array(e, dtype=F32).reshape(-1, ARITY[name])


@functools.lru_cache(None)
def helper_operands(name):
    """(n, 7) float32: the grid of math_cases' special values (arity 1 and 2), rows drawn from the special values and from the domain,
    the branch boundaries, then the domain set itself (the last DOMAIN_N rows)"""
    k = ARITY[name]
    sp = mc.floats(mc.specials())
    r = np.random.RandomState(4100 + HELPERS.index(name))
    parts = [_helper_edges(name)]
    if k == 1:
        parts.append(sp[:, None])
    elif k == 2:
        parts.append(np.stack([np.repeat(sp, sp.size), np.tile(sp, sp.size)], -1))
    dom = helper_domain(name)
    mixed = dom[r.randint(0, len(dom), 4096)].copy()                     # a domain row with one to all operands replaced by special values
    repl = r.rand(4096, k) < 0.35
    repl[np.arange(4096), r.randint(0, k, 4096)] = True
    mixed[repl] = sp[r.randint(0, sp.size, int(repl.sum()))]
    parts += [mixed, dom]
    rows = np.concatenate(parts).astype(F32)
    out = np.zeros((len(rows), 7), dtype=F32)
    out[:, :k] = rows
    out.setflags(write=False)
    return out


# ---- the input sets --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _oracle_buffers():
    """a one-quad scene with MATERIALS and the six textures, for oracle.bsdf_probe (the geometry is never looked at)"""
    from oracle import pyoracle
    from unity_webgpu_pathtracer_amd import plugin, scenes
    sb = scenes.SoupBuilder()
    sb.quad((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0), 1, 1, 0)
    verts, attrs = sb.finish()
    s = scenes.Scene("bsdf_cases", verts, attrs, np.array(materials()), np.zeros((0, 16), dtype=F32), np.array(texture_data()),
                     scenes.Camera(eye=(0, 1, -3), target=(0, 0, 0), vfov_deg=40.0))
    nodes, tris = plugin.build_cwbvh(s.vertices)
    return pyoracle.SceneBuffers(s, nodes, tris)


def oracle_run(what, values):
    from oracle import pyoracle
    return pyoracle.bsdf_probe(_oracle_buffers(), what, values)


def block_name(what, mi):
    return {1: TEXTURE_NAMES, 2: HELPERS}.get(what, MATERIAL_NAMES)[mi]


@functools.lru_cache(None)
def inputs(what, mi):
    vn, _ = pairs()
    if what == 0:                # every uv pair; ray direction and normal take turns through every (direction, normal)
        uv = uv_pairs() if MATERIAL_NAMES[mi] in TEXTURED else uv_pairs()[:: 23]
        with np.errstate(all="ignore"):                                   # the oracle's wrap is the shader's literal +-1 loops: |u| iterations
            t = np.abs(uv * materials()[mi, 28:30] + materials()[mi, 30:32])
        uv = uv[~((t > 4096.0) & (t < TWO24)).any(axis=1)]
        i = np.arange(max(len(uv), len(vn)))
        out = np.concatenate([np.full((len(i), 1), mi, F32), uv[i % len(uv)], -vn[i % len(vn), :3], vn[i % len(vn), 3:]], axis=1)
    elif what == 1:
        out = np.concatenate([np.full((len(uv_pairs()), 1), mi, F32), uv_pairs()], axis=1)
    elif what == 2:
        ops = helper_operands(HELPERS[mi])
        out = np.concatenate([np.full((len(ops), 1), mi, F32), ops], axis=1)
    elif what == 3:
        out = _shade_head(mi, np.tile(vn, (5, 1)))                        # five times over: every pair meets every floor
    elif what == 4:              # every (V, normal) x every L about that normal x both flags
        rows = []
        for ni in range(len(normals())):
            d = directions_about(ni)
            v = np.repeat(d, len(d), axis=0)
            l = np.tile(d, (len(d), 1))
            rows.append(np.concatenate([v, np.broadcast_to(normals()[ni], v.shape), l], axis=1))
        d = directions_about(3)
        rows.append(np.concatenate([np.broadcast_to(vn[-1], (len(d), 6)), d], axis=1))       # the NaN V under the zero normal
        rows = np.concatenate(rows)
        rows = np.concatenate([np.repeat(rows, 2, axis=0), np.tile(np.array([[0.0], [1.0]], F32), (len(rows), 1))], axis=1)
        out = np.concatenate([_shade_head(mi, rows[:, :6]), rows[:, 6:]], axis=1)
    elif what == 5:              # every pair x 96 plain states; 16 spread pairs x all 256; the boundary draws
        st = plain_states()
        grid_vn, grid_st = np.repeat(vn, 96, axis=0), np.tile(st[:96], len(vn))
        wide = vn[:: max(1, len(vn) // 16)][:16]
        wide_vn, wide_st = np.repeat(wide, 256, axis=0), np.tile(st, len(wide))
        head = np.concatenate([np.full((len(BOUNDARY_PAIRS), 1), mi, F32), np.tile(UV_SHADE[0], (len(BOUNDARY_PAIRS), 1)), BOUNDARY_PAIRS,
                               np.zeros((len(BOUNDARY_PAIRS), 1), F32)], axis=1).astype(F32)
        b = boundary_states(oracle_run(3, head)[:, 7:])
        bound = head[[p for p, _ in b]] if b else np.zeros((0, 10), F32)
        bound_st = np.array([s for _, s in b], dtype=U32)
        out = np.concatenate([np.concatenate([_shade_head(mi, np.concatenate([grid_vn, wide_vn])), bound]),
                              np.concatenate([grid_st, wide_st, bound_st]).astype(U32).view(F32)[:, None]], axis=1)
    else:
        raise ValueError(what)
    out = np.ascontiguousarray(out, dtype=F32)
    assert out.shape[1] == PER_IN[what] and 0 < len(out) <= N_MAX, (what, mi, out.shape)
    out.setflags(write=False)
    return out


def boundary_rows(mi):
    """the slice of inputs(5, mi) that holds the boundary draws"""
    n = len(pairs()[0]) * 96 + 16 * 256
    return slice(n, len(inputs(5, mi)))


@functools.lru_cache(None)
def oracle_probe(what, mi):
    """oracle_bsdf_probe over inputs(what, mi): computed once, shared, read-only"""
    out = oracle_run(what, inputs(what, mi))
    out.setflags(write=False)
    return out
