"""The material fetch and the Disney BSDF at their edges, on the CPU: the oracle (oracle_bsdf_probe) over the materials, textures and inputs
of tests/bsdf_cases.py, held to exact equivalences between materials that clamp onto each other, to known answers of the texture lookup,
to the float64 transcription of tests/test_oracle_analytic.py, to a float64 restatement of every sampling helper, and to a recorded lobe
histogram.  What holds here is what tests/test_gpu_bsdf.py then holds the kernels to, bit for bit."""
import json
import os

import numpy as np
import pytest

import bsdf_cases as bc
import math_cases as mc

F32, F64, U32 = np.float32, np.float64, np.uint32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bsdf_sample_record.json")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def _same(name, got, want):
    """bit for bit, a NaN matched by any NaN"""
    g, w = _bits(got).ravel(), _bits(want).ravel()
    x = np.arange(g.size, dtype=U32)
    mc.assert_same_bits(name, x, np.zeros_like(x), g, w, "first", "second")


def test_the_pointwise_materials_are_the_analytic_tests_list():
    import test_oracle_analytic as toa
    assert bc.POINTWISE == toa._POINTWISE_MATERIALS
    assert len(set(bc.MATERIAL_NAMES)) == len(bc.MATERIALS) >= 40
    for what in (0, 3, 4):
        for mi in (0, bc.MI["tex_base"]):
            assert len(bc.inputs(what, mi)) <= bc.N_MAX


def test_the_pairs_reach_both_branches_of_the_basis_choice():
    """normal != ffnormal on some pairs (a basis of its own), equal on others, and on one pair the two differ in the sign of zero
    components only, which `==` calls equal: the zero normal under a V with a NaN (the dot product is NaN, so -normal is taken)."""
    vn, _ = bc.pairs()
    v, n = vn[:, :3], vn[:, 3:]
    with np.errstate(all="ignore"):
        d = (n * -v).sum(axis=1, dtype=F32)
    ff = np.where((d <= 0)[:, None], n, -n)
    same = (ff == n).all(axis=1)
    assert same.any() and (~same).any()
    sign_only = same & (_bits(ff) != _bits(n)).any(axis=1)
    assert sign_only.any(), "no pair where normal and ffnormal differ in the sign of a zero only"


# ---------------------------------------------------------------------------------------------------------------------------
# exact equivalences
# ---------------------------------------------------------------------------------------------------------------------------
EQUIVALENT = [("rough0", "rough0.001"), ("ior0.5", "ior1.0"), ("ior1.0", "ior1.001"), ("ior2.5", "ior2.0"), ("aniso-1", "aniso-0.9"),
              ("aniso1", "aniso0.9"), ("opacity1.5", "opacity1"), ("opacity-0.5", "opacity0")]


@pytest.mark.parametrize("a,b", EQUIVALENT)
def test_clamped_parameters_are_the_clamp_value(oracle, a, b):
    """A parameter outside its range is the range's end: every output of what 0, 3, 4 and 5 has the same bits (opacity: but for
    Material.opacity itself, which is not clamped), over every direction pair and every draw."""
    ia, ib = bc.MI[a], bc.MI[b]
    for what in (0, 3, 4, 5):
        assert np.array_equal(_bits(bc.inputs(what, ia)[:, 1:]), _bits(bc.inputs(what, ib)[:, 1:])), (what, "the two input sets differ")
        ga, gb = np.array(bc.oracle_probe(what, ia)), np.array(bc.oracle_probe(what, ib))
        if what == 0 and a.startswith("opacity"):
            assert not np.array_equal(ga[:, 3], gb[:, 3])
            ga[:, [3, 27]] = gb[:, [3, 27]]
        _same(f"{a} == {b}, what {what}", ga, gb)


def _axis_rows(mi):
    """the rows of inputs(4, mi) under the normals +-z with their local V.z and L.z (exact: the basis' z row is (0, 0, +-1))"""
    vin = bc.inputs(4, mi)
    n = vin[:, 6:9]
    keep = (n[:, 0] == 0) & (n[:, 1] == 0) & (np.abs(n[:, 2]) == 1)
    vin = vin[keep]
    nz, vz, lz, flag = vin[:, 8], vin[:, 5], vin[:, 12], vin[:, 13]
    ffz = np.where(nz * -vz <= 0, nz, -nz)
    bz = np.where(flag == 0, ffz, nz)
    return keep, vin, bz * vz, bz * lz


OPAQUE = ("pointwise0", "pointwise2", "pointwise4", "pointwise5", "pointwise6", "aniso0.9", "opacity1", "opacity1.5", "black_base",
          "base_above_1", "metallic0", "coat_alone", "sheen1_subsurface1", "tints1", "inf_sheen")


@pytest.mark.parametrize("name", OPAQUE)
def test_an_opaque_material_is_black_across_the_surface(oracle, name):
    """specTrans == 0 and L.z * V.z <= 0 (local, the zero vector and +-0 included): f = 0 and pdf = 0 exactly"""
    keep, vin, vz, lz = _axis_rows(bc.MI[name])
    got = bc.oracle_probe(4, bc.MI[name])[keep]
    across = vz * lz <= 0
    assert across.sum() > 500 and (~across).sum() > 500
    assert (got[across] == 0).all()
    assert (got[~across, 3] != 0).any()


@pytest.mark.parametrize("name", ("opacity0", "opacity-0.5", "pointwise8"))
def test_glass_gives_nothing_across_the_surface_upwards(oracle, name):
    """no reflection (L.z * V.z <= 0) and L.z >= 0: the refraction lobe returns 0.  The pdf is 0 * (1 - F): 0, or NaN where the half
    vector is 0 / 0 (V or L the zero vector, or L = -V with L.z > 0, where H = normalize(L + V))."""
    keep, vin, vz, lz = _axis_rows(bc.MI[name])
    got = bc.oracle_probe(4, bc.MI[name])[keep]
    sel = (vz * lz <= 0) & (lz >= 0)
    zero_vec = ~vin[:, 3:6].any(axis=1) | ~vin[:, 10:13].any(axis=1) | (vin[:, 3:6] == -vin[:, 10:13]).all(axis=1)
    assert (sel & ~zero_vec).sum() > 200
    assert (got[sel & ~zero_vec] == 0).all()
    assert (got[sel][:, :3] == 0).all()
    assert ((got[sel & zero_vec, 3] == 0) | np.isnan(got[sel & zero_vec, 3])).all()
    below = (vz > 0) & (lz < 0)
    assert (got[below, 3] > 0).any()                       # and the lobe is there on the other side


def test_a_one_texel_texture_is_its_texel_everywhere(oracle):
    """1 x 1: tu = u * 0, both fractions 0 -- the texel at every uv, +-2^24 and +-inf (wrapped to 0) included.  A NaN coordinate gives
    NaN in every channel (NaN * 0 is the fraction): that is the shader's arithmetic, pinned."""
    uv = bc.inputs(1, bc.TEX["w1h1"])[:, 1:]
    got = bc.oracle_probe(1, bc.TEX["w1h1"])
    texel = bc.texture_bytes()["w1h1"][0, 0].astype(F32) / F32(255.0)
    nan = np.isnan(uv).any(axis=1)
    assert nan.sum() > 100 and np.isnan(got[nan]).all()
    assert np.array_equal(got[~nan], np.broadcast_to(np.tile(texel, 5), got[~nan].shape))


@pytest.mark.parametrize("name", bc.TEXTURE_NAMES)
def test_texel_exact_uv_returns_the_texel(oracle, name):
    """u = k / (W - 1) and v = j / (H - 1) wherever the float32 product with the extent is the whole number again: channel / 255"""
    t = bc.texture_bytes()[name]
    h, w = t.shape[:2]
    uv = bc.inputs(1, bc.TEX[name])[:, 1:]
    got = bc.oracle_probe(1, bc.TEX[name])
    with np.errstate(all="ignore"):
        tu, tv = uv[:, 0] * F32(w - 1), uv[:, 1] * F32(h - 1)
        ok = (uv >= 0).all(axis=1) & (uv <= 1).all(axis=1) & (tu == np.floor(tu)) & (tv == np.floor(tv))
    assert ok.sum() >= w * h
    x, y = tu[ok].astype(int), tv[ok].astype(int)
    assert len(set(zip(x.tolist(), y.tolist()))) == w * h                   # every texel is asked for
    want = t[y, x].astype(F32) / F32(255.0)
    assert np.array_equal(got[ok], np.tile(want, (1, 5)))
    assert (got[:, :4] == got[:, 4:8]).all() or np.isnan(got).any()


@pytest.mark.parametrize("name", bc.MATERIAL_NAMES)
def test_one_fetch_counts_its_slots(oracle, name):
    """what 0: 1 material fetch, one descriptor per texture slot in use, four texels per slot in use"""
    slots = sum(1 for k in ("tex_base", "tex_mr", "tex_emission", "tex_occlusion") if bc.MATERIALS[bc.MI[name]][1].get(k, -1) >= 0)
    got = bc.oracle_probe(0, bc.MI[name])
    assert (got[:, 48] == 1).all() and (got[:, 49] == slots).all() and (got[:, 50] == 4 * slots).all()
    _same(name, got[:, :24], got[:, 24:48])


@pytest.mark.parametrize("name", bc.MATERIAL_NAMES)
def test_lobe_probabilities_are_not_negative(oracle, name):
    got = bc.oracle_probe(3, bc.MI[name])[:, 10:15]
    fin = np.isfinite(got).all(axis=1)
    assert (got[fin] >= 0).all()
    if name not in ("nan_roughness", "inf_sheen"):
        assert fin.sum() > 0.5 * len(got)
        assert np.abs(got[fin].sum(axis=1, dtype=F64) - 1.0).max() < 1e-5


@pytest.mark.parametrize("name", bc.MATERIAL_NAMES)
def test_sampling_draws_three_numbers(oracle, name):
    """the RNG state after SampleBRDF is three steps on, whichever lobe is taken (NaN results included)"""
    vin, got = bc.inputs(5, bc.MI[name]), bc.oracle_probe(5, bc.MI[name])
    assert np.array_equal(_bits(got[:, 7]), bc.third_draw(_bits(vin[:, 10]))[1])


def test_the_boundary_draws_sit_on_the_boundaries(oracle):
    """inputs(5, .) ends in draws whose r3 is cdf0, cdf2 or cdf3 of their pair or a float beside it: some material has all three, and
    across such a boundary the sampled lobe changes (the direction does)"""
    seen = set()
    for name in ("pointwise9", "ior2.0", "rough0"):
        mi = bc.MI[name]
        rows = bc.inputs(5, mi)[bc.boundary_rows(mi)]
        assert len(rows) >= 27, (name, len(rows))
        lobes = bc.oracle_run(3, rows[:, :10])[:, 10:14].astype(F32)
        cdf0 = lobes[:, 0]
        cdf2 = (cdf0 + lobes[:, 1]).astype(F32) + lobes[:, 2]
        cdf3 = cdf2 + lobes[:, 3]
        r3, _ = bc.third_draw(_bits(rows[:, 10]))
        for k, c in enumerate((cdf0, cdf2, cdf3)):
            near = np.abs(_bits(r3).astype(np.int64) - _bits(c).astype(np.int64)) <= 1
            if near.any() and (r3[near] < c[near]).any() and (r3[near] >= c[near]).any():
                seen.add(k)
    assert seen == {0, 1, 2}


def test_glass_samples_reflect_and_refract(oracle):
    """r3' falls on either side of F: both outcomes, from outside and from inside, and total internal reflection at grazing V inside"""
    mi = bc.MI["opacity0"]
    vin, got = bc.inputs(5, mi), bc.oracle_probe(5, mi)
    axis = (vin[:, 6] == 0) & (vin[:, 7] == 0) & (np.abs(vin[:, 8]) == 1) & (vin[:, 9] == 0)
    vz, lz, nz = vin[axis, 5], got[axis, 2], vin[axis, 8]
    ok = np.isfinite(got[axis]).all(axis=1) & (got[axis, 6] > 0)
    for inside in (False, True):
        sel = ok & ((vz * nz < 0) == inside) & (np.abs(vz) == 0.5)
        assert (vz[sel] * lz[sel] > 0).sum() > 20 and (vz[sel] * lz[sel] < 0).sum() > 20, inside


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 transcription of tests/test_oracle_analytic.py on the new materials
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.TRANSCRIBED)
def test_eval_brdf_against_the_second_transcription(oracle, name):
    """test_oracle_analytic's pointwise check, its filter and its bounds (|L.z| > 0.05, 2e-3 worst, 2e-6 median, 90 % of the points kept),
    on the new finite materials of roughness >= 0.15"""
    import ctypes as C
    from test_oracle_analytic import _np_eval_brdf
    lib = oracle.load_oracle()
    md = np.ascontiguousarray(bc.materials()[bc.MI[name]], dtype=F32)
    assert np.isfinite(md).all() and md[9] >= 0.15 and (md[22:27] < 0).all()
    rng = np.random.RandomState(900 + bc.MI[name])
    n = 4000
    L = rng.normal(size=(n, 3)); L /= np.linalg.norm(L, axis=-1, keepdims=True)
    L = np.ascontiguousarray(L.astype(F32))
    for N, V in (((0.0, 0.0, 1.0), (0.3, 0.2, 0.9)), ((0.3, -0.5, 0.8), (0.7, 0.1, 0.4)), ((-0.2, 0.9, -0.4), (0.1, 0.8, 0.1))):
        N = np.ascontiguousarray((np.array(N, F64) / np.linalg.norm(N)).astype(F32))
        V = np.ascontiguousarray((np.array(V) / np.linalg.norm(V)).astype(F32))
        out = np.zeros((n, 4), F32)
        lib.oracle_eval_brdf_batch(md.ctypes.data, V.ctypes.data, N.ctypes.data, C.c_float(0.0), L.ctypes.data, C.c_uint64(n), out.ctypes.data)
        f64, p64 = _np_eval_brdf(md, np.broadcast_to(V.astype(F64), (n, 3)), N.astype(F64), L.astype(F64))
        got = out.astype(F64)
        Lz = L.astype(F64) @ (N.astype(F64) / np.linalg.norm(N))
        ok = (np.abs(Lz) > 0.05) & np.isfinite(f64).all(axis=-1) & np.isfinite(p64)
        scale = np.maximum(np.abs(f64).max(axis=-1), 1e-3)
        err_f = np.abs(got[:, :3] - f64).max(axis=-1) / scale
        err_p = np.abs(got[:, 3] - p64) / np.maximum(np.abs(p64), 1e-3)
        assert ok.sum() > 0.9 * n, (name, int(ok.sum()))
        assert err_f[ok].max() < 2e-3 and err_p[ok].max() < 2e-3, (name, err_f[ok].max(), err_p[ok].max())
        assert np.median(err_f[ok]) < 2e-6 and np.median(err_p[ok]) < 2e-6


# ---------------------------------------------------------------------------------------------------------------------------
# the helpers against a float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _norm(v):
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _helper64(name, a):
    """util/sampling.hlsl and util/common.hlsl restated in float64 over operand columns a[:, k]; returns (n, results)"""
    c = [a[:, k] for k in range(a.shape[1])]
    pi = np.pi
    if name == "gtr1":
        a2 = c[1] * c[1]
        return ((a2 - 1) / (pi * np.log(a2) * (1 + (a2 - 1) * c[0] * c[0])))[:, None]
    if name == "sample_gtr1":
        al = np.maximum(0.001, c[0]); a2 = al * al
        ct = np.sqrt((1 - a2 ** (1 - c[2])) / (1 - a2))
        st = np.clip(np.sqrt(1 - ct * ct), 0, 1)
        return np.stack([st * np.cos(2 * pi * c[1]), st * np.sin(2 * pi * c[1]), ct], -1)
    if name == "sample_ggx_vndf":
        V, ax, ay, r1, r2 = np.stack(c[:3], -1), c[3], c[4], c[5], c[6]
        Vh = _norm(np.stack([ax * V[:, 0], ay * V[:, 1], V[:, 2]], -1))
        lensq = Vh[:, 0] ** 2 + Vh[:, 1] ** 2
        T1 = np.stack([-Vh[:, 1], Vh[:, 0], np.zeros_like(lensq)], -1) / np.sqrt(lensq)[:, None]
        T2 = np.cross(Vh, T1)
        r, phi = np.sqrt(r1), 2 * pi * r2
        t1, t2 = r * np.cos(phi), r * np.sin(phi)
        s = 0.5 * (1 + Vh[:, 2])
        t2 = (1 - s) * np.sqrt(1 - t1 * t1) + s * t2
        Nh = t1[:, None] * T1 + t2[:, None] * T2 + np.sqrt(np.maximum(0, 1 - t1 * t1 - t2 * t2))[:, None] * Vh
        return _norm(np.stack([ax * Nh[:, 0], ay * Nh[:, 1], np.maximum(0, Nh[:, 2])], -1))
    if name == "gtr2_aniso":
        q = (c[1] / c[3]) ** 2 + (c[2] / c[4]) ** 2 + c[0] ** 2
        return (1 / (pi * c[3] * c[4] * q * q))[:, None]
    if name == "smith_g":
        a2, b2 = c[1] * c[1], c[0] * c[0]
        return (2 * c[0] / (c[0] + np.sqrt(a2 + b2 - a2 * b2)))[:, None]
    if name == "smith_g_aniso":
        return (2 * c[0] / (c[0] + np.sqrt((c[1] * c[3]) ** 2 + (c[2] * c[4]) ** 2 + c[0] ** 2)))[:, None]
    if name == "schlick_weight":
        return (np.clip(1 - c[0], 0, 1) ** 5)[:, None]
    if name == "dielectric_fresnel":
        ci, e = c
        s2 = e * e * (1 - ci * ci)
        ct = np.sqrt(np.maximum(1 - s2, 0))
        rs, rp = (e * ct - ci) / (e * ct + ci), (e * ci - ct) / (e * ci + ct)
        return np.where(s2 > 1, 1.0, 0.5 * (rs * rs + rp * rp))[:, None]
    if name == "cosine_sample_hemisphere":
        r, phi = np.sqrt(c[0]), 2 * pi * c[1]
        x, y = r * np.cos(phi), r * np.sin(phi)
        return np.stack([x, y, np.sqrt(np.maximum(0, 1 - x * x - y * y))], -1)
    if name == "power_heuristic":
        return (c[0] ** 2 / (c[1] ** 2 + c[0] ** 2))[:, None]
    i, n = np.stack(c[:3], -1), (np.stack(c[3:6], -1) if len(c) >= 6 else None)
    if name == "reflect3":
        return i - 2 * (n * i).sum(-1, keepdims=True) * n
    if name == "refract3":
        e = c[6][:, None]
        d = (n * i).sum(-1, keepdims=True)
        k = 1 - e * e * (1 - d * d)
        return np.where(k < 0, 0.0, e * i - (e * d + np.sqrt(np.maximum(k, 0))) * n)
    if name == "make_onb":
        z = _norm(i)
        k = 1 / np.maximum(1 + z[:, 2], 0.00001)
        p = z[:, 1] * k
        b, q = z[:, 1] * p, -z[:, 0] * p
        x = _norm(np.stack([z[:, 2] + b, q, -z[:, 0]], -1))
        y = _norm(np.stack([q, 1 - b, -z[:, 1]], -1))
        return np.concatenate([x, y, z], -1)
    if name == "luminance3":
        return (0.299 * c[0] + 0.587 * c[1] + 0.114 * c[2])[:, None]
    raise ValueError(name)


def _helper_error(name):
    """the oracle's worst error over helper_domain(name), in float32 ulps of the float64 value (of its largest component, where the
    result is a vector: the others are sums that cancel)"""
    k = bc.HELPERS.index(name)
    dom = bc.helper_domain(name)
    got = bc.oracle_probe(2, k)[-len(dom):, :bc.RESULTS.get(name, 1)].astype(F64)
    assert np.array_equal(bc.inputs(2, k)[-len(dom):, 1:1 + bc.ARITY[name]], dom)
    with np.errstate(all="ignore"):
        ref = _helper64(name, dom.astype(F64))
    assert np.isfinite(ref).all() and np.isfinite(got).all(), name
    if name == "make_onb":                       # three vectors
        got, ref = got.reshape(-1, 3), ref.reshape(-1, 3)
    ulp = np.spacing(np.abs(ref).max(axis=1).astype(F32)).astype(F64)
    return float((np.abs(got - ref).max(axis=1) / ulp).max())


# measured on the CPU over bsdf_cases.helper_domain (this test prints the figures); the bound is about twice the measurement, rounded up
HELPER_ULP = {             # name: (measured, bound)
    "gtr1": (8.5649, 18), "sample_gtr1": (49.1488, 100), "sample_ggx_vndf": (24.5065, 50), "gtr2_aniso": (7.2577, 15), "smith_g": (1.9141, 4),
    "smith_g_aniso": (2.1515, 5), "schlick_weight": (5.7988, 12), "dielectric_fresnel": (13.1072, 27), "cosine_sample_hemisphere": (6.1054, 13),
    "power_heuristic": (2.1392, 5), "reflect3": (3.4607, 7), "refract3": (8.7898, 18), "make_onb": (13.3495, 27), "luminance3": (1.6623, 4),
}
# Where the figures come from: sample_gtr1 forms sinTheta = sqrt(1 - cosTheta^2) with cosTheta near 1 (a sharp lobe), sample_ggx_vndf
# sqrt(1 - t1^2 - t2^2) near the rim of the disc, make_onb 1 / (1 + z) down to z = -0.9, dielectric_fresnel rs and rp as differences;
# schlick_weight is 1 - u followed by four multiplications at small 1 - u.  Each is the shader's own float32 arithmetic.


@pytest.mark.parametrize("name", bc.HELPERS)
def test_helpers_against_a_float64_restatement(oracle, name):
    err = _helper_error(name)
    measured, bound = HELPER_ULP[name]
    print(f"{name}: measured {err:.4f} ulp (recorded {measured}, bound {bound})")
    assert err <= bound, (name, err, bound)


def test_helpers_at_their_branch_points(oracle):
    """the known answers on the boundaries: gtr1 at a >= 1, total internal reflection, the zero vector's basis, the clamp of k"""
    def run(name, *rows):
        vin = np.zeros((len(rows), 8), F32)
        vin[:, 0] = bc.HELPERS.index(name)
        for r, row in enumerate(rows):
            vin[r, 1:1 + len(row)] = row
        return bc.oracle_run(2, vin)
    below = np.nextafter(F32(1), F32(0))
    g = run("gtr1", (0.3, 1.0), (0.3, 2.0), (0.3, below))
    assert g[0, 0] == g[1, 0] == F32(1 / np.pi) and g[2, 0] != g[0, 0] and abs(g[2, 0] - 1 / np.pi) < 1e-5
    f = run("dielectric_fresnel", (0.5, 2.0), (0.9, 2.0), (1.0, 1.5))
    assert f[0, 0] == 1.0 and 0 < f[1, 0] < 1 and abs(f[2, 0] - 0.04) < 1e-6
    r = run("refract3", (0.8, 0, -0.6, 0, 0, 1, 2.0), (0.0, 0, -1.0, 0, 0, 1, 2.0))
    assert (r[0, :3] == 0).all() and np.array_equal(r[1, :3], [0, 0, -1])
    o = run("make_onb", (0, 0, 0), (-0.0, -0.0, -0.0), (0, 0, 1), (0, 0, -1))
    ident = np.eye(3, dtype=F32).ravel()
    assert np.array_equal(o[0], ident) and np.array_equal(o[1], ident) and np.array_equal(o[2], ident)
    assert np.array_equal(np.abs(o[3]), ident) and o[3, 0] == -1 and o[3, 8] == -1 and o[3, 4] == 1          # k = 1e5 and y = 0: x = (-1, 0, 0)
    v = run("sample_ggx_vndf", (0, 0, 1, 0.3, 0.3, 0.0, 0.5), (0, 0, 1, 0.3, 0.3, 0.25, 0.0))
    assert np.array_equal(v[0, :3], [0, 0, 1]) and v[1, 0] > 0 and v[1, 1] == 0                           # lensq == 0: T1 = (1, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# recorded results
# ---------------------------------------------------------------------------------------------------------------------------
def sample_record(mi):
    """of what 5 over inputs(5, mi): [elements, results with a NaN in L, f or pdf, draws of the diffuse lobe, of a reflection lobe, of
    glass, of the coat] -- the lobe from r3 against the oracle's own cdf (float32 sums, as SampleBRDF forms them)"""
    vin, got = bc.inputs(5, mi), bc.oracle_probe(5, mi)
    w = bc.oracle_run(3, vin[:, :10])[:, 10:14].astype(F32)
    with np.errstate(all="ignore"):
        cdf0 = w[:, 0]
        cdf2 = (cdf0 + w[:, 1]).astype(F32) + w[:, 2]
        cdf3 = cdf2 + w[:, 3]
        r3, _ = bc.third_draw(_bits(vin[:, 10]))
        lobe = np.where(r3 < cdf0, 0, np.where(r3 < cdf2, 1, np.where(r3 < cdf3, 2, 3)))
    return [len(vin), int(np.isnan(got[:, :7]).any(axis=1).sum())] + [int(v) for v in np.bincount(lobe, minlength=4)]


def test_sampling_matches_the_record(oracle):
    """NaN count and lobe histogram per material as recorded in tests/golden: a silent change of the oracle shows here"""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {name: sample_record(mi) for mi, name in enumerate(bc.MATERIAL_NAMES)}
    assert got == want, {k: (got[k], want.get(k)) for k in got if got[k] != want.get(k)}
