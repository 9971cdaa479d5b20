"""Lightmap charts (include/ptmi_plugin.h Part 14) without a GPU: exports and struct layout, the host twins against the numpy
restatement of the rule (chart_ref.py) byte for byte, the geometry of a floor quad's receivers, the resolve, the sanitizer program
and the compile-time resources of the kernels.  tests/test_gpu_lightmap.py holds the kernels to the twins.

Every statement about a case's content (ties, overlaps, exclusions) is asserted on the numpy reference before anything is compared."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from kernel_resources import resources
import chart_cases as cases
import chart_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["PTRasterizeChart", "PTRasterizeChartHost", "PTResolveLightmap", "PTResolveLightmapHost"]
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_lightmap_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    part14 = header[header.index("Part 14: lightmap charts"):]
    for name in SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in part14, name
        assert getattr(lib, name).restype is C.c_int


def test_chart_desc_matches_c_header():
    fields = ["structSize", "bvhOffset", "triOffset", "triAttributeOffset", "triangleCount", "instance", "width", "height", "seedBase", "reserved"]
    lines = ['printf("PTChartDesc %zu\\n", sizeof(PTChartDesc));'] + [f'printf("{f} %zu\\n", offsetof(PTChartDesc, {f}));' for f in fields]
    lines += ['printf("MAX_SIZE %u\\n", PT_CHART_MAX_SIZE);', 'printf("MAX_DILATE %u\\n", PT_CHART_MAX_DILATE);']
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTChartDesc"]) == C.sizeof(abi.PTChartDesc) == 48
    for f in fields:
        assert int(got[f]) == getattr(abi.PTChartDesc, f).offset, f
    assert [int(got[f]) for f in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]
    assert int(got["MAX_SIZE"]) == abi.PT_CHART_MAX_SIZE == 8192 and int(got["MAX_DILATE"]) == abi.PT_CHART_MAX_DILATE == 16


def test_null_context_is_named():
    lib = plugin.load_library()
    d = abi.chart_desc(4, 4, 2)
    buf = (C.c_float * 256)()
    count = C.c_uint64(7)
    assert lib.PTRasterizeChart(None, C.byref(d), None, C.addressof(buf), C.addressof(buf), 4, C.byref(count)) == abi.PT_ERR_INVALID_ARG
    assert b"PTRasterizeChart" in lib.PTGetLastError() and b"ctx == NULL" in lib.PTGetLastError()
    assert lib.PTResolveLightmap(None, C.addressof(buf), C.addressof(buf), 1, 4, 4, 0, C.addressof(buf)) == abi.PT_ERR_INVALID_ARG
    assert b"PTResolveLightmap" in lib.PTGetLastError() and b"ctx == NULL" in lib.PTGetLastError()


# ---------------------------------------------------------------------------------------------------------------------------
# the host twin against numpy
# ---------------------------------------------------------------------------------------------------------------------------
def _same(got, ref):
    texels, recv = got
    assert texels.dtype == np.uint32 and recv.dtype == np.float32 and recv.shape == (len(texels), 8)
    assert np.array_equal(texels, ref["texels"]), (len(texels), len(ref["texels"]))
    diff = np.nonzero((_bits(recv) != _bits(ref["recv"])).any(axis=1))[0]
    assert len(diff) == 0, (len(diff), recv[diff[:3]], ref["recv"][diff[:3]])


@pytest.fixture(scope="module")
def quad():
    verts, attrs = cases.quad_mesh()
    return cases.blas_of(verts), attrs


@pytest.fixture(scope="module")
def zoo():
    verts, attrs, caller = cases.zoo_mesh()
    tris = cases.blas_of(verts)
    prim = chart_ref.records(tris)[3]
    assert sorted(prim.tolist()) == list(range(cases.ZOO_TRIANGLES))
    assert not np.array_equal(prim, np.arange(cases.ZOO_TRIANGLES)), "the tree keeps the input order: the case would not tell primIdx from the record index"
    return tris, attrs, caller


@pytest.mark.parametrize("size", cases.QUAD_SIZES)
def test_quad_covers_every_texel_once(quad, size):
    tris, attrs = quad
    w, h = size
    ref = chart_ref.rasterize(tris, attrs, w, h, seed=cases.WRAP_SEED)
    assert len(ref["texels"]) == w * h and (ref["cover"] >= 1).all()
    assert (ref["cover"] == 2).any() == ref["on_edge"]            # only a sample on the diagonal is covered twice
    # A sample (256 x + 128, 256 y + 128) lies on the diagonal from (0, 0) to (256 w, 256 h) when 2 (y w - x h) = h - w: never
    # when h - w is odd (130 x 67), otherwise somewhere (1 x 1, 7 x 5 and 64 x 64 each have one)
    assert ref["on_edge"] == ((h - w) % 2 == 0), "no sample lies on the diagonal"
    if w * h > 1:
        assert ref["owners"] == {0, 1}
    seeds = ref["recv"][:, 3].view(np.uint32)
    assert seeds[0] == cases.WRAP_SEED and (w * h <= 16 or seeds[16] == 0), "the seeds must wrap"
    _same(plugin.rasterize_chart(tris, attrs, w, h, seed=cases.WRAP_SEED), ref)


def _zoo_facts(ref, w, h, caller):
    """what the zoo is for, shown on the reference"""
    cov, owners = ref["covered"], ref["owners"]
    shared = ref["shared01"]
    assert shared.sum() >= 20 and (ref["owner"][shared] == cases.OVER_A).all(), int(shared.sum())
    assert cov[cases.OVER_B] > shared.sum() and cases.OVER_B in owners
    for p in (cases.ZERO_AREA_UV, cases.FLAT_IN_SPACE, cases.WHOLLY_OUT, cases.TOO_FAR, cases.SUB_TEXEL):
        assert cov[p] == 0 and p not in owners, p
    assert (cov[cases.NAN_UV] == 0) == caller
    assert 0 < cov[cases.PARTLY_OUT] and cases.PARTLY_OUT in owners
    assert cases.ZERO_NORMAL in owners
    rows = ref["recv"][ref["owner"].reshape(-1)[ref["texels"]] == cases.ZERO_NORMAL]
    assert len(rows) and np.isfinite(rows[:, 4:7]).all(), "the geometric normal must take the zero normal's place"
    assert cases.BIG in owners and cov[cases.BIG] > 0.3 * w * h
    assert (ref["cover"] > 1).sum() > 20 and (ref["owner"] == chart_ref.NO_OWNER).any()
    assert np.isfinite(ref["recv"][:, :3]).all() and np.isfinite(ref["recv"][:, 4:7]).all()
    n = np.linalg.norm(ref["recv"][:, 4:7].astype(np.float64), axis=1)
    assert np.abs(n - 1).max() < 1e-5


@pytest.mark.parametrize("size", cases.ZOO_SIZES + [(300, 300)])
@pytest.mark.parametrize("variant", ["attr_uvs", "caller_uvs_instance"])
def test_zoo_host_twin_equals_numpy(zoo, size, variant):
    tris, attrs, caller = zoo
    w, h = size
    kw = {}
    if variant == "caller_uvs_instance":
        l2w, w2l, _ = cases.instance_matrix()
        kw = dict(uvs=caller, l2w=l2w, w2l=w2l)
    ref = chart_ref.rasterize(tris, attrs, w, h, seed=5, **kw)
    _zoo_facts(ref, w, h, variant == "caller_uvs_instance")
    if size == (300, 300):
        assert ref["covered"][cases.BIG] > 64 * 64, "no triangle covers more than 64 x 64 texels"
        blocks = np.add.reduceat((ref["owner"].reshape(-1) != chart_ref.NO_OWNER).astype(np.int64), np.arange(0, w * h, 256))
        assert (blocks == 0).sum() >= 1 and (blocks > 0).sum() >= 100 and ((blocks > 0) & (blocks < 256)).any()
    got = plugin.rasterize_chart(tris, attrs, w, h, uvs=kw.get("uvs"), local_to_world=kw.get("l2w"), world_to_local=kw.get("w2l"), seed=5)
    _same(got, ref)


def test_mirrored_chart_is_the_same_coverage(zoo):
    """the caller's UVs are the attribute UVs with u and v swapped: on a square atlas the owner map is the transpose"""
    tris, attrs, caller = zoo
    a = chart_ref.rasterize(tris, attrs, 64, 64)["owner"]
    caller = caller.copy()
    caller[cases.NAN_UV] = np.concatenate([attrs[cases.NAN_UV][f"uv{c}"][::-1] for c in range(3)])
    b = chart_ref.rasterize(tris, attrs, 64, 64, uvs=caller)["owner"]
    assert np.array_equal(a, b.T)


def test_floor_quad_geometry(quad):
    """position within 2e-6 of origin + u * eu + v * ev at the texel centre (fewer than ten roundings of 2^-24 at magnitude 2),
    the quad's normal exactly, texel (0, 0) at the origin's corner"""
    tris, attrs = quad
    W = H = 16
    texels, recv = plugin.rasterize_chart(tris, attrs, W, H)
    assert np.array_equal(texels, np.arange(W * H))
    x, y = texels % W, texels // W
    u, v = (x + 0.5) / W, (y + 0.5) / H
    want = np.asarray(cases.QUAD_ORIGIN)[None, :] + u[:, None] * np.asarray(cases.QUAD_EU)[None, :] + v[:, None] * np.asarray(cases.QUAD_EV)[None, :]
    err = np.abs(recv[:, :3].astype(np.float64) - want).max()
    print(f"[lightmap] floor quad: largest position error {err:.3e}")
    assert err <= 2e-6
    assert (recv[:, 4:7] == np.asarray(cases.QUAD_NORMAL, F)[None, :]).all()
    d = np.linalg.norm(recv[:, :3].astype(np.float64) - np.asarray(cases.QUAD_ORIGIN), axis=1)
    assert d.argmin() == 0 and np.allclose(recv[0, :3], (-1 + 1 / 16, 0, -1 + 1 / 16), atol=2e-6)
    assert recv[1, 0] > recv[0, 0] and recv[1, 2] == recv[0, 2] and recv[W, 2] > recv[0, 2]      # x runs along eu, y along ev


def test_host_twin_refusals(quad):
    tris, attrs = quad
    lib = plugin.load_library()
    for w, h in ((0, 4), (8193, 4), (4, 0), (4, 8193)):
        with pytest.raises(plugin.PluginError, match="8192"):
            plugin.rasterize_chart(tris, attrs, w, h)
    d = abi.chart_desc(8, 8, 2)
    count = C.c_uint64()
    texels, recv = np.full(70, 0xABCDABCD, np.uint32), np.full((70, 8), 7.5, F)
    assert lib.PTRasterizeChartHost(C.byref(d), tris.ctypes.data, attrs.ctypes.data, None, None, None, texels.ctypes.data, recv.ctypes.data, 63, C.byref(count)) == 0
    assert count.value == 64 and (texels == 0xABCDABCD).all() and (recv == 7.5).all()
    assert lib.PTRasterizeChartHost(C.byref(d), tris.ctypes.data, attrs.ctypes.data, None, None, None, texels.ctypes.data, recv.ctypes.data, 70, C.byref(count)) == 1
    assert count.value == 64 and (texels[64:] == 0xABCDABCD).all() and (recv[64:] == 7.5).all() and np.array_equal(texels[:64], np.arange(64))
    d.reserved[1] = 1
    assert lib.PTRasterizeChartHost(C.byref(d), tris.ctypes.data, attrs.ctypes.data, None, None, None, None, None, 0, C.byref(count)) == 0
    assert b"reserved" in lib.PTGetBVHBuildError()


# ---------------------------------------------------------------------------------------------------------------------------
# resolve
# ---------------------------------------------------------------------------------------------------------------------------
def test_resolve_twin_equals_numpy(zoo):
    tris, attrs, _ = zoo
    w, h = 37, 23
    texels = chart_ref.rasterize(tris, attrs, w, h)["texels"]
    rng = np.random.RandomState(3)
    irr = rng.uniform(0, 4, (len(texels), 4)).astype(F)
    scatter = np.zeros((h * w, 4), F)
    scatter[texels, :3], scatter[texels, 3] = irr[:, :3], 1.0
    assert (_bits(plugin.resolve_lightmap(texels, irr, w, h, dilate=0)) == _bits(scatter.reshape(h, w, 4))).all()          # the scatter alone
    for dilate in (0, 1, 2, 4, 16):
        want = chart_ref.resolve(texels, irr, w, h, dilate)
        got = plugin.resolve_lightmap(texels, irr, w, h, dilate=dilate)
        assert got.shape == (h, w, 4) and (_bits(got) == _bits(want)).all(), dilate
    assert ((chart_ref.resolve(texels, irr, w, h, 2)[..., 3] == 0.5).sum()) > 20


@pytest.mark.parametrize("at", ["middle", "corner"])
def test_one_texel_grows_by_a_ring_per_pass(at):
    w = h = 9
    x, y = (4, 4) if at == "middle" else (8, 0)
    texels, irr = np.array([y * w + x], np.uint32), np.array([[0.25, 1.5, 3.0, 9.0]], F)
    for k in range(0, 5):
        got = plugin.resolve_lightmap(texels, irr, w, h, dilate=k)
        assert (_bits(got) == _bits(chart_ref.resolve(texels, irr, w, h, k))).all()
        ys, xs = np.mgrid[0:h, 0:w]
        ring = np.maximum(np.abs(ys - y), np.abs(xs - x))
        assert ((got[..., 3] != 0) == (ring <= k)).all()
        if at == "middle":
            assert (got[..., 3] != 0).sum() == (2 * k + 1) ** 2
        assert got[y, x, 3] == 1.0 and (got[..., 3][(ring >= 1) & (ring <= k)] == 0.5).all()
        assert (got[..., :3][ring <= k] == irr[0, :3]).all()           # a mean of equal values is that value


def test_resolve_refusals():
    irr = np.ones((1, 4), F)
    with pytest.raises(plugin.PluginError, match="width \\* height"):
        plugin.resolve_lightmap(np.array([81], np.uint32), irr, 9, 9, dilate=1)
    with pytest.raises(plugin.PluginError, match="16"):
        plugin.resolve_lightmap(np.array([3], np.uint32), irr, 9, 9, dilate=17)
    with pytest.raises(plugin.PluginError, match="8192"):
        plugin.resolve_lightmap(np.array([0], np.uint32), irr, 0, 9, dilate=1)


# ---------------------------------------------------------------------------------------------------------------------------
# the sanitizers and the kernels' resources
# ---------------------------------------------------------------------------------------------------------------------------
def test_host_twin_under_sanitizers(tmp_path):
    """`make lightmap-sanitize`: chart_host.cpp and csrc/lightmap_sanitize_main.cpp (its own main) with -fsanitize=address,undefined,
    built and run, nothing preloaded: it rasterises, resolves and makes the refusals, and must finish without a report."""
    csrc = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "lightmap-sanitize", "LIGHTMAP_SANITIZE_OUT=" + str(tmp_path / "lightmap_sanitize")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "lightmap ok" in out.stdout, out.stdout + out.stderr


KERNELS = ["pt_lm_coverage", "pt_lm_coverage_large", "pt_lm_count", "pt_lm_scan", "pt_lm_emit", "pt_lm_scatter", "pt_lm_dilate"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_lightmap_kernels_fit_the_shade_kernels_budget():
    with ThreadPoolExecutor(3) as ex:
        fa = ex.submit(resources, "pt_wavefront.hip", "a")
        fb = ex.submit(resources, "pt_wavefront.hip", "b")
        fl = ex.submit(resources, "pt_lightmap.hip")
        res_a, res_b, res_l = fa.result(), fb.result(), fl.result()
    assert len(res_l) == len(KERNELS) and all("pt_lm_" in k for k in res_l), sorted(res_l)
    for name in KERNELS:
        assert len([k for k in res_l if f"{len(name)}{name}E" in k]) == 1, (name, sorted(res_l))
    for unit, res in (("a", res_a), ("b", res_b)):
        shade = [v for k, v in res.items() if "pt_wf_shadeILb0E" in k and "PTRayMap" in k]
        assert len(shade) == 1, sorted(res)
        for k, r in res_l.items():
            print(f"[resources] {k}: {r}  (unit {unit} shade: {shade[0]})")
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
            assert r["vgprs"] <= shade[0]["vgprs"], (k, r, shade[0])
        assert not [k for k in res if "pt_lm_" in k], sorted(res)
    res_g = resources("pt_gather.hip")
    assert not [k for k in res_g if "pt_lm_" in k], sorted(res_g)
