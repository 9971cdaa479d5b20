"""The lightmap denoiser (include/ptmi_plugin.h Part 17) without a GPU: exports and struct layout, every refusal, the host twin
against the numpy restatement of the rule (lmfilter_ref.py) bit for bit, what the filter is for -- no light crosses a chart seam
or a fold, a constant image stays, noise falls --, the sanitizer program and the compile-time resources of the kernels (DESIGN.md
5.22).  tests/test_gpu_lightmap_denoise.py holds the kernels to the twin.

Every statement about a case's content is asserted on the numpy reference or on the case itself before anything is compared."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from kernel_resources import resources
import lmfilter_cases as cases
import lmfilter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["PTDenoiseLightmap", "PTDenoiseLightmapHost"]
F = np.float32
# 25 products, 24 adds and a divide of equal values, each within 2^-24 relative, and as much again for the weights' own sum
EQUAL_TOL = (2 * 25 + 2) * 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_lmfilter_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    part17 = header[header.index("Part 17: the lightmap denoiser"):]
    for name in SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in part17, name
        assert getattr(lib, name).restype is C.c_int


def test_params_match_c_header():
    fields = ["structSize", "samples", "iterations", "normalPower", "sigmaLuminance", "sigmaPosition", "sigmaPlane", "reserved"]
    lines = ['printf("PTLightmapDenoiseParams %zu\\n", sizeof(PTLightmapDenoiseParams));']
    lines += [f'printf("{f} %zu\\n", offsetof(PTLightmapDenoiseParams, {f}));' for f in fields]
    lines += ['printf("MAX_ITERATIONS %u\\n", PT_LMFILTER_MAX_ITERATIONS);', 'printf("MAX_NORMAL_POWER %u\\n", PT_LMFILTER_MAX_NORMAL_POWER);',
              'printf("MAX_SAMPLES %u\\n", PT_LMFILTER_MAX_SAMPLES);']
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTLightmapDenoiseParams"]) == C.sizeof(abi.PTLightmapDenoiseParams) == 48
    for f in fields:
        assert int(got[f]) == getattr(abi.PTLightmapDenoiseParams, f).offset, f
    assert [int(got[f]) for f in fields] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert int(got["MAX_ITERATIONS"]) == abi.PT_LMFILTER_MAX_ITERATIONS == 8
    assert int(got["MAX_NORMAL_POWER"]) == abi.PT_LMFILTER_MAX_NORMAL_POWER == 7
    assert int(got["MAX_SAMPLES"]) == abi.PT_LMFILTER_MAX_SAMPLES == 1 << 24
    p = abi.lightmap_denoise_params(16)
    assert (p.structSize, p.samples, p.iterations, p.normalPower) == (48, 16, 5, 5)
    assert (p.sigmaLuminance, p.sigmaPosition, p.sigmaPlane) == (4.0, 4.0, 1.0) and not any(p.reserved)


def test_null_context_is_named():
    lib = plugin.load_library()
    p = abi.lightmap_denoise_params(16)
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    assert lib.PTDenoiseLightmap(None, C.byref(p), a, a, a, 1, 4, 4, a) == abi.PT_ERR_INVALID_ARG
    assert b"PTDenoiseLightmap" in lib.PTGetLastError() and b"ctx == NULL" in lib.PTGetLastError()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals of the twin (the context's entry point shares check_params and check_size with it)
# ---------------------------------------------------------------------------------------------------------------------------
def _small():
    texels, recv, irr, _ = cases.generated_list(7, 5, seed=2, bad=False, isolated=False)
    return texels, recv, irr


REFUSED_PARAMS = [
    ("samples", dict(samples=1)), ("samples", dict(samples=0)), ("samples", dict(samples=(1 << 24) + 1)),
    ("iterations", dict(iterations=9)), ("normalPower", dict(normal_power=8)),
    ("sigmaLuminance", dict(sigma_luminance=0.0)), ("sigmaLuminance", dict(sigma_luminance=float("nan"))),
    ("sigmaPosition", dict(sigma_position=-1.0)), ("sigmaPosition", dict(sigma_position=float("inf"))),
    ("sigmaPlane", dict(sigma_plane=0.0)), ("sigmaPlane", dict(sigma_plane=float("-inf"))),
]


@pytest.mark.parametrize("word,kw", REFUSED_PARAMS)
def test_twin_refuses_parameters_out_of_range(word, kw):
    texels, recv, irr = _small()
    with pytest.raises(plugin.PluginError, match=word):
        plugin.denoise_lightmap(texels, recv, irr, 7, 5, cases.SAMPLES, params=kw)


def test_twin_accepts_the_ends_of_the_ranges():
    texels, recv, irr = _small()
    for kw in (dict(samples=2), dict(samples=1 << 24), dict(iterations=0), dict(iterations=8), dict(normal_power=0), dict(normal_power=7)):
        assert plugin.denoise_lightmap(texels, recv, irr, 7, 5, cases.SAMPLES, params=kw).shape == (len(texels), 4)


def test_twin_refusals_of_sizes_lists_and_structs():
    texels, recv, irr = _small()
    lib = plugin.load_library()
    for w, h in ((0, 5), (8193, 5), (7, 0), (7, 8193)):
        with pytest.raises(plugin.PluginError, match="8192"):
            plugin.denoise_lightmap(texels, recv, irr, w, h, cases.SAMPLES)
    with pytest.raises(plugin.PluginError, match="more entries than texels"):
        plugin.denoise_lightmap(texels, recv, irr, 2, 2, cases.SAMPLES)
    t2 = texels.copy()
    t2[3] = 35
    with pytest.raises(plugin.PluginError, match="width \\* height"):
        plugin.denoise_lightmap(t2, recv, irr, 7, 5, cases.SAMPLES)
    t2[3] = t2[9]
    with pytest.raises(plugin.PluginError, match="twice"):
        plugin.denoise_lightmap(t2, recv, irr, 7, 5, cases.SAMPLES)
    out = np.full((len(texels), 4), 7.5, F)
    args = (texels.ctypes.data, recv.ctypes.data, irr.ctypes.data, len(texels), 7, 5, out.ctypes.data)
    p = abi.lightmap_denoise_params(cases.SAMPLES)
    assert lib.PTDenoiseLightmapHost(None, *args) == 0 and b"params == NULL" in lib.PTGetBVHBuildError()
    for k in range(5):
        p = abi.lightmap_denoise_params(cases.SAMPLES)
        p.reserved[k] = 1
        assert lib.PTDenoiseLightmapHost(C.byref(p), *args) == 0 and b"reserved" in lib.PTGetBVHBuildError()
    p = abi.lightmap_denoise_params(cases.SAMPLES)
    p.structSize = 44
    assert lib.PTDenoiseLightmapHost(C.byref(p), *args) == 0 and b"structSize" in lib.PTGetBVHBuildError()
    p.structSize = 48
    for missing in range(3):
        a = list(args)
        a[missing] = None
        assert lib.PTDenoiseLightmapHost(C.byref(p), *a) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTDenoiseLightmapHost(C.byref(p), *args[:6], None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert (out == 7.5).all(), "a refused call wrote"
    assert lib.PTDenoiseLightmapHost(C.byref(p), *args) == 1 and lib.PTGetBVHBuildError() == b""
    # a later header's larger struct is read as far as this one knows it
    big = (C.c_uint32 * 16)()
    C.memmove(big, C.byref(p), 48)
    big[0] = 64
    out2 = np.empty_like(out)
    assert lib.PTDenoiseLightmapHost(C.cast(big, C.POINTER(abi.PTLightmapDenoiseParams)), *args[:6], out2.ctypes.data) == 1
    assert (_bits(out2) == _bits(out)).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the host twin against numpy
# ---------------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    diff = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
    assert len(diff) == 0, (what, len(diff), len(got), got[diff[:3]], want[diff[:3]])


def test_empty_list():
    for it in cases.ITERATIONS:
        out = plugin.denoise_lightmap(np.zeros(0, np.uint32), np.zeros((0, 8), F), np.zeros((0, 4), F), 7, 5, cases.SAMPLES, iterations=it)
        assert out.shape == (0, 4)
    lib = plugin.load_library()
    p = abi.lightmap_denoise_params(cases.SAMPLES)
    assert lib.PTDenoiseLightmapHost(C.byref(p), None, None, None, 0, 7, 5, None) == 1


@pytest.mark.parametrize("size", cases.SIZES)
@pytest.mark.parametrize("cover", [1.0, 0.6])
def test_twin_equals_numpy(size, cover):
    w, h = size
    texels, recv, irr, made = cases.generated_list(w, h, seed=w * 100 + h, cover=cover)
    if w * h >= 49:
        assert made["lone"] is not None
    if len(texels) >= 12:
        assert sorted(made["bad"]) == sorted(cases.BAD_KINDS)
    for it in cases.ITERATIONS:
        want, info = ref.denoise(texels, recv, irr, w, h, cases.SAMPLES, iterations=it, details=True)
        # what the case is for, on the reference
        flags = info["flags"].reshape(-1)
        assert (flags[texels[list(made["bad"].values())]] == ref.BAD).all() and (flags == ref.BAD).sum() == len(made["bad"])
        if made["lone"] is not None:
            assert flags[made["lone"]] == ref.GOOD and not info["active"].reshape(-1)[made["lone"]]
            k = int(np.nonzero(texels == made["lone"])[0][0])
            assert (_bits(want[k, :3]) == _bits(irr[k, :3])).all(), "an isolated texel keeps its e bit for bit"
        for k in made["bad"].values():
            assert (_bits(want[k]) == _bits(irr[k])).all(), "a bad entry keeps its 16 bytes"
        if it == 0:
            good = ~np.isin(np.arange(len(texels)), list(made["bad"].values()))
            assert (_bits(want[good, :3]) == _bits(irr[good, :3])).all()
            assert (_bits(want[good, 3]) == _bits(ref.entry_variance(irr[good, :3], irr[good, 3], cases.SAMPLES))).all()
        elif w * h > 1 and cover == 1.0:
            assert (_bits(want[:, :3]) != _bits(irr[:, :3])).any(axis=1).mean() > 0.5, "the filter did nothing"
        _same(plugin.denoise_lightmap(texels, recv, irr, w, h, cases.SAMPLES, iterations=it), want, (size, cover, it))


@pytest.mark.parametrize("noise_seed", [None, 11])
def test_atlas64_twin_equals_numpy(noise_seed):
    texels, recv, irr, _, _ = cases.atlas64_list(noise_seed)
    for it in cases.ITERATIONS:
        want = ref.denoise(texels, recv, irr, 64, 64, cases.SAMPLES, iterations=it)
        _same(plugin.denoise_lightmap(texels, recv, irr, 64, 64, cases.SAMPLES, iterations=it), want, it)


@pytest.mark.parametrize("normal_power", [0, 7])
def test_normal_power_ends(normal_power):
    texels, recv, irr, _ = cases.generated_list(33, 20, seed=5, cover=0.9)
    kw = dict(normal_power=normal_power, sigma_luminance=2.0, sigma_position=3.0, sigma_plane=0.5)
    want = ref.denoise(texels, recv, irr, 33, 20, cases.SAMPLES, iterations=3, **kw)
    other = ref.denoise(texels, recv, irr, 33, 20, cases.SAMPLES, iterations=3, **dict(kw, normal_power=5))
    assert (_bits(want) != _bits(other)).any(), "the normal power changes nothing"
    _same(plugin.denoise_lightmap(texels, recv, irr, 33, 20, cases.SAMPLES, params=dict(kw, iterations=3)), want, normal_power)


def test_list_order_does_not_matter():
    texels, recv, irr, _ = cases.generated_list(33, 20, seed=8, cover=0.8)
    a = plugin.denoise_lightmap(texels, recv, irr, 33, 20, cases.SAMPLES)
    b = plugin.denoise_lightmap(texels[::-1], recv[::-1], irr[::-1], 33, 20, cases.SAMPLES)
    assert (_bits(a) == _bits(b[::-1])).all()
    perm = np.random.RandomState(4).permutation(len(texels))
    c = plugin.denoise_lightmap(texels[perm], recv[perm], irr[perm], 33, 20, cases.SAMPLES)
    assert (_bits(a[perm]) == _bits(c)).all()
    _same(b, ref.denoise(texels[::-1], recv[::-1], irr[::-1], 33, 20, cases.SAMPLES), "descending")


# ---------------------------------------------------------------------------------------------------------------------------
# what the filter is for
# ---------------------------------------------------------------------------------------------------------------------------
OFF = 1e30          # a sigma that switches its weight off


def _rel_change(out, irr, sel):
    return float((np.abs(out[sel, :3].astype(np.float64) - irr[sel, :3]) / irr[sel, :3]).max())


def test_no_light_crosses_a_seam_or_a_fold():
    """Noise-free input, constant v, the luminance weight off: every texel of the dark floor, the bright wall and the coplanar
    patch sees only taps of its own value -- the cut keeps the other charts out, the normal weight the other side of the fold --
    and must keep it to EQUAL_TOL.  The two sides of a leak differ by factors of 10 to 80."""
    texels, recv, irr, truth, chart = cases.atlas64_list()
    assert (truth[chart == cases.WALL] / truth[chart == cases.DARK][0] == 80).all() and truth[chart == cases.PATCH][0] / truth[chart == cases.FLOOR].max() >= 10
    const = np.isin(chart, (cases.PATCH, cases.DARK, cases.WALL))
    for it in (1, 3, 5, 8):
        for kw in (dict(), dict(normal_power=0)):
            out = plugin.denoise_lightmap(texels, recv, irr, 64, 64, cases.SAMPLES, params=dict(kw, iterations=it, sigma_luminance=OFF))
            for c in (cases.PATCH, cases.DARK, cases.WALL):
                change = _rel_change(out, irr, chart == c)
                print(f"[lmfilter] {it} levels {kw}: chart {c} changes by {change:.3e} (bound {EQUAL_TOL:.3e})")
                assert change <= EQUAL_TOL, (it, kw, c)
            assert _rel_change(out, irr, chart == cases.FLOOR) > 0.01, "the floor's gradient and edge were not filtered at all"
    # the cut is what holds the patch: without it the coplanar floor, a tenth as bright, comes in
    out = plugin.denoise_lightmap(texels, recv, irr, 64, 64, cases.SAMPLES, params=dict(iterations=5, sigma_luminance=OFF, sigma_position=OFF))
    assert _rel_change(out, irr, chart == cases.PATCH) > 0.2
    assert _rel_change(out, irr, chart == cases.WALL) <= EQUAL_TOL, "the fold is held by the normals, not by the cut"
    assert const.sum() == 4 * 8 + 2 * 30 * 32


def test_a_constant_image_is_a_fixed_point():
    """whatever the guides are: a weighted mean of equal values is that value to EQUAL_TOL"""
    for (w, h), seed in (((33, 20), 3), ((130, 67), 4)):
        texels, recv, _, _ = cases.generated_list(w, h, seed=seed, cover=0.8, bad=False)
        irr = cases.exact_rows(np.full(len(texels), 0.7))
        for it in (1, 5, 8):
            out = plugin.denoise_lightmap(texels, recv, irr, w, h, cases.SAMPLES, iterations=it)
            assert _rel_change(out, irr, slice(None)) <= EQUAL_TOL, (w, h, it)


def test_noise_falls_with_every_level():
    """16 Gaussian samples per texel: the mean squared error against the true E over the covered texels falls with every one of
    levels 1 to 5, the returned variance with it, and at level 5 the error is below a quarter of the unfiltered one"""
    texels, recv, irr, truth, _ = cases.atlas64_list(noise_seed=11)
    want = truth[:, None].astype(np.float64) * cases.TINT[None, :]
    mse, var = [], []
    for it in range(6):
        out = plugin.denoise_lightmap(texels, recv, irr, 64, 64, cases.SAMPLES, iterations=it)
        mse.append(float(((out[:, :3] - want) ** 2).mean()))
        var.append(float(out[:, 3].astype(np.float64).mean()))
    print("[lmfilter] mse by level:", " ".join(f"{m:.4g}" for m in mse))
    print("[lmfilter] mean v by level:", " ".join(f"{v:.4g}" for v in var))
    for it in range(1, 6):
        assert mse[it] < mse[it - 1], (it, mse)
        assert var[it] < var[it - 1], (it, var)
    assert mse[5] < 0.25 * mse[0], mse


# ---------------------------------------------------------------------------------------------------------------------------
# the sanitizers and the kernels' resources
# ---------------------------------------------------------------------------------------------------------------------------
def test_host_twin_under_sanitizers(tmp_path):
    """`make lmfilter-sanitize`: lmfilter_host.cpp and csrc/lmfilter_sanitize_main.cpp (its own main) with -fsanitize=address,undefined,
    built and run, nothing preloaded: it filters in place and out of place at every number of levels and makes the refusals, and
    must finish without a report."""
    csrc = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "lmfilter-sanitize", "LMFILTER_SANITIZE_OUT=" + str(tmp_path / "lmfilter_sanitize")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "lmfilter ok" in out.stdout, out.stdout + out.stderr


KERNELS = ["pt_lmf_scatter", "pt_lmf_footprint", "pt_lmf_atrous", "pt_lmf_collect"]
STAGED = {1: 19200, 2: 27648, 4: 49152}         # pt_lmf_atrous_lds<S>: (16 + 4 S)^2 texels of 48 bytes
SHADE_VGPRS = 128           # what tests/test_kernel_resources.py holds pt_wf_shade<false, PTRayMap> to


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_lmfilter_kernels_fit_the_shade_kernels_budget():
    res = resources("pt_lmfilter.hip")
    assert len(res) == len(KERNELS) + len(STAGED) and all("pt_lmf_" in k for k in res), sorted(res)
    for name in KERNELS:
        assert len([k for k in res if f"{len(name)}{name}E" in k]) == 1, (name, sorted(res))
    for step, lds in STAGED.items():
        staged = [r for k, r in res.items() if f"pt_lmf_atrous_ldsILi{step}EE" in k]
        assert len(staged) == 1 and staged[0]["lds"] == lds, (step, sorted(res))
    for k, r in res.items():
        print(f"[resources] {k}: {r}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
        assert r["vgprs"] <= SHADE_VGPRS, (k, r)
    for other in ("pt_lightmap.hip", "pt_gather.hip"):
        assert not [k for k in resources(other) if "pt_lmf_" in k], other
