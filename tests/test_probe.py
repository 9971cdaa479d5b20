"""SH light probes (include/ptmi_plugin.h Part 15) without a GPU: exports, struct layout, argument checks, the host twins against
the numpy restatement of the rule (tests/probe_ref.py) bit for bit, the statistics of the sphere directions, the sanitizer build of
the host twins and the compile-time resources of the probe kernels.  tests/test_gpu_probe.py holds the kernels
to the rule."""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from kernel_resources import resources
import probe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
F = np.float32
CONTEXT_SYMBOLS = ["PTProbeSH", "PTProbeSHHost", "PTProbeRays", "PTProbeIrradiance"]
HOST_SYMBOLS = ["PTProbeDirectionsHost", "PTProbeProjectHost", "PTProbeIrradianceHost"]
# the probe whose 65,536 directions the statistics below are taken over: fixed after checking that it passes them
STAT_SEED = 0x5EED


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_probe_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in CONTEXT_SYMBOLS + HOST_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 15: SH light probes" in header


def test_probe_structs_match_c_header():
    fields = {"PTProbe": ["position", "seed"], "PTProbeCoeffs": ["sh", "m2"], "PTProbeQuery": ["normal", "probe"]}
    lines = []
    for s, fs in fields.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    lines.append('printf("flag %u\\n", PT_PROBE_DELTA_LIGHTS);')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTProbe"]) == C.sizeof(abi.PTProbe) == 16
    assert int(got["PTProbeCoeffs"]) == C.sizeof(abi.PTProbeCoeffs) == 112
    assert int(got["PTProbeQuery"]) == C.sizeof(abi.PTProbeQuery) == 16
    for s, fs in fields.items():
        for f in fs:
            assert int(got[f"{s}.{f}"]) == getattr(getattr(abi, s), f).offset, (s, f)
    assert [int(got[f"PTProbeCoeffs.{f}"]) for f in fields["PTProbeCoeffs"]] == [0, 108]
    assert int(got["flag"]) == abi.PT_PROBE_DELTA_LIGHTS == 1


def test_probe_argument_errors_without_context():
    lib = plugin.load_library()
    p = abi.PTFrameParams()
    p.OutputWidth, p.OutputHeight = 4, 4
    buf = (C.c_float * 256)()
    a = C.addressof(buf)
    calls = {"PTProbeSH": lambda: lib.PTProbeSH(None, C.byref(p), a, 4, 0, 2, 0, a),
             "PTProbeSHHost": lambda: lib.PTProbeSHHost(None, C.byref(p), a, 4, 0, 2, 0, a),
             "PTProbeRays": lambda: lib.PTProbeRays(None, C.byref(p), a, 4, 0, 2, a),
             "PTProbeIrradiance": lambda: lib.PTProbeIrradiance(None, a, 1, a, 4, a)}
    for name, call in calls.items():
        assert call() == abi.PT_ERR_INVALID_ARG, name
        assert b"ctx" in lib.PTGetLastError() and b"NULL" in lib.PTGetLastError() and name.encode() in lib.PTGetLastError()
    # the host twins: 0 and a message
    rows = plugin.probe_rows(np.zeros((2, 3), F))
    for bad in (0, 65537):
        with pytest.raises(plugin.PluginError, match="samples"):
            plugin.probe_directions(rows[:, :3], bad)
    assert lib.PTProbeDirectionsHost(None, 2, 0, 4, a) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTProbeProjectHost(None, a, 1, 4, a) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTProbeIrradianceHost(a, 1, None, 1, a) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert plugin.probe_directions(np.zeros((0, 3), F), 4).shape == (0, 8)


# ---------------------------------------------------------------------------------------------------------------------------
# the host twins hold the rule
# ---------------------------------------------------------------------------------------------------------------------------
def test_directions_follow_the_seed_rule(oracle):
    """origin, RNG state and reserved word of every entry; the direction from the oracle's own draws, in float32 steps"""
    lib = oracle.load_oracle()
    pos = np.array([(0.5, -1.25, 3.0), (7.0, 8.0, 9.0)], F)
    seeds = np.array([0xFFFFFFF0, 12345], np.uint32)
    samples, first = 5, 0xFFFFFFFE
    rays = plugin.probe_directions(pos, samples, first_sample=first, seeds=seeds)
    assert rays.shape == (2 * samples, 8) and (_bits(rays[:, 7]) == 0).all()
    for i in range(2):
        for j in range(samples):
            s = C.c_uint32(probe_ref.sample_seed(int(seeds[i]), first, j))
            r1 = F(lib.oracle_random_float(C.byref(s)))
            r2 = F(lib.oracle_random_float(C.byref(s)))
            row = rays[i * samples + j]
            assert int(_bits(row[6:7])[0]) == s.value, (i, j)
            assert (row[0:3] == pos[i]).all()
            z = F(F(1.0) - F(F(2.0) * r1))
            assert _bits(row[5:6])[0] == _bits(z)[0], (i, j)
            rho = np.sqrt(max(F(F(1.0) - F(z * z)), F(0.0)), dtype=F)
            phi = float(F(F(6.28318530717958648) * r2))
            # pt_sin / pt_cos are polynomials of the project's own: they agree with libm to a few ulp of 1
            assert abs(float(row[3]) - float(rho) * math.cos(phi)) < 2e-6 and abs(float(row[4]) - float(rho) * math.sin(phi)) < 2e-6
    # samples [a, a + n) are the same however the range is split
    tail = plugin.probe_directions(pos, 2, first_sample=(first + 3) & 0xFFFFFFFF, seeds=seeds)
    assert (_bits(tail.reshape(2, 2, 8)) == _bits(rays.reshape(2, samples, 8)[:, 3:5])).all()


def test_directions_are_uniform_on_the_sphere():
    n = 65536
    rays = plugin.probe_directions(np.zeros((1, 3), F), n, seeds=[STAT_SEED])
    w = rays[:, 3:6].astype(np.float64)
    assert np.abs(1.0 - np.linalg.norm(w, axis=1)).max() < 4e-7
    Y = probe_ref.basis(rays[:, 3:6]).astype(np.float64)
    for k in range(1, 9):
        mean, bound = Y[:, k].mean(), 5.0 * math.sqrt(1.0 / (4.0 * math.pi * n))
        sq = 4.0 * math.pi * Y[:, k] ** 2
        err, tol = abs(sq.mean() - 1.0), 5.0 * math.sqrt(sq.var(ddof=1) / n)
        print(f"[probe] Y{k}: |mean| = {abs(mean):.2e} (bound {bound:.2e})  |4 PI mean(Y^2) - 1| = {err:.2e} (bound {tol:.2e})")
        assert abs(mean) < bound, k
        assert err < tol, k


@pytest.mark.parametrize("samples", [1, 63, 64, 70, 4096])
def test_project_host_equals_the_restated_rule(samples):
    n = 3
    rng = np.random.default_rng(samples)
    d = plugin.probe_directions(rng.uniform(-1, 1, (n, 3)).astype(F), samples, seeds=[5, 6, 7])[:, 3:6].reshape(n, samples, 3)
    c = (rng.uniform(0, 4, (n, samples, 3)) * (rng.uniform(0, 1, (n, samples, 1)) < 0.7)).astype(F)
    sh, m2 = plugin.probe_project(d, c)
    want_sh, want_m2 = probe_ref.project(d, c)
    assert sh.shape == (n, 9, 3) and m2.shape == (n,)
    assert (_bits(sh) == _bits(want_sh)).all(), np.argwhere(_bits(sh) != _bits(want_sh))[:5]
    assert (_bits(m2) == _bits(want_m2)).all()
    assert np.abs(sh).max() > 0                          # (about a third of the samples are black: zeros are added too)


@pytest.mark.parametrize("samples", [64, 70, 4096, 65536])
def test_constant_radiance_projects_to_band_zero(samples):
    d = plugin.probe_directions(np.zeros((1, 3), F), samples, seeds=[STAT_SEED])[:, 3:6].reshape(1, samples, 3)
    sh, m2 = plugin.probe_project(d, np.ones((1, samples, 3), F))
    want = 2.0 * math.sqrt(math.pi)
    rel = np.abs(sh[0, 0].astype(np.float64) - want).max() / want
    bound = (samples / 64 + 6) * 2.0 ** -24           # each lane adds samples / 64 terms, the tree six more: the summation bound
    print(f"[probe] {samples} samples of radiance 1: sh[0] = {sh[0, 0, 0]!r}, relative error {rel:.2e} (bound {bound:.2e})")
    assert rel <= bound
    assert np.abs(sh[0, 1:].astype(np.float64)).max() < 5.0 * math.sqrt(4.0 * math.pi / samples)
    assert abs(float(m2[0]) - samples) <= samples * 1e-5


def test_irradiance_host_equals_the_restated_rule():
    rng = np.random.default_rng(11)
    n, q = 5, 64
    sh = rng.normal(0, 1, (n, 9, 3)).astype(F)
    nrm = rng.normal(0, 1, (q, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    idx = rng.integers(0, n, q).astype(np.uint32)
    idx[7], idx[8] = n, 0xFFFFFFFF                      # out of range: zeros
    out = plugin.probe_irradiance(sh, nrm, idx)
    assert out.shape == (q, 4) and (out[:, 3] == 0).all()
    for k in range(q):
        want = probe_ref.irradiance(sh[idx[k]], nrm[k]) if idx[k] < n else np.zeros(3, F)
        assert (_bits(out[k, :3]) == _bits(want)).all(), k
    # constant radiance L: only sh[0] = 2 sqrt(PI) L is set, and E = PI L whatever the normal
    L = np.array([0.25, 1.0, 3.0])
    flat = np.zeros((1, 9, 3), F)
    flat[0, 0] = (2.0 * math.sqrt(math.pi) * L).astype(F)
    E = plugin.probe_irradiance(flat, nrm, np.zeros(q, np.uint32))[:, :3].astype(np.float64)
    assert (np.abs(E - math.pi * L) <= 1e-6 * math.pi * L).all(), np.abs(E / (math.pi * L) - 1).max()


def test_probe_sanitize_target_runs_clean():
    """the three host twins under AddressSanitizer + UBSan in a stand-alone program (csrc/probe_sanitize_main.cpp)"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", CSRC, "probe-sanitize", "PROBE_SANITIZE_OUT=" + os.path.join(d, "probe_sanitize")],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "probe ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


# ---------------------------------------------------------------------------------------------------------------------------
# kernel resources: the probe kernels fit the budget of the shade kernel they hand their slots to, and the
# kernels between them are the ray map's -- pt_wavefront.hip's two compilations hold the kernels they held before
# ---------------------------------------------------------------------------------------------------------------------------
KERNELS = ["pt_wf_probe_init", "pt_wf_probe_rays", "pt_wf_probe_resolve", "pt_probe_delta_rays", "pt_probe_irradiance"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_probe_kernels_fit_the_shade_kernels_budget():
    with ThreadPoolExecutor(3) as ex:
        fa = ex.submit(resources, "pt_wavefront.hip", "a")
        fb = ex.submit(resources, "pt_wavefront.hip", "b")
        fp = ex.submit(resources, "pt_probe.hip")
        res_a, res_b, res_p = fa.result(), fb.result(), fp.result()
    assert len(res_p) == len(KERNELS), sorted(res_p)
    for name in KERNELS:
        assert len([k for k in res_p if f"{len(name)}{name}E" in k]) == 1, (name, sorted(res_p))
    golden = open(os.path.join(ROOT, "tests", "golden", "wavefront_kernel_names.txt")).read().split()
    for unit, res in (("a", res_a), ("b", res_b)):
        shade = [v for k, v in res.items() if "pt_wf_shadeILb0E" in k and "PTRayMap" in k]
        assert len(shade) == 1, sorted(res)
        for k, r in res_p.items():
            print(f"[resources] {k}: {r}  (unit {unit} shade: {shade[0]})")
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
            assert r["vgprs"] <= shade[0]["vgprs"], (k, r, shade[0])
        assert not [k for k in res if "probe" in k.lower()], sorted(res)                     # the probe's kernels live in pt_probe.hip
        # the kernels of this compilation, by name, are the ones it held before probes existed
        assert sorted(res) == sorted(n[2:] for n in golden if n.startswith(unit + ":")), unit
    assert not [k for k in res_p if "pt_wf_shade" in k or "pt_wf_trace" in k or "pt_wf_cleanup" in k], sorted(res_p)
