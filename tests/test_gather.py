"""Irradiance gathers (include/ptmi_plugin.h Part 13) without a GPU: exports, struct layout, argument checks and the compile-time
resources of the gather kernels.  tests/test_gpu_gather.py holds the kernels to the rule."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from kernel_resources import resources
import gather_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER_SYMBOLS = ["PTGatherIrradiance", "PTGatherIrradianceHost", "PTGatherRays"]


def test_gather_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in GATHER_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 13: irradiance gathers" in header


def test_gather_structs_match_c_header():
    fields = {"PTReceiver": ["position", "seed", "normal", "reserved"], "PTIrradiance": ["rgb", "m2"]}
    lines = []
    for s, fs in fields.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTReceiver"]) == C.sizeof(abi.PTReceiver) == 32
    assert int(got["PTIrradiance"]) == C.sizeof(abi.PTIrradiance) == 16
    for s, fs in fields.items():
        for f in fs:
            assert int(got[f"{s}.{f}"]) == getattr(getattr(abi, s), f).offset, (s, f)
    assert [int(got[f"PTReceiver.{f}"]) for f in fields["PTReceiver"]] == [0, 12, 16, 28]
    assert [int(got[f"PTIrradiance.{f}"]) for f in fields["PTIrradiance"]] == [0, 12]


def test_gather_argument_errors_without_context():
    lib = plugin.load_library()
    p = abi.PTFrameParams()
    p.OutputWidth, p.OutputHeight = 4, 4
    buf = (C.c_float * 256)()
    for fn in (lib.PTGatherIrradiance, lib.PTGatherIrradianceHost, lib.PTGatherRays):
        rc = fn(None, C.byref(p), C.addressof(buf), 4, 0, 2, C.addressof(buf))
        assert rc == abi.PT_ERR_INVALID_ARG
        assert b"ctx" in lib.PTGetLastError() and b"NULL" in lib.PTGetLastError()


def test_seed_rule_restatement(oracle):
    """gather_ref's PCG step is the oracle's: the state one draw leaves"""
    lib = oracle.load_oracle()
    for seed in (0, 1, 0xFFFFFFFF, 0x5AD1A, 0x80000000):
        s = C.c_uint32(seed)
        lib.oracle_random_float(C.byref(s))
        assert gather_ref.rng_next(seed) == s.value, seed
    # s += firstSample + j wraps, and samples [a, a + n) do not depend on how the range is split
    assert gather_ref.sample_seed(7, 0xFFFFFFFF, 1) == gather_ref.rng_next(7)
    assert gather_ref.sample_seed(7, 3, 2) == gather_ref.sample_seed(7, 5, 0) == gather_ref.sample_seed(7, 0, 5)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel resources: the gather kernels fit the budget of the shade kernel they hand their slots to, and the
# kernels between them are the ray map's -- no instantiation of a shade, trace or cleanup kernel exists for the gather
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_gather_kernels_fit_the_shade_kernels_budget():
    with ThreadPoolExecutor(3) as ex:
        fa = ex.submit(resources, "pt_wavefront.hip", "a")
        fb = ex.submit(resources, "pt_wavefront.hip", "b")
        fg = ex.submit(resources, "pt_gather.hip")
        res_a, res_b, res_g = fa.result(), fb.result(), fg.result()
    gather = {k: v for k, v in res_g.items() if "pt_wf_gather" in k}
    assert len([k for k in gather if "pt_wf_gather_init" in k]) == 2, sorted(res_g)          # with and without statistics
    assert len([k for k in gather if "pt_wf_gather_resolve" in k]) == 1 and len([k for k in gather if "pt_wf_gather_rays" in k]) == 1, sorted(res_g)
    assert len(gather) == 4, sorted(res_g)
    for unit, res in (("a", res_a), ("b", res_b)):
        shade = [v for k, v in res.items() if "pt_wf_shadeILb0E" in k and "PTRayMap" in k]
        assert len(shade) == 1, sorted(res)
        for k, r in gather.items():
            print(f"[resources] {k}: {r}  (unit {unit} shade: {shade[0]})")
            assert r["scratch"] == 0 and r["scratch"] <= shade[0]["scratch"], (k, r)
            assert r["vgprs"] <= shade[0]["vgprs"], (k, r, shade[0])
        middle = [k for k in res if "pt_wf_shade" in k or "pt_wf_trace" in k or "pt_wf_cleanup" in k]
        assert middle and not [k for k in middle if "gather" in k.lower()], middle
        assert not [k for k in res if "gather" in k.lower()], sorted(res)                    # the gather's kernels live in pt_gather.hip
    assert not [k for k in res_g if "pt_wf_shade" in k or "pt_wf_trace" in k or "pt_wf_cleanup" in k], sorted(res_g)
