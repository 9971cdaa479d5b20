"""Ray queries (include/ptmi_plugin.h Part 3) without a GPU: exports, struct layouts, argument checks, kernel resources."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

from kernel_resources import resources
from unity_webgpu_pathtracer_amd import abi, plugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
QUERY_SYMBOLS = ["PTTraceRays", "PTTraceRaysHost"]


def test_query_symbols_are_exported():
    plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in QUERY_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name


def test_query_structs_match_c_header():
    fields = {"PTRay": ["origin", "direction", "tmax", "reserved"],
              "PTRayHit": ["t", "u", "v", "prim"],
              "PTRaySurface": ["position", "t", "normal", "materialIndex", "uv", "instance", "prim"]}
    lines = []
    for s, fs in fields.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) +
           '\nprintf("flags %u %u %u\\n", PT_QUERY_CLOSEST, PT_QUERY_ANY_HIT, PT_QUERY_SURFACE);\nreturn 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert got["flags"] == f"{abi.PT_QUERY_CLOSEST} {abi.PT_QUERY_ANY_HIT} {abi.PT_QUERY_SURFACE}"
    for s, fs in fields.items():
        cls = getattr(abi, s)
        assert int(got[s]) == C.sizeof(cls), s
        for f in fs:
            assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, (s, f)
    assert (C.sizeof(abi.PTRay), C.sizeof(abi.PTRayHit), C.sizeof(abi.PTRaySurface)) == (32, 16, 48)


def test_query_argument_errors_without_context():
    lib = plugin.load_library()
    rays = (abi.PTRay * 4)()
    hits = (abi.PTRayHit * 4)()
    surf = (abi.PTRaySurface * 4)()
    for fn in (lib.PTTraceRays, lib.PTTraceRaysHost):
        assert fn(None, C.addressof(rays), 4, abi.PT_QUERY_CLOSEST, C.addressof(hits), None) == abi.PT_ERR_INVALID_ARG
        assert b"ctx == NULL" in lib.PTGetLastError()
        for flags in (4, 0x80000000, abi.PT_QUERY_ANY_HIT | abi.PT_QUERY_SURFACE):
            assert fn(None, C.addressof(rays), 4, flags, C.addressof(hits), C.addressof(surf)) == abi.PT_ERR_INVALID_ARG
            msg = lib.PTGetLastError()
            assert b"flag" in msg or b"SURFACE" in msg, msg


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
@pytest.mark.parametrize("defines", [(), ("-DPT_Q_LDS_STACK=1",)], ids=["default", "stress"])
def test_query_kernels_have_no_scratch(defines):
    """The CWBVH query kernels keep their whole stack in LDS + the HBM slab: no scratch, no spill, 8 waves per SIMD
    (DESIGN.md "Ray queries").  The HAS_TLAS ones keep the render's TLAS code and at least 4 waves per SIMD."""
    res = resources("pt_query.hip", defines=defines)
    names = ["pt_query_" + m + s for m in ("closest", "anyhit", "surface") for s in ("", "_stats")]
    for n in names:
        assert n in res, (n, sorted(res))
        r = res[n]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (n, r)
        assert r["occupancy"] >= 8, (n, r)
        assert r["lds"] <= 5120, (n, r)                   # 32 one-wave workgroups per CU fit in 160 KB
    for n in ["pt_query_tlas_" + m[len("pt_query_"):] for m in names]:
        assert n in res, (n, sorted(res))
        assert res[n]["vgpr_spill"] == 0 and res[n]["occupancy"] >= 4, (n, res[n])
