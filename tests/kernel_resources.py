"""What hipcc reports about every kernel of a source file, compiled with the flags the product is built with.

hipcc cross-compiles gfx950 without a GPU and reports every kernel's resources with -Rpass-analysis=kernel-resource-usage.  The
resource tests (test_kernel_resources.py and the per-feature ones) import this module the way the stack tests import
stack_cases.py; a report is computed once per process and (source, unit, defines)."""
import os
import re
import subprocess
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")

_lock = threading.Lock()
_reports = {}           # (src, unit, defines) -> [lock, report or None]


def device_flags(unit=None):
    """FLAGS / HIPFLAGS of csrc/Makefile (minus -Wall).  pt_wavefront.hip is compiled twice: unit "a" adds what HIPFLAGS_A adds
    (the plain refill trace and its shade kernels come from there), unit "b" adds -DPT_WF_TU_B (everything else)."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    hip = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1)
    extra = hip.replace("$(FLAGS)", "").replace("--offload-arch=$(ARCH)", "").split()
    assert unit in (None, "a", "b"), unit
    if unit == "a":
        extra += re.search(r"^HIPFLAGS_A\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(HIPFLAGS)", "").split()
    elif unit == "b":
        extra += ["-DPT_WF_TU_B"]
    return [f for f in flags if f != "-Wall"] + extra


def parse_report(stderr):
    """kernel name -> {vgprs, scratch, occupancy, vgpr_spill, sgpr_spill, lds} from the compiler's remarks"""
    res, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        for key, name in (("VGPRs:", "vgprs"), ("ScratchSize", "scratch"), ("Occupancy", "occupancy"), ("VGPRs Spill", "vgpr_spill"), ("SGPRs Spill", "sgpr_spill"),
                          ("LDS Size", "lds")):
            m = re.search(re.escape(key) + r"[^0-9]*(\d+)", line)
            if m and cur is not None and key in line:
                cur[name] = int(m.group(1))
    return res


def resources(src, unit=None, defines=()):
    """The report of csrc/<src>; callers treat it as read-only.  Safe to call from several threads: each report is compiled once."""
    key = (src, unit, tuple(defines))
    with _lock:
        entry = _reports.setdefault(key, [threading.Lock(), None])
    with entry[0]:
        if entry[1] is None:
            out = subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-c", src, "-o", os.devnull,
                                  "-Rpass-analysis=kernel-resource-usage"] + device_flags(unit) + list(defines),
                                 cwd=CSRC, capture_output=True, text=True, timeout=900)
            assert out.returncode == 0, out.stderr[-2000:]
            entry[1] = parse_report(out.stderr)
    return entry[1]
