"""The instruction stream of every kernel of a source file, as hipcc -S writes it with the flags the product is built with.

A kernel's stream is its instructions in order with comments dropped and its local labels (.LBBn_m) renumbered by first appearance,
so two compilations give the same stream exactly when the kernel is instruction for instruction the same.  fingerprint() is
what tests/golden keeps of a stream: the instruction count and a SHA-256."""
import hashlib
import os
import re
import subprocess
import tempfile

from kernel_resources import CSRC, device_flags

_cache = {}


def parse_streams(asm):
    """mangled kernel or function name -> list of normalised instruction lines"""
    out, cur, labels = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur, labels = out.setdefault(m.group(1), []), {}
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        text = line.split(";", 1)[0].strip()
        if not text or (text.startswith(".") and not text.startswith(".LBB")):
            continue                                              # directives and the assembler's other local labels
        text = re.sub(r"\.LBB\d+_\d+", lambda m: "L%d" % labels.setdefault(m.group(0), len(labels)), text)
        cur.append(re.sub(r"\s+", " ", text))
    return {k: v for k, v in out.items() if v}


def streams(src, unit=None, defines=(), csrc=CSRC):
    key = (src, unit, tuple(defines), csrc)
    if key not in _cache:
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(tmp, "out.s")
            r = subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", s] + device_flags(unit) + list(defines),
                               cwd=csrc, capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            _cache[key] = parse_streams(open(s).read())
    return _cache[key]


def fingerprint(stream):
    return sum(not l.endswith(":") for l in stream), hashlib.sha256("\n".join(stream).encode()).hexdigest()
