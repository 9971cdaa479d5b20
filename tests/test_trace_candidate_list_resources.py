"""The candidate list of the main refill trace launch against its budgets, at compile time.

The list adds 512 bytes of LDS to a one-wave workgroup, and 32 such workgroups must still fit the CU's 160 KB (5,120 bytes
each); the kernel must stay at 8 waves per SIMD (<= 64 VGPRs, no scratch).  The change touched nothing else in unit a: the TAIL
instantiations and every pt_wf_shade are, instruction for instruction, what the commit before it compiled to --
tests/golden/wavefront_unit_a_streams.txt holds the instruction count and the SHA-256 of each of those streams (labels
renumbered, comments dropped; tests/kernel_streams.py), taken from that commit with the same compiler.  The pt_wf_shade streams
were taken again when pt_exp2's scale was clamped at the top (include/ptmi_math.h; pow is in the shade step): 10 instructions more
in each of the six, the tail streams untouched."""
import os
import shutil

import pytest

from kernel_resources import resources
from kernel_streams import fingerprint, streams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavefront_unit_a_streams.txt")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")


def test_main_refill_kernels_keep_lds_registers_and_scratch():
    res = resources("pt_wavefront.hip", unit="a")
    main = {k: v for k, v in res.items() if "pt_wf_trace_refillILb" in k and "ELb0ELj" in k}      # <*, false, *>
    assert len(main) == 4, sorted(res)                              # STATS on / off x RANGE 64 / 128
    for k, r in main.items():
        assert r["lds"] <= 5120, (k, r)
        assert r["vgprs"] <= 64 and r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)


def test_tail_and_shade_kernels_are_the_parents_instruction_for_instruction():
    got = streams("pt_wavefront.hip", unit="a")
    want = [l.split() for l in open(GOLDEN).read().splitlines() if l and not l.startswith("#")]
    names = {n for n in got if ("pt_wf_trace_refillILb" in n and "ELb1ELj" in n) or "pt_wf_shadeILb" in n}
    assert names == {n for n, _, _ in want} and len(names) == 10, sorted(names)     # 4 tail + 6 shade instantiations
    for n, count, digest in want:
        assert fingerprint(got[n]) == (int(count), digest), (n, fingerprint(got[n])[0], int(count))
