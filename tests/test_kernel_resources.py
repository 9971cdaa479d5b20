"""The register / scratch budget the measured performance rests on, checked at compile time.

hipcc cross-compiles gfx950 without a GPU and reports every kernel's resources with -Rpass-analysis=kernel-resource-usage.
ANY scratch in the refill trace kernel costs it its occupancy (+8 % when it was removed), and the shade kernel's fourth wave
per SIMD (<= 128 VGPRs) is worth 10 %: a change that silently crosses one of these lines should fail here, not in a benchmark."""
import shutil

import pytest

from kernel_resources import resources


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_trace_and_shade_kernels_keep_their_register_budget():
    res = resources("pt_wavefront.hip", unit="a")               # refill trace + shade of the default schedule
    res_b = resources("pt_wavefront.hip", unit="b")             # HAS_TLAS (and schedules 0, 2, 3, 4)

    def pick(*parts, res=res):
        hits = [v for k, v in res.items() if all(p in k for p in parts)]
        assert hits, (parts, sorted(res))
        return hits

    # refill trace kernel, no-statistics instantiations (the ones a render uses): main and tail launch, 64- and 128-slot ranges
    for r in pick("pt_wf_trace_refillILb0E"):
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["occupancy"] == 8 and r["vgprs"] <= 64, r
        assert r["lds"] <= 5120, r                      # 32 one-wave workgroups per CU in 160 KB
    # ... and the statistics instantiations of its main launch (fullStats renders): no scratch either.  (Those of the TAIL launch,
    # ILb1ELb1E, have had 36 bytes since before this line was drawn; they are not held to it.)
    for r in pick("pt_wf_trace_refillILb1ELb0E"):
        assert r["scratch"] == 0, r
    # shade kernel: four waves per SIMD, no scratch
    for r in pick("pt_wf_shadeILb0E"):
        assert r["scratch"] == 0 and r["vgprs"] <= 128 and r["occupancy"] >= 4, r
    # HAS_TLAS refill kernel: six waves per SIMD, no scratch
    for r in pick("pt_wf_trace_refill_tlasILb0E", res=res_b):
        assert r["scratch"] == 0 and r["vgprs"] <= 80 and r["occupancy"] >= 6, r
        assert r["lds"] * 24 <= 160 * 1024, r
