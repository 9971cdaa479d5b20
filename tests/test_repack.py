"""The mid-pass slot repack of the default schedule without a GPU (csrc/repack_rule.h, repack_host.cpp):
the rule on the host against a plain loop, the stand-alone sanitizer program, and the register line of the shade kernels that
run in a repacked sequence."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from kernel_resources import resources
from unity_webgpu_pathtracer_amd import plugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256
DONE = 2


def plan(flags, capacity, num, den):
    """PTRepackPlanHost -> (go, L, E, dest)"""
    f = np.ascontiguousarray(flags, dtype=np.uint32)
    out, dest = np.zeros(3, np.uint32), np.zeros(len(f), np.uint32)
    ok = plugin.load_library().PTRepackPlanHost(f.ctypes.data, len(f), capacity, num, den, out.ctypes.data, dest.ctypes.data)
    assert ok == 1
    return bool(out[0]), int(out[1]), int(out[2]), dest


def reference(flags, capacity, num, den):
    """the rule as one loop over the slots: the k-th live slot goes to slot k"""
    dest = np.full(len(flags), 0xFFFFFFFF, np.uint32)
    live, last = 0, -1
    for s, f in enumerate(flags):
        if (int(f) & 3) != DONE:
            dest[s] = live
            live, last = live + 1, s
    extent = (last // BLOCK + 1) * BLOCK if live else 0
    go = 0 < live <= capacity and live * den <= extent * num
    return go, live, extent, dest


def check(flags, capacity, num, den, expect_go=None):
    got, want = plan(flags, capacity, num, den), reference(flags, capacity, num, den)
    assert got[:3] == want[:3], (got[:3], want[:3])
    assert np.array_equal(got[3], want[3])
    if expect_go is not None:
        assert got[0] == expect_go, got[:3]


def test_host_twin_against_a_plain_loop():
    rng = np.random.default_rng(7)
    for _ in range(60):
        n = int(rng.integers(1, 24)) * BLOCK
        density = rng.random()
        state = np.where(rng.random(n) < density, rng.integers(0, 2, n), DONE).astype(np.uint32)
        flags = state | (rng.integers(0, 1 << 30, n).astype(np.uint32) << 2)          # the other bits of a flags word do not matter
        for num, den in ((3, 4), (1, 1)):
            check(flags, n // 2, num, den)
    n, cap = 8 * BLOCK, 4 * BLOCK
    check(np.full(n, DONE, np.uint32), cap, 1, 1, expect_go=False)                     # no live slot
    check(np.zeros(n, np.uint32), cap, 1, 1, expect_go=False)                          # all live: more than the capacity
    check(np.zeros(n, np.uint32), n, 1, 1, expect_go=True)                             # ... with room for all of them, no threshold
    check(np.zeros(n, np.uint32), n, 3, 4, expect_go=False)                            # ... and dense already at 3/4
    f = np.full(n, DONE, np.uint32)
    f[1::2] = 1
    check(f, cap, 1, 1, expect_go=True)                                                # L == capacity
    f[0] = 0
    check(f, cap, 1, 1, expect_go=False)                                               # L == capacity + 1: refused
    f = np.full(n, DONE, np.uint32)
    f[[n - BLOCK, n - 7, n - 1]] = 0
    check(f, cap, 3, 4, expect_go=True)                                                # live slots only in the last block
    f = np.full(BLOCK, DONE, np.uint32)
    f[[5, 200]] = 1
    check(f, BLOCK // 2, 3, 4, expect_go=True)                                         # an extent of one block
    # what the twin refuses
    lib = plugin.load_library()
    out = np.zeros(3, np.uint32)
    f = np.zeros(BLOCK + 1, np.uint32)
    assert lib.PTRepackPlanHost(f.ctypes.data, BLOCK + 1, BLOCK, 3, 4, out.ctypes.data, None) == 0
    assert lib.PTRepackPlanHost(f.ctypes.data, BLOCK, BLOCK, 3, 0, out.ctypes.data, None) == 0
    assert lib.PTRepackPlanHost(None, BLOCK, BLOCK, 3, 4, out.ctypes.data, None) == 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_repack_kernels_keep_the_shade_budget():
    """csrc/pt_repack.hip, compiled with the flags of the default schedule's unit as the Makefile does: the shade kernel of a
    repacked sequence meets the line tests/test_kernel_resources.py draws for pt_wf_shade (<= 128 VGPRs, no scratch, four waves per
    SIMD), the four repack kernels use no scratch, and the file holds nothing else but the cleanup kernels.  pt_wavefront.hip
    keeps the kernels it had (tests/golden/wavefront_kernel_names.txt, checked by the probe and reflection tests), the refill
    trace kernels among them: their line stands (58 VGPRs in the main launch of the benchmark)."""
    res = resources("pt_repack.hip", unit="a")
    shade = {k: r for k, r in res.items() if "pt_wf_shade_repackILb0E" in k}
    assert len(shade) == 1, sorted(res)
    for k, r in shade.items():
        print(f"[resources] {k}: {r}")
        assert r["scratch"] == 0 and r["vgprs"] <= 128 and r["occupancy"] >= 4, (k, r)
    stats = [r for k, r in res.items() if "pt_wf_shade_repackILb1E" in k]
    assert len(stats) == 1 and stats[0]["scratch"] == 0 and stats[0]["vgprs"] <= 128, stats
    moves = {k: r for k, r in res.items() if "pt_wf_repack_" in k}
    assert len(moves) == 4, sorted(res)
    for k, r in moves.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
    assert len([k for k in res if "pt_wf_cleanup_repack" in k]) == 4 and len(res) == 10, sorted(res)
    for k, r in resources("pt_wavefront.hip", unit="a").items():
        assert "repack" not in k, k
        if "pt_wf_trace_refillILb0E" in k:
            assert r["scratch"] == 0 and r["vgprs"] <= 64 and r["occupancy"] == 8, (k, r)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_host_twin_under_sanitizers(tmp_path):
    """`make repack-sanitize`: the host twin and csrc/repack_sanitize_main.cpp (its own main) with -fsanitize=address,undefined,
    built and run -- it plans and moves generated flag arrays, walks the edges of the decision, and must finish without a report."""
    csrc = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "repack-sanitize", "REPACK_SANITIZE_OUT=" + str(tmp_path / "repack_sanitize")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "repack ok" in out.stdout, out.stdout + out.stderr
