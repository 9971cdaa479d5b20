"""The overflow rule of the two 32-entry traversal stacks (include/ptmi_plugin.h, Part 3) on the CPU oracle.

The inputs and their expected records come from tests/stack_cases.py: computed there from the rule and the construction in float64,
never from the code under test.  The GPU side of the same cases is tests/test_gpu_stack_overflow.py."""
import os
import subprocess

import numpy as np
import pytest

import stack_cases as sc
from unity_webgpu_pathtracer_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "deep_cwbvh32": lambda: sc.deep_cwbvh(32),          # the last depth that fits
    "deep_cwbvh33": lambda: sc.deep_cwbvh(33),          # the first that does not
    "deep_cwbvh40": lambda: sc.deep_cwbvh(40),
    "deep_tlas48": lambda: sc.deep_tlas(48),
    "deep_blas_instances": lambda: sc.deep_blas_instances(40),
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_expectations_state_the_rule():
    """What the helper expects, spelled out: which rays the rule loses."""
    for levels, lost in ((32, []), (33, [32]), (40, list(range(32, 40)))):
        c = sc.deep_cwbvh(levels)
        assert c.families["terminal_first"]["hit"].all() and c.families["terminal_first"]["overflows"] == 0
        f = c.families["chain_first"]
        assert list(np.where(~f["hit"])[0]) == lost                          # entry k sits at stack index k; the last terminal is entered directly
        assert f["overflows"] == (levels + 1 if lost else 0)
        miss = _bits(f["expected"][~f["hit"]])
        assert (miss == np.array([sc.FAR.view(np.uint32), 0, 0, sc.MISS], np.uint32)).all()          # {tmax, 0, 0, 0xFFFFFFFF}
    t = sc.deep_tlas(48)
    assert t.families["leaf_first"]["hit"].all()
    assert list(np.where(~t.families["chain_first"]["hit"])[0]) == list(range(32, 47))
    for fam, x0 in (("leaf_first", -10.0), ("chain_first", 100.0)):
        e = t.families[fam]["expected"]
        hit = t.families[fam]["hit"]
        assert (e[hit, 0] == np.abs(np.arange(48) - x0)[hit]).all()           # the closed-form t: instance j stands at x = j


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_follows_the_rule(oracle, name):
    case = CASES[name]()
    buffers = case.buffers(oracle)
    for fam, f in case.families.items():
        rays = f["rays"].view(oracle.ORACLE_RAY_DTYPE).reshape(-1)
        rec, st = oracle.trace_rays(buffers, rays)
        same = (_bits(rec) == _bits(f["expected"])).all(axis=1)
        assert same.all(), (name, fam, np.where(~same)[0], rec[~same], f["expected"][~same])
        assert st.stackOverflows == f["overflows"], (name, fam, st.stackOverflows)
        assert st.maxStackDepth == f["max_depth"], (name, fam, st.maxStackDepth)
        assert st.closestHitRays == len(rays) and st.shadowRays == 0
        # any hit: occluded exactly where the closest-hit expectation is a hit
        shadow = f["rays"].copy()
        shadow[:, 7] = 1.0
        occ, st = oracle.trace_rays(buffers, shadow.view(oracle.ORACLE_RAY_DTYPE).reshape(-1))
        assert ((_bits(occ[:, 3]) != sc.MISS) == f["hit"]).all(), (name, fam)
        assert st.stackOverflows == f["overflows"] and st.shadowRays == len(rays)
    if not case.scene.use_tlas:
        # the flat walk is also what oracle.trace_uv reports
        f = case.families["chain_first"]
        rec, _, _ = oracle.trace_uv(buffers, f["rays"].view(oracle.ORACLE_RAY_DTYPE).reshape(-1))
        assert (_bits(rec) == _bits(f["expected"])).all()


def test_oracle_renders_the_builder_made_chain(oracle):
    """A TLAS from BuildTLAS deeper than the stack: the frame is finished (before the fix the walk read past its stack) and
    the path is proven to be reached."""
    case = sc.Case("chain", sc.geometric_chain_scene())
    buffers = case.buffers(oracle)
    T = case.bvh.tlas_data[:case.bvh.tlas_index_offset].view(sc.abi.TLAS_NODE)
    node, depth = 0, 0
    while T[node]["triCount"] == 0:                                            # a chain: the left child goes on, the right one is a leaf
        assert T[T[node]["right"]]["triCount"] > 0
        node, depth = T[node]["left"], depth + 1
    assert depth > sc.STACK + 8, depth
    p = scenes.frame_params(case.scene, 32, 24, spp=2, seed=0xABCD)
    for any_hit in (False, True):
        frame, st = oracle.render(buffers, p, shadow_any_hit=any_hit)
        assert np.isfinite(frame).all() and st.stackOverflows > 0 and st.tlasNodeVisits > 32 * 24 * depth


def test_fixture_of_the_sanitizer_program_is_current():
    with open(os.path.join(ROOT, "tests", "golden", "stack_overflow_cases.bin"), "rb") as fh:
        assert fh.read() == sc.fixture_bytes()


def test_oracle_walks_are_clean_under_sanitizers():
    """make -C oracle asan-stack-test: a stand-alone program (no Python, nothing preloaded) built with -fsanitize=address,undefined
    traces deep_cwbvh(40) and deep_tlas(48) through the oracle.  Before the fix UBSan stopped it in RayIntersectTLAS
    (index 46 out of bounds for type 'unsigned int [32]')."""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "asan-stack-test"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.count("0 records differ") == 4 and "stackOverflows 48 (expected 48)" in out.stdout, out.stdout
