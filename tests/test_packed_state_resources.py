"""The packed path state of a repacked sequence (csrc/pt_wf_state.h, shade_slot's PACKED in csrc/pt_wf_shade.h, csrc/pt_repack.hip;
DESIGN.md 4, 9.1) against its budgets, at compile time.

The RNG state and the pending throughput ride in the fourth lanes of rad, envC, lightC and thr, so the shade kernel of a repacked
sequence requests two arrays fewer than pt_wf_shade and the repack moves two planes fewer.  One more value lives across
sample_brdf for it, and the shade kernel sits on its 128-VGPR line: the line of tests/test_repack.py must hold, and the cleanup
kernels must not have paid for it either.  The figures of the commit before the packed layout were read from a compilation of
that commit with the same compiler and flags."""
import shutil

import pytest

from kernel_resources import resources
from kernel_streams import streams

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")

# pt_wf_cleanup_repack<STATS, TLAS> before the packed layout: scratch bytes per lane and waves per SIMD
PARENT_CLEANUP_SCRATCH = 192
PARENT_CLEANUP_OCCUPANCY = {"ILb0ELb0E": 3, "ILb0ELb1E": 2, "ILb1ELb0E": 2, "ILb1ELb1E": 2}
# pt_wf_repack_out before the packed layout: global_load and global_store instructions in its stream
PARENT_REPACK_OUT_LOADS, PARENT_REPACK_OUT_STORES = 15, 15


def _count(stream, prefix):
    return sum(l.startswith(prefix) for l in stream)


def _one(table, part):
    hits = [k for k in table if part in k]
    assert len(hits) == 1, (part, sorted(table))
    return table[hits[0]]


def test_repack_unit_keeps_its_lines():
    res = resources("pt_repack.hip", unit="a")
    shade = _one(res, "pt_wf_shade_repackILb0E")
    print(f"[resources] pt_wf_shade_repack<0>: {shade}")
    assert shade["vgprs"] <= 128 and shade["scratch"] == 0 and shade["occupancy"] >= 4, shade
    stats = _one(res, "pt_wf_shade_repackILb1E")
    print(f"[resources] pt_wf_shade_repack<1>: {stats}")
    assert stats["vgprs"] <= 128 and stats["scratch"] == 0, stats
    for inst, occupancy in PARENT_CLEANUP_OCCUPANCY.items():
        r = _one(res, "pt_wf_cleanup_repack" + inst)
        print(f"[resources] pt_wf_cleanup_repack<{inst}>: {r}")
        assert r["scratch"] <= PARENT_CLEANUP_SCRATCH and r["occupancy"] >= occupancy, (inst, r)
    moves = {k: r for k, r in res.items() if "pt_wf_repack_" in k}
    assert len(moves) == 4, sorted(res)
    for k, r in moves.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)


def test_packed_shade_requests_fewer_arrays_than_the_plain_one():
    """one load more than pt_wf_shade<false, PTTileMap> for pixelOf, two fewer for rng and pthr"""
    packed = _one(streams("pt_repack.hip", unit="a"), "pt_wf_shade_repackILb0E")
    plain = _one(streams("pt_wavefront.hip", unit="a"), "pt_wf_shadeILb0E9PTTileMap")
    n_packed, n_plain = _count(packed, "global_load"), _count(plain, "global_load")
    print(f"[streams] global_load: pt_wf_shade_repack<0> {n_packed}, pt_wf_shade<0, PTTileMap> {n_plain}")
    assert n_packed < n_plain, (n_packed, n_plain)


def test_repack_moves_two_planes_fewer():
    out = _one(streams("pt_repack.hip", unit="a"), "pt_wf_repack_outE")
    loads, stores = _count(out, "global_load"), _count(out, "global_store")
    print(f"[streams] pt_wf_repack_out: {loads} loads, {stores} stores ({PARENT_REPACK_OUT_LOADS}, {PARENT_REPACK_OUT_STORES} before)")
    assert loads == PARENT_REPACK_OUT_LOADS - 2 and stores == PARENT_REPACK_OUT_STORES - 2, (loads, stores)
