"""Adaptive sampling (include/ptmi_plugin.h Part 7) without a GPU: exports, struct layout, argument checks, the host-side block
selection against hand-made maps, the list slot -> pixel mapping against pt_slot_to_pixel's, and the compile-time resources of
the list-mapped kernels.  tests/test_gpu_adaptive.py holds the kernels to the contract."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from unity_webgpu_pathtracer_amd.pathtracer import list_slot_to_pixel, select_blocks
from kernel_resources import resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTIVE_SYMBOLS = ["PTAdaptiveBegin", "PTAdaptiveEnd", "PTSetActiveBlocks", "PTSelectActiveBlocks", "PTGetActiveBlocks",
                    "PTGetBlockSamples", "PTRenderPassActive", "PTRenderPassActiveTo", "PTAccumulateMomentsActive",
                    "PTAccumulateMomentsActiveTo"]


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_adaptive_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in ADAPTIVE_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int


def test_adaptive_struct_matches_c_header():
    fs = ["structSize", "threshold", "maxSamples", "addSamples", "dilate"]
    lines = ['printf("PTAdaptiveSelect %zu\\n", sizeof(PTAdaptiveSelect));']
    lines += [f'printf("PTAdaptiveSelect.{f} %zu\\n", offsetof(PTAdaptiveSelect, {f}));' for f in fs]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTAdaptiveSelect"]) == C.sizeof(abi.PTAdaptiveSelect) == 20
    for f in fs:
        assert int(got[f"PTAdaptiveSelect.{f}"]) == getattr(abi.PTAdaptiveSelect, f).offset, f
    s = abi.adaptive_select(0.05, 64, 8)
    assert (s.structSize, s.threshold, s.maxSamples, s.addSamples, s.dilate) == (20, np.float32(0.05), 64, 8, 1)


def test_adaptive_argument_errors_without_context():
    lib = plugin.load_library()
    p = abi.PTFrameParams()
    sel = abi.adaptive_select(0.05, 64, 8)
    n = C.c_uint32()
    ids = (C.c_uint32 * 4)()
    buf = (C.c_float * 16)()
    for rc in (lib.PTAdaptiveBegin(None, C.byref(p), 0), lib.PTAdaptiveEnd(None),
               lib.PTSetActiveBlocks(None, ids, 4, C.byref(n)), lib.PTSelectActiveBlocks(None, C.byref(sel), C.byref(n)),
               lib.PTGetActiveBlocks(None, ids, 4, C.byref(n)), lib.PTGetBlockSamples(None, ids, 4),
               lib.PTRenderPassActive(None, C.byref(p), 1),
               lib.PTRenderPassActiveTo(None, C.byref(p), 1, C.addressof(buf), C.addressof(buf)),
               lib.PTAccumulateMomentsActive(None, C.byref(p), 1),
               lib.PTAccumulateMomentsActiveTo(None, C.byref(p), 1, C.addressof(buf), C.addressof(buf))):
        assert rc == abi.PT_ERR_INVALID_ARG
        assert b"ctx" in lib.PTGetLastError() and b"NULL" in lib.PTGetLastError()


# ---------------------------------------------------------------------------------------------------------------------------
# selection (PTSelectActiveBlocks restated)
# ---------------------------------------------------------------------------------------------------------------------------
def test_select_blocks_on_hand_made_maps():
    f32 = np.float32
    tiles = np.zeros((3, 4), f32)
    samples = np.full((3, 4), 8, np.uint32)
    # at the threshold: > and not >=
    tiles[1, 1] = f32(0.05)
    tiles[1, 2] = np.nextafter(f32(0.05), f32(1))
    assert select_blocks(tiles, samples, 0.05, 64, 8, False).tolist() == [1 * 4 + 2]
    assert select_blocks(tiles, samples, np.nextafter(f32(0.05), f32(0)), 64, 8, False).tolist() == [5, 6]
    # a corner block under dilation: itself and its three neighbours
    tiles[:] = 0
    tiles[0, 0] = 1
    assert select_blocks(tiles, samples, 0.05, 64, 8, True).tolist() == [0, 1, 4, 5]
    tiles[0, 0], tiles[2, 3] = 0, 1
    assert select_blocks(tiles, samples, 0.05, 64, 8, True).tolist() == [6, 7, 10, 11]
    # an inner block: all nine
    tiles[:] = 0
    tiles[1, 1] = 1
    assert select_blocks(tiles, samples, 0.05, 64, 8, True).tolist() == [0, 1, 2, 4, 5, 6, 8, 9, 10]
    # the max_samples cut: n + add <= max, for the block itself and for dilated neighbours
    samples[1, 1] = 56
    assert select_blocks(tiles, samples, 0.05, 64, 8, False).tolist() == [5]
    samples[1, 1] = 57
    assert select_blocks(tiles, samples, 0.05, 64, 8, False).tolist() == []
    assert select_blocks(tiles, samples, 0.05, 64, 8, True).tolist() == []          # a block over the limit does not dilate either
    samples[1, 1] = 8
    samples[0, 1], samples[2, 2] = 57, 60
    assert select_blocks(tiles, samples, 0.05, 64, 8, True).tolist() == [0, 2, 4, 5, 6, 8, 9]
    # nothing above the threshold: empty, of the right type
    got = select_blocks(np.zeros((3, 4), f32), samples, 0.05, 64, 8, True)
    assert got.dtype == np.uint32 and got.size == 0
    # NaN never compares greater
    tiles[:] = np.nan
    assert select_blocks(tiles, samples, 0.05, 64, 8, True).size == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the list mapping against pt_slot_to_pixel's
# ---------------------------------------------------------------------------------------------------------------------------
def _slot_to_pixel(W, H, slots):
    """pt_slot_to_pixel of csrc/pt_launch.h for rank 0 of 1 and full coverage, restated."""
    bx_n = (W + 15) // 16
    block, tid = slots >> 8, slots & 255
    by, bx = block // bx_n, block % bx_n
    wave, lane = tid >> 6, tid & 63
    px = bx * 16 + (wave & 1) * 8 + (lane & 7)
    py = by * 16 + (wave >> 1) * 8 + (lane >> 3)
    return px, py, (px < W) & (py < H)


def test_list_mapping_with_all_blocks_is_the_frame_mapping():
    W, H = 40, 24                                   # 3 x 2 blocks, the last column 8 px wide, the last row 8 px high
    ids = np.arange(6)
    px, py, ok = list_slot_to_pixel(W, H, ids)
    rx, ry, rok = _slot_to_pixel(W, H, np.arange(6 * 256))
    assert (px == rx).all() and (py == ry).all() and (ok == rok).all()
    assert int(ok.sum()) == W * H
    assert len({(int(x), int(y)) for x, y in zip(px[ok], py[ok])}) == W * H        # every pixel exactly once
    # a sub-list: entry e holds block ids[e], whatever its position
    sub = np.array([1, 4, 5])
    sx, sy, sok = list_slot_to_pixel(W, H, sub)
    for e, b in enumerate(sub):
        s = slice(e * 256, (e + 1) * 256)
        t = slice(b * 256, (b + 1) * 256)
        assert (sx[s] == rx[t]).all() and (sy[s] == ry[t]).all() and (sok[s] == rok[t]).all()
    assert int(sok[512:].sum()) == 8 * 8                                             # block 5 is partial both ways
    # dispatch coverage cuts inside blocks
    cx, cy, cok = list_slot_to_pixel(44, 28, np.arange(6), cover=(40, 24))
    assert int(cok.sum()) == 40 * 24 and (cx[cok] < 40).all() and (cy[cok] < 24).all()


# ---------------------------------------------------------------------------------------------------------------------------
# kernel resources
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_list_mapped_kernels_keep_the_register_budget():
    with ThreadPoolExecutor(3) as ex:
        fa = ex.submit(resources, "pt_wavefront.hip", "a")
        fb = ex.submit(resources, "pt_wavefront.hip", "b")
        fm = ex.submit(resources, "pt_moments.hip")
        res_a, res_b, res_m = fa.result(), fb.result(), fm.result()
    for unit, res in (("a", res_a), ("b", res_b)):
        shade = {k: v for k, v in res.items() if "pt_wf_shadeILb0E" in k and "PTListMap" in k}
        assert len(shade) == 1, sorted(res)
        for k, r in shade.items():
            print(f"[resources] unit {unit} {k}: {r}")
            assert r["scratch"] == 0 and r["vgprs"] <= 128 and r["occupancy"] >= 4, (unit, r)
        for part in ("pt_wf_initI", "pt_wf_resolveI"):
            hits = [v for k, v in res.items() if part in k and "PTListMap" in k]
            assert hits, (part, sorted(res))
            for r in hits:
                assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (part, r)
    r = res_m["pt_moments_accumulate_blocks"]
    print(f"[resources] pt_moments_accumulate_blocks: {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, r
