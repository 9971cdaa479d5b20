"""The lightmap lookup on the host (include/ptmi_plugin.h Part 22): the host twin (csrc/lightmap_lookup_host.cpp)
equals the numpy restatement (tests/lightmap_lookup_ref.py) bit for bit over tests/lightmap_lookup_cases.py; a constant image
comes back exactly, an affine ramp within a measured bound of float64, an invalid texel is never read; refusals; the struct, the
kernel resources, the sanitizer program."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin

from kernel_resources import resources
import lightmap_lookup_cases as cases
import lightmap_lookup_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc")
F = np.float32
NONE = abi.PT_LIGHTMAP_NONE
CONTEXT_SYMBOLS = ["PTBindLightmaps", "PTLightmapLookup", "PTShadeLightmapped", "PTShadeLightmappedFrame"]
HOST_SYMBOLS = ["PTLightmapLookupHost"]
# texel (x, y) of channel c holds a + bx * x + by * y
RAMP = ((1.0, 0.25, 0.5), (2.0, -0.125, 0.75), (0.5, 1.0, -0.0625))
# The numpy restatement against a float64 evaluation of RAMP at the entries' (x, y), each clamped to the texel centres (beyond the
# outermost centres only one tap of a pair is inside the image, and the filter returns it), over the four sizes and the 1,024
# entries of the case generator: the largest absolute difference is 9.5367e-07 (size 24 x 8, channel 2, values up to 23.3).  The cap
# is twice that.
RAMP_MEASURED = 9.5367431640625e-07
RAMP_CAP = 2 * RAMP_MEASURED


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def attrs():
    return cases.tri_attrs()


@pytest.fixture(scope="module")
def rows():
    return cases.entries()


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_lightmap_shade_symbols_are_exported():
    lib = plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in CONTEXT_SYMBOLS + HOST_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).restype is C.c_int
    assert "Part 22: first hits shaded from baked lightmaps" in header


def test_lightmap_binding_matches_c_header():
    fields = ["firstPrim", "primCount", "instance", "flags", "width", "height", "reserved", "dImage", "dUvs"]
    lines = ['printf("%zu %zu %u %u %u\\n", sizeof(PTLightmapBinding), sizeof(PTShadeInputs), PT_LIGHTMAP_TWO_SIDED, PT_LIGHTMAP_MAX_BINDINGS, PT_LIGHTMAP_NONE);']
    lines += [f'printf("{f} %zu\\n", offsetof(PTLightmapBinding, {f}));' for f in fields]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = subprocess.check_output([exe]).decode().splitlines()
    assert [int(x) for x in got[0].split()] == [48, 120, abi.PT_LIGHTMAP_TWO_SIDED, abi.PT_LIGHTMAP_MAX_BINDINGS, abi.PT_LIGHTMAP_NONE]
    assert C.sizeof(abi.PTLightmapBinding) == 48 and C.sizeof(abi.PTShadeInputs) == 120
    offs = dict(l.split(" ") for l in got[1:])
    for f in fields:
        assert int(offs[f]) == getattr(abi.PTLightmapBinding, f).offset, f


# ---------------------------------------------------------------------------------------------------------------------------
# the twin against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
TABLES = sorted(cases.tables(cases.tri_attrs()))


@pytest.mark.parametrize("name", TABLES)
def test_twin_equals_restatement(attrs, rows, name):
    table = cases.tables(attrs)[name]
    got, which = plugin.lightmap_lookup(table, attrs, cases.MATERIALS, *rows)
    want, want_which = ref.lookup(table, attrs, cases.MATERIALS, *rows)
    assert (which == want_which).all()
    assert (_bits(got) == _bits(want)).all()
    assert not got[which == NONE].view(np.uint32).any() and not got[:, 3].view(np.uint32).any()          # zero bits; m2 = 0.0f
    hits, surf = rows[1], rows[2]
    miss = (hits.view(np.uint32)[:, 3] == NONE) | (surf.view(np.uint32)[:, 7] >= cases.MATERIALS)
    assert miss.sum() > len(miss) // 8 and (which[miss] == NONE).all()                                    # every seventh row, and the bad material indices
    assert (which[which != NONE] < max(len(table), 1)).all()


def test_named_edge_cases(attrs, rows):
    """rows 0 ... 15 sit on the special UVs at size 8; rows 16 ... 19 around the span [10, 20)"""
    rays, hits, surf = rows
    img = cases.image("full", 8, 8, seed=1)
    got, which = plugin.lightmap_lookup([cases.binding(img)], attrs, cases.MATERIALS, rays, hits, surf)
    # x on -1 and on the width: nothing; the NaN: nothing; just outside (-0.07 * 8 - 0.5 = -1.06): nothing
    for base in (0, 8):
        assert list(which[base:base + 8] == NONE) == [True, True, False, False, True, False, False, True], which[base:base + 8]
    # a texel centre returns the texel, bit for bit (fx = 0, fy = 0: c00 + 0 * (c10 - c00))
    assert (_bits(got[2, 0:3]) == _bits(img[3, 3, 0:3])).all() and (_bits(got[10, 0:3]) == _bits(img[3, 3, 0:3])).all()
    # a texel edge is the mean of the two texels (fx = 0.5)
    assert np.allclose(got[3, 0:3], (img[3, 3, 0:3] + img[3, 4, 0:3]) / 2, rtol=1e-6) and np.allclose(got[11, 0:3], (img[3, 3, 0:3] + img[4, 3, 0:3]) / 2, rtol=1e-6)
    # the first and the last half texel: the outer tap lies outside the image, the inner one comes back alone
    assert (_bits(got[5, 0:3]) == _bits(img[3, 0, 0:3])).all() and (_bits(got[6, 0:3]) == _bits(img[3, 7, 0:3])).all()
    # around a span: just below and just past it nothing, its first and last primitive found
    _, which = plugin.lightmap_lookup(cases.tables(attrs)["span-10-20"], attrs, cases.MATERIALS, rays, hits, surf)
    assert list(which[16:20] != NONE) == [False, True, True, False]
    prim = hits.view(np.uint32)[:, 3]
    assert ((which != NONE) <= ((prim >= 10) & (prim < 20))).all()


def test_binding_order_instances_and_sides(attrs, rows):
    rays, hits, surf = rows
    prim, inst = hits.view(np.uint32)[:, 3], surf.view(np.uint32)[:, 10]
    miss, back = ref.step1(cases.MATERIALS, rays, hits, surf)
    assert 0.3 < back[~miss].mean() < 0.7
    t = cases.tables(attrs)
    look = lambda name: plugin.lightmap_lookup(t[name], attrs, cases.MATERIALS, rays, hits, surf)[1]
    # overlapping spans: the lower index wins where both match
    which = look("overlap")
    both = ~miss & (prim >= 20) & (prim < 40)
    assert both.sum() > 50 and set(np.unique(which[both])) <= {0, NONE} and (which[~miss & (prim >= 40) & (prim < 60)] != 0).all()
    # the same span bound twice with different instances
    which = look("instances")
    assert (which[which == 0].size and (inst[which == 0] == 1).all()) and (which[which == 1].size and (inst[which == 1] == 2).all())
    assert (which[~miss & ((inst == 0) | (inst == NONE))] == NONE).all()
    # an instance's binding first, any instance second
    which = look("instance-then-any")
    assert (inst[which == 0] == 0).all() and not back[which == 0].any() and (which[~miss & (inst == 0) & ~back] != 1).all()
    # back-facing hits with and without PT_LIGHTMAP_TWO_SIDED
    assert (look("one-sided")[back] == NONE).all()
    which = look("one-sided-then-two")
    assert (which[back] != 0).all() and (which[back] == 1).sum() > 100 and (which[~back & ~miss] != 1).all()
    # 64 bindings of one primitive each: the binding is the primitive
    which = look("sixty-four")
    assert (which[which != NONE] == prim[which != NONE]).all() and len(np.unique(which)) > 40


# ---------------------------------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.SIZES)
@pytest.mark.parametrize("kind", ["full", "checker", "single", "w-values"])
def test_constant_image_comes_back_exactly(attrs, rows, size, kind):
    const = np.array([0.7, 3.1, 1e-3], F)
    img = cases.image(kind, *size, seed=2, constant=const, poison=True)
    got, which = plugin.lightmap_lookup([cases.binding(img, two_sided=True)], attrs, cases.MATERIALS, *rows)
    found = which != NONE
    assert found.sum() > 10
    assert (_bits(got[found, 0:3]) == _bits(const)).all()


@pytest.mark.parametrize("size", cases.SIZES)
def test_affine_ramp_is_within_the_measured_bound(attrs, rows, size):
    w, h = size
    img = cases.image("full", w, h, ramp=RAMP)
    table = [cases.binding(img, two_sided=True)]
    got, which = plugin.lightmap_lookup(table, attrs, cases.MATERIALS, *rows)
    restated, _, x, y = ref.lookup(table, attrs, cases.MATERIALS, *rows, details=True)
    found = which != NONE
    assert found.sum() > 800
    xc, yc = np.clip(x[found].astype(np.float64), 0, w - 1), np.clip(y[found].astype(np.float64), 0, h - 1)
    worst = worst_restated = 0.0
    for c in range(3):
        want = RAMP[c][0] + RAMP[c][1] * xc + RAMP[c][2] * yc
        worst = max(worst, np.abs(got[found, c].astype(np.float64) - want).max())
        worst_restated = max(worst_restated, np.abs(restated[found, c].astype(np.float64) - want).max())
    print(f"[lightmap] ramp {w} x {h}: twin {worst:.4e}, restatement {worst_restated:.4e} (cap {RAMP_CAP:.4e})")
    assert worst_restated <= RAMP_MEASURED and worst <= RAMP_CAP


@pytest.mark.parametrize("name", TABLES)
def test_a_found_entry_never_reads_an_invalid_tap(attrs, rows, name):
    """the rgb of every texel that is not valid is NaN: nothing of it reaches an output, and what is found does not change"""
    clean = plugin.lightmap_lookup(cases.tables(attrs)[name], attrs, cases.MATERIALS, *rows)
    got, which = plugin.lightmap_lookup(cases.tables(attrs, poison=True)[name], attrs, cases.MATERIALS, *rows)
    assert np.isfinite(got).all()
    assert (which == clean[1]).all() and (_bits(got) == _bits(clean[0])).all()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _table(a, n=1, **over):
    t = (abi.PTLightmapBinding * n)()
    for b in t:
        b.firstPrim, b.primCount, b.instance, b.flags, b.width, b.height, b.dImage, b.dUvs = 0, cases.PRIMS, NONE, 0, 8, 8, a, None
        for k, v in over.items():
            if k == "reserved":
                b.reserved[1] = v
            else:
                setattr(b, k, v)
    return t


def test_lightmap_shade_refusals():
    lib = plugin.load_library()
    buf = np.zeros(8192, np.uint8)
    a = buf.ctypes.data
    a += (-a) % 16
    b = a + 4096
    host = lambda t, n, attrs=a, rays=a, out=b: lib.PTLightmapLookupHost(t, n, attrs, cases.PRIMS, cases.MATERIALS, rays, a, a, 0, out, None)
    assert host(_table(a), 1) == 1 and host(None, 0) == 1
    bad = [({"dImage": None}, b"image"), ({"dImage": a + 8}, b"aligned"), ({"dUvs": a + 4}, b"aligned"), ({"width": 0}, b"size"), ({"height": 8193}, b"size"),
           ({"primCount": 0}, b"span"), ({"firstPrim": 1}, b"span"), ({"firstPrim": 0xFFFFFFFF, "primCount": 2}, b"span"), ({"flags": 2}, b"flag"),
           ({"reserved": 1}, b"reserved")]
    for over, word in bad:
        assert host(_table(a, **over), 1) == 0 and word in lib.PTGetBVHBuildError(), over
    assert host(_table(a, 65), 65) == 0 and b"at most 64" in lib.PTGetBVHBuildError()
    assert host(None, 1) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert host(_table(a), 1, attrs=None) == 0 and b"attrs" in lib.PTGetBVHBuildError()
    assert host(_table(a, dUvs=a), 1, attrs=None) == 1                                          # every binding has its UVs
    assert lib.PTLightmapLookupHost(_table(a), 1, a, cases.PRIMS, cases.MATERIALS, None, a, a, 1, b, None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    assert lib.PTLightmapLookupHost(_table(a), 1, a, cases.PRIMS, cases.MATERIALS, a, a, a, 1, None, None) == 0 and b"NULL" in lib.PTGetBVHBuildError()
    with pytest.raises(plugin.PluginError):
        plugin.lightmap_lookup([cases.binding(np.zeros((8, 8, 4), F), 0, cases.PRIMS + 1)], cases.tri_attrs(), cases.MATERIALS, *cases.entries(32))
    # the context's calls: refused on their arguments alone, before the context is used
    p = abi.PTFrameParams()
    p.structSize = C.sizeof(p)
    p.OutputWidth = p.OutputHeight = 8
    from test_shade_baked import _inputs
    ok = _inputs(buf[a - buf.ctypes.data:])
    calls = {"PTBindLightmaps": lambda c: lib.PTBindLightmaps(c, _table(a), 1),
             "PTLightmapLookup": lambda c: lib.PTLightmapLookup(c, a, a, a, 1, b, None),
             "PTShadeLightmapped": lambda c: lib.PTShadeLightmapped(c, C.byref(ok), a, a, a, 1, b),
             "PTShadeLightmappedFrame": lambda c: lib.PTShadeLightmappedFrame(c, C.byref(p), C.byref(ok), b, None)}
    for name, call in calls.items():
        assert call(None) == abi.PT_ERR_INVALID_ARG, name
        assert b"ctx" in lib.PTGetLastError() and name.encode() in lib.PTGetLastError()
    ctx = C.c_void_p(1)         # never dereferenced: every call below is refused on its arguments alone
    assert lib.PTBindLightmaps(ctx, None, 1) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError()
    assert lib.PTBindLightmaps(ctx, _table(a, 65), 65) == abi.PT_ERR_INVALID_ARG and b"at most 64" in lib.PTGetLastError()
    for args in ((None, a, a, b, None), (a, None, a, b, None), (a, a, None, b, None), (a, a, a, None, None)):
        assert lib.PTLightmapLookup(ctx, args[0], args[1], args[2], 1, args[3], args[4]) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError(), args
    for args in ((a + 8, a, a, b, None), (a, a + 4, a, b, None), (a, a, a + 8, b, None), (a, a, a, b + 8, None), (a, a, a, b, b + 2)):
        assert lib.PTLightmapLookup(ctx, args[0], args[1], args[2], 1, args[3], args[4]) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError(), args
    # inputs are checked exactly as PTShadeBaked checks them
    for over, word in [({"res": 12}, b"res"), ({"levels": 1}, b"levels"), ({"dSH": None}, b"NULL"), ({"dDFG": None}, b"NULL"), ({"dfgRes": 17}, b"res"),
                       ({"dBoxes": a, "dProbes": None, "probeCount": 0}, b"boxes without probes"), ({"dSH": a + 8}, b"aligned"), ({"dDFG": a + 4}, b"aligned")]:
        s = _inputs(buf[a - buf.ctypes.data:], **over)
        for call in (lambda: lib.PTShadeLightmapped(ctx, C.byref(s), a, a, a, 1, b), lambda: lib.PTShadeBaked(ctx, C.byref(s), a, a, a, 1, b),
                     lambda: lib.PTShadeLightmappedFrame(ctx, C.byref(p), C.byref(s), b, None)):
            assert call() == abi.PT_ERR_INVALID_ARG and word in lib.PTGetLastError(), over
    assert lib.PTShadeLightmapped(ctx, None, a, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and b"inputs" in lib.PTGetLastError()
    assert lib.PTShadeLightmapped(ctx, C.byref(ok), None, a, a, 1, b) == abi.PT_ERR_INVALID_ARG and lib.PTShadeLightmapped(ctx, C.byref(ok), a, a, a, 1, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeLightmapped(ctx, C.byref(ok), a, a, a, 1, b + 8) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()
    assert lib.PTShadeLightmappedFrame(ctx, None, C.byref(ok), b, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeLightmappedFrame(ctx, C.byref(p), C.byref(ok), None, None) == abi.PT_ERR_INVALID_ARG
    assert lib.PTShadeLightmappedFrame(ctx, C.byref(p), C.byref(ok), b, a + 8) == abi.PT_ERR_INVALID_ARG and b"aligned" in lib.PTGetLastError()


# ---------------------------------------------------------------------------------------------------------------------------
# kernel resources and the sanitizer build
# ---------------------------------------------------------------------------------------------------------------------------
KERNELS = ["pt_lightmap_lookup", "pt_shade_lightmapped", "pt_shade_lightmapped_placed"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_lightmap_shade_kernel_resources():
    """no kernel of the compile unit has scratch, spills or LDS; the table of DESIGN.md 5.27 is this test's output"""
    res = resources("pt_shade_lightmap.hip")
    assert len(res) == len(KERNELS), sorted(res)
    for name in KERNELS:
        hits = [r for k, r in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1, (name, sorted(res))
        print(f"[resources] {name}: {hits[0]}")
        assert hits[0]["scratch"] == 0 and hits[0]["vgpr_spill"] == 0 and hits[0]["lds"] == 0, (name, hits[0])
        assert hits[0]["occupancy"] >= 4, (name, hits[0])


def test_lightmap_shade_sanitize_target_runs_clean():
    """the host twin under AddressSanitizer + UBSan in a stand-alone program (csrc/lightmap_shade_sanitize_main.cpp)"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", CSRC, "lightmap-shade-sanitize", "LIGHTMAP_SHADE_SANITIZE_OUT=" + os.path.join(d, "lightmap_shade_sanitize")],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "lightmap shade ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
