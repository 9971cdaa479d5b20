"""The lightmap denoiser (PTDenoiseLightmap / PathTracer.denoise_lightmap / bake_lightmap(denoise=...), include/ptmi_plugin.h Part 17)
on the MI355X.

The kernels are held to the host twin byte for byte (the twin to the numpy restatement by tests/test_lightmap_denoise.py) on the
lists of lmfilter_cases.py, in place and out of place, and on the gathered list of a real chart.  A denoised bake is the resolve of
the denoised gather, bit for bit; a bake without `denoise` is what it was.  Only the quality statement compares against something
else: a 4,096-sample bake of the same receivers."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
import chart_cases
import lmfilter_cases as cases

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL_F = 7.25


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def box():
    scene = chart_cases.lit_box()
    pt = PathTracer(scene, width=32, height=32, samplesPerPass=1, maxRayBounces=3, schedule=1)
    yield pt, chart_cases.floor_only_uvs(len(scene.tri_attrs))
    pt.close()


def _upload(pt, texels, recv, irr):
    import torch
    dev = torch.device(f"cuda:{pt.device}")
    return (torch.from_numpy(np.ascontiguousarray(texels).view(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(recv)).to(dev),
            torch.from_numpy(np.ascontiguousarray(irr)).to(dev))


def _assert_rows(got, want, what):
    diff = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
    assert got.shape == want.shape and len(diff) == 0, (what, len(diff), len(want), got[diff[:3]], want[diff[:3]])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. device against twin
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.SIZES)
@pytest.mark.parametrize("cover", [1.0, 0.6])
def test_device_equals_twin(box, size, cover):
    pt, _ = box
    w, h = size
    texels, recv, irr, _ = cases.generated_list(w, h, seed=w * 100 + h, cover=cover)
    d = _upload(pt, texels, recv, irr)
    for it in cases.ITERATIONS:
        want = plugin.denoise_lightmap(texels, recv, irr, w, h, cases.SAMPLES, iterations=it)
        got = pt.denoise_lightmap(*d, w, h, cases.SAMPLES, iterations=it).cpu().numpy()
        _assert_rows(got, want, (size, cover, it))


@pytest.mark.parametrize("noise_seed", [None, 11])
def test_atlas64_device_equals_twin(box, noise_seed):
    pt, _ = box
    texels, recv, irr, _, _ = cases.atlas64_list(noise_seed)
    d = _upload(pt, texels, recv, irr)
    for it in cases.ITERATIONS:
        kw = dict(sigma_luminance=1e30) if noise_seed is None else {}
        want = plugin.denoise_lightmap(texels, recv, irr, 64, 64, cases.SAMPLES, params=dict(kw, iterations=it))
        _assert_rows(pt.denoise_lightmap(*d, 64, 64, cases.SAMPLES, params=dict(kw, iterations=it)).cpu().numpy(), want, (noise_seed, it))


def test_parameters_and_list_order(box):
    pt, _ = box
    texels, recv, irr, _ = cases.generated_list(33, 20, seed=5, cover=0.9)
    for kw in (dict(normal_power=0), dict(normal_power=7), dict(sigma_luminance=2.0, sigma_position=3.0, sigma_plane=0.5, iterations=3)):
        want = plugin.denoise_lightmap(texels, recv, irr, 33, 20, cases.SAMPLES, params=kw)
        _assert_rows(pt.denoise_lightmap(*_upload(pt, texels, recv, irr), 33, 20, cases.SAMPLES, params=kw).cpu().numpy(), want, kw)
    # a list in descending order: the texel state does not depend on the order of the list
    want = plugin.denoise_lightmap(texels, recv, irr, 33, 20, cases.SAMPLES)
    got = pt.denoise_lightmap(*_upload(pt, texels[::-1], recv[::-1], irr[::-1]), 33, 20, cases.SAMPLES).cpu().numpy()
    _assert_rows(got[::-1], want, "descending")


def test_in_place_and_nothing_past_count(box):
    import torch
    pt, _ = box
    lib = plugin.load_library()
    w, h = 130, 67
    texels, recv, irr, _ = cases.generated_list(w, h, seed=21, cover=0.7)
    n = len(texels)
    want = plugin.denoise_lightmap(texels, recv, irr, w, h, cases.SAMPLES)
    dt, dr, _ = _upload(pt, texels, recv, irr)
    dev = dt.device
    p = abi.lightmap_denoise_params(cases.SAMPLES)
    # out of place into a longer array, and in place in one: sentinels past count on both
    padded = np.full((n + 64, 4), SENTINEL_F, F)
    padded[:n] = irr
    src, out = torch.from_numpy(padded).to(dev), torch.full((n + 64, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    plugin.check(lib.PTDenoiseLightmap(pt.ctx, C.byref(p), dt.data_ptr(), dr.data_ptr(), src.data_ptr(), n, w, h, out.data_ptr()))
    plugin.check(lib.PTDenoiseLightmap(pt.ctx, C.byref(p), dt.data_ptr(), dr.data_ptr(), src.data_ptr(), n, w, h, src.data_ptr()))
    pt.synchronize()
    for name, t in (("out of place", out), ("in place", src)):
        got = t.cpu().numpy()
        _assert_rows(got[:n], want, name)
        assert (got[n:] == SENTINEL_F).all(), name + ": something past count was written"


def test_an_index_out_of_range_is_skipped(box):
    pt, _ = box
    texels, recv, irr, _ = cases.generated_list(17, 16, seed=6, cover=0.9, bad=False)
    want = plugin.denoise_lightmap(texels, recv, irr, 17, 16, cases.SAMPLES)
    t2 = np.concatenate([texels[:40], np.array([17 * 16, 0xFFFFFFFF], np.uint32), texels[40:]])
    r2 = np.concatenate([recv[:40], recv[:2], recv[40:]])
    e2 = np.concatenate([irr[:40], np.full((2, 4), 3.5, F), irr[40:]])
    got = pt.denoise_lightmap(*_upload(pt, t2, r2, e2), 17, 16, cases.SAMPLES).cpu().numpy()
    _assert_rows(np.concatenate([got[:40], got[42:]]), want, "the list around the skipped entries")
    assert (got[40:42] == 3.5).all(), "a skipped entry gets its input bytes"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. a real chart, the bake, the quality
# ---------------------------------------------------------------------------------------------------------------------------
W = H = 48


@pytest.fixture(scope="module")
def gathered(box):
    """the box's floor at 48 x 48: its list, an 8-sample gather and the 4,096-sample reference of the same receivers"""
    pt, uvs = box
    p = pt.params(seed=0)
    texels, recv = pt.chart_receivers(W, H, uvs=uvs, seed=77)
    assert texels.shape[0] == W * H
    irr8 = pt.irradiance(receivers=recv, spp=8, params=p)
    ref = pt.irradiance(receivers=recv, spp=4096, first_sample=1 << 20, params=p)
    return p, texels, recv, irr8, ref.cpu().numpy()


def test_a_real_chart_device_equals_twin(box, gathered):
    pt, _ = box
    _, texels, recv, irr8, _ = gathered
    got = pt.denoise_lightmap(texels, recv, irr8, W, H, 8).cpu().numpy()
    want = plugin.denoise_lightmap(texels.cpu().numpy().view(np.uint32), recv.cpu().numpy(), irr8.cpu().numpy(), W, H, 8)
    assert (_bits(got[:, :3]) != _bits(irr8.cpu().numpy()[:, :3])).any(axis=1).mean() > 0.9, "the filter did nothing"
    _assert_rows(got, want, "the box's floor")


def test_bake_lightmap_denoise(box, gathered):
    pt, uvs = box
    p, texels, recv, irr8, _ = gathered
    kw = dict(spp=8, uvs=uvs, seed=77, params=p)
    # None: today's bytes -- the scatter of the gather, dilated
    plain = pt.bake_lightmap(W, H, **kw)
    assert (_bits(plain) == _bits(pt.resolve_lightmap(texels, irr8, W, H).cpu().numpy())).all()
    assert (_bits(pt.bake_lightmap(W, H, denoise=None, **kw)) == _bits(plain)).all()
    scatter = np.zeros((H * W, 4), F)
    scatter[texels.cpu().numpy(), :3], scatter[texels.cpu().numpy(), 3] = irr8.cpu().numpy()[:, :3], 1.0
    assert (_bits(pt.bake_lightmap(W, H, dilate=0, **kw)) == _bits(scatter.reshape(H, W, 4))).all()
    # an int: that many levels between gather and resolve
    want = pt.resolve_lightmap(texels, pt.denoise_lightmap(texels, recv, irr8, W, H, 8, iterations=5), W, H).cpu().numpy()
    got = pt.bake_lightmap(W, H, denoise=5, **kw)
    assert (_bits(got) == _bits(want)).all() and (_bits(got) != _bits(plain)).any()
    want3 = pt.resolve_lightmap(texels, pt.denoise_lightmap(texels, recv, irr8, W, H, 8, iterations=3), W, H).cpu().numpy()
    assert (_bits(pt.bake_lightmap(W, H, denoise=3, **kw)) == _bits(want3)).all() and (_bits(want3) != _bits(want)).any()
    # a dict: the parameters
    over = dict(iterations=4, sigma_luminance=2.0, normal_power=2)
    want = pt.resolve_lightmap(texels, pt.denoise_lightmap(texels, recv, irr8, W, H, 8, params=over), W, H).cpu().numpy()
    assert (_bits(pt.bake_lightmap(W, H, denoise=over, **kw)) == _bits(want)).all()


def test_denoised_bake_is_closer_to_the_reference(box, gathered):
    """8 samples against 4,096 of the same receivers: the denoised error must be below the undenoised one.  The ratio is printed
    (DESIGN.md 5.22 has the figure measured on the card)."""
    pt, _ = box
    _, texels, recv, irr8, ref = gathered
    den = pt.denoise_lightmap(texels, recv, irr8, W, H, 8).cpu().numpy()
    raw = irr8.cpu().numpy()
    assert (ref[:, :3].max(axis=1) > 0).mean() > 0.9
    mse_raw = float(((raw[:, :3].astype(np.float64) - ref[:, :3]) ** 2).mean())
    mse_den = float(((den[:, :3].astype(np.float64) - ref[:, :3]) ** 2).mean())
    print(f"[lmfilter] box floor 48 x 48, 8 samples: mse {mse_raw:.4e} raw, {mse_den:.4e} denoised, ratio {mse_raw / mse_den:.2f}")
    assert mse_den < mse_raw


# ---------------------------------------------------------------------------------------------------------------------------
# 3. errors that need a context
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors(box):
    import torch
    pt, _ = box
    lib = plugin.load_library()
    texels, recv, irr, _ = cases.generated_list(7, 5, seed=2, bad=False, isolated=False)
    dt, dr, de = _upload(pt, texels, recv, irr)
    out = torch.full((len(texels), 4), SENTINEL_F, dtype=torch.float32, device=dt.device)
    torch.cuda.synchronize(dt.device)
    n = len(texels)

    def call(p, t=dt.data_ptr(), r=dr.data_ptr(), e=de.data_ptr(), count=n, w=7, h=5, o=out.data_ptr()):
        return lib.PTDenoiseLightmap(pt.ctx, None if p is None else C.byref(p), t, r, e, count, w, h, o)

    good = abi.lightmap_denoise_params(cases.SAMPLES)
    assert call(None) == abi.PT_ERR_INVALID_ARG and b"params == NULL" in lib.PTGetLastError()
    for kw, word in ((dict(samples=1), b"samples"), (dict(iterations=9), b"iterations"), (dict(normal_power=8), b"normalPower"),
                     (dict(sigma_luminance=0.0), b"sigmaLuminance"), (dict(sigma_position=float("nan")), b"sigmaPosition"),
                     (dict(sigma_plane=float("inf")), b"sigmaPlane")):
        assert call(plugin.lightmap_denoise_params(cases.SAMPLES, 5, kw)) == abi.PT_ERR_INVALID_ARG and word in lib.PTGetLastError(), kw
    p = abi.lightmap_denoise_params(cases.SAMPLES)
    p.reserved[0] = 1
    assert call(p) == abi.PT_ERR_INVALID_ARG and b"reserved" in lib.PTGetLastError()
    p = abi.lightmap_denoise_params(cases.SAMPLES)
    p.structSize = 40
    assert call(p) == abi.PT_ERR_INVALID_ARG and b"structSize" in lib.PTGetLastError()
    for w, h in ((0, 5), (8193, 5), (7, 0), (7, 8193)):
        assert call(good, w=w, h=h) == abi.PT_ERR_INVALID_ARG and b"8192" in lib.PTGetLastError()
    assert call(good, w=2, h=2) == abi.PT_ERR_INVALID_ARG and b"more entries" in lib.PTGetLastError()
    for name in ("t", "r", "e", "o"):
        assert call(good, **{name: None}) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.PTGetLastError(), name
    assert call(good, t=dt.data_ptr() + 2) == abi.PT_ERR_INVALID_ARG and b"misaligned" in lib.PTGetLastError()
    for name, ptr in (("r", dr.data_ptr()), ("e", de.data_ptr()), ("o", out.data_ptr())):
        assert call(good, **{name: ptr + 4}) == abi.PT_ERR_INVALID_ARG and b"misaligned" in lib.PTGetLastError(), name
    # an empty list is fine and launches nothing; so far nothing was written
    assert call(good, t=None, r=None, e=None, o=None, count=0) == abi.PT_OK
    pt.synchronize()
    assert (out == SENTINEL_F).all().item(), "a refused call wrote something"
    # no scene is needed, and the context still works
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(pt.device, C.byref(ctx)))
    try:
        assert lib.PTDenoiseLightmap(ctx, C.byref(good), dt.data_ptr(), dr.data_ptr(), de.data_ptr(), n, 7, 5, out.data_ptr()) == abi.PT_OK
        plugin.check(lib.PTSynchronize(ctx))
        first = out.cpu().numpy()
    finally:
        lib.PTDestroy(ctx)
    assert call(good) == abi.PT_OK
    pt.synchronize()
    want = plugin.denoise_lightmap(texels, recv, irr, 7, 5, cases.SAMPLES)
    _assert_rows(out.cpu().numpy(), want, "after the refusals")
    _assert_rows(first, want, "a context without a scene")
