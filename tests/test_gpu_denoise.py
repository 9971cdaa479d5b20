"""Guides and denoising (PTRenderGuides / PTDenoise, include/ptmi_plugin.h Part 4) on the MI355X.

The guides equal, bit for bit, what the ray queries (PTTraceRays with surface records) return for the same pinhole rays; the
albedo equals a numpy evaluation of the base colour times its bilinear texel.  The filter equals the float64 restatement of
tests/test_denoise.py.  Denoising lowers the error of a 4 spp frame against a 2048 spp one, and neither call changes what the
render computes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
from test_denoise import denoise_ref, random_guides

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRESS = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib", "libpt-stress-small-stacks.so")
MISS = np.uint32(0xFFFFFFFF)
f32 = np.float32

SCENES = {
    "cornell": lambda: scenes.cornell_box(),
    "zoo": lambda: scenes.material_zoo(),
    "instanced": lambda: scenes.instanced_scene(count=60, detail=8),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# the guide rays and the guide arithmetic, restated in float32
# ---------------------------------------------------------------------------------------------------------------------------
def _mul44(m, v):
    return [m[r] * v[0] + m[4 + r] * v[1] + m[8 + r] * v[2] + m[12 + r] * v[3] for r in range(4)]


def subpixel_rays(p, n):
    """(H, W, n*n, 8) float32: the rays of sample (i, j) (j-major) of every pixel, in the device's float32 operation order
    (PathTracer.camera_ray with the offset (i + 0.5) / n)."""
    W, H = p.OutputWidth, p.OutputHeight
    inv = np.array(p.CamInvProj[:], np.float32)
    c2w = np.array(p.CamToWorld[:], np.float32)
    o = _mul44(c2w, [f32(0), f32(0), f32(0), f32(1)])
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.zeros((H, W, n * n, 8), np.float32)
    for j in range(n):
        for i in range(n):
            pcx = xs.astype(np.float32) + f32((i + 0.5) / n)
            pcy = ys.astype(np.float32) + f32((j + 0.5) / n)
            uvx = pcx / f32(W) * f32(2.0) - f32(1.0)
            uvy = pcy / f32(H) * f32(2.0) - f32(1.0)
            zero, one = np.zeros_like(uvx), np.ones_like(uvx)
            d4 = _mul44(inv, [uvx, uvy, zero, one])
            w4 = _mul44(c2w, [d4[0], d4[1], d4[2], zero])
            inv_len = f32(1.0) / np.sqrt(w4[0] * w4[0] + w4[1] * w4[1] + w4[2] * w4[2])
            k = j * n + i
            rays[:, :, k, 0:3] = np.stack([o[0], o[1], o[2]], -1)
            rays[:, :, k, 3:6] = np.stack([w4[0] * inv_len, w4[1] * inv_len, w4[2] * inv_len], -1)
            rays[:, :, k, 6] = abi.PT_FAR_PLANE
    return rays


def _unorm8(b):
    return (b & 0xFF).astype(np.float64) / 255.0


def base_color(scene, mat, uv):
    """GetBaseColorOpacity's rgb for materials `mat` at uvs `uv` (float64 bilinear texel; the device's texel addressing)."""
    m = np.asarray(scene.materials, np.float32).reshape(-1, 8, 4)[mat]
    bc = m[:, 0, :3].astype(np.float64)
    tex = np.asarray(scene.texture_data, np.uint32)
    tidx = m[:, 5, 2]
    use = (tex.size > 0) & ~(tidx < 0)
    for k in np.nonzero(use)[0]:
        t = int(tidx[k])
        w, h, off = (int(v) for v in tex[t * 4: t * 4 + 3])
        tr = m[k, 7]
        u = f32(uv[k, 0] * tr[0] + tr[2])
        v = f32(uv[k, 1] * tr[1] + tr[3])

        def wrap(a):
            if abs(a) >= 16777216.0:
                return f32(0)
            if a > 1:
                return f32(a - (np.ceil(a) - f32(1)))
            if a < 0:
                return f32(a + np.ceil(-a))
            return a
        tu, tv = f32(wrap(u) * f32(w - 1.0)), f32(wrap(v) * f32(h - 1.0))
        tx, ty = int(tu), int(tv)
        uf, vf = float(tu - f32(tx)), float(tv - f32(ty))

        def px(x, y):
            x, y = min(x, w - 1), min(y, h - 1)
            p = tex[off + y * w + x]
            return np.array([_unorm8(p >> s) for s in (0, 8, 16)])
        top = px(tx, ty) + uf * (px(tx + 1, ty) - px(tx, ty))
        bot = px(tx, ty + 1) + uf * (px(tx + 1, ty + 1) - px(tx, ty + 1))
        bc[k] = (top + vf * (bot - top)) * bc[k]
    return bc


def guides_restated(pt, p, n):
    """The guides from ray queries over the sub-pixel rays, summed in float32 in sample order (the header's definition)."""
    H, W = p.OutputHeight, p.OutputWidth
    S = n * n
    rays = subpixel_rays(p, n)
    hits, surf = pt.trace_rays(rays.reshape(-1, 8), surface=True)
    hit = (_bits(hits[:, 3]) != MISS).reshape(H, W, S)
    surf = surf.reshape(H, W, S, 12)
    alb_s = np.ones((H * W * S, 3))
    hm = hit.reshape(-1)
    sf = surf.reshape(-1, 12)
    alb_s[hm] = base_color(pt.scene, sf[hm, 7].view(np.int32), sf[hm, 8:10])
    alb_s = alb_s.reshape(H, W, S, 3)
    alb_s = alb_s.astype(np.float32)
    albedo = np.zeros((H, W, 3), np.float32)
    for k in range(S):
        albedo = albedo + alb_s[:, :, k]
    albedo = albedo / f32(S)
    cnt = hit.sum(-1)
    nsum = np.zeros((H, W, 3), np.float32)
    dsum = np.zeros((H, W), np.float32)
    seen = np.zeros((H, W), bool)
    for k in range(S):
        h = hit[:, :, k]
        first = h & ~seen
        more = h & seen
        nsum[first] = surf[:, :, k, 4:7][first]
        dsum[first] = surf[:, :, k, 3][first]
        nsum[more] = nsum[more] + surf[:, :, k, 4:7][more]
        dsum[more] = dsum[more] + surf[:, :, k, 3][more]
        seen |= h
    nrm = nsum.copy()
    multi = cnt > 1
    dot = nsum[..., 0] * nsum[..., 0] + nsum[..., 1] * nsum[..., 1] + nsum[..., 2] * nsum[..., 2]
    inv = f32(1.0) / np.sqrt(np.where(dot > 0, dot, f32(1)))
    nrm[multi] = (nsum * inv[..., None])[multi]
    nrm[multi & ~(dot > 0)] = 0
    depth = np.where(cnt > 0, dsum / np.maximum(cnt, 1).astype(np.float32), f32(0)).astype(np.float32)
    cover = (cnt.astype(np.float32) / f32(S))
    return albedo, cover, nrm, depth, hit, surf


def _assert_within_ulp(a, b, ulp, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    same_sign = np.sign(a) == np.sign(b)
    bad = ~((a == b) | (same_sign & (d <= ulp)))
    assert not bad.any(), (what, int(bad.sum()), a[bad][:5], b[bad][:5])


# ---------------------------------------------------------------------------------------------------------------------------
# 1: guides against ray queries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_guides_match_ray_queries(name):
    W, H = 203, 117                                                     # not multiples of 8
    pt = PathTracer(SCENES[name](), width=W, height=H)
    try:
        p = pt.params(seed=0)
        # S = 1: the guide rays are camera_ray's, bit for bit, and the guides are the surface records
        ref = subpixel_rays(p, 1)
        for x, y in ((0, 0), (202, 116), (101, 58), (37, 99)):
            assert (_bits(ref[y, x, 0]) == _bits(pt.camera_ray(x, y, p))).all(), (x, y)
        for n in (1, 2, 4):
            pt.render_guides(samples=n * n, params=p)
            alb, nd = pt.guides()
            albedo, cover, nrm, depth, hit, surf = guides_restated(pt, p, n)
            assert alb.shape == (H, W, 4) and nd.shape == (H, W, 4)
            assert (alb[..., 3] == cover).all(), n
            assert np.abs(alb[..., :3] - albedo).max() <= 1e-6, (n, np.abs(alb[..., :3] - albedo).max())
            if n == 1:
                h = hit[..., 0]
                assert (alb[~h] == np.array([1, 1, 1, 0], np.float32)).all()
                assert (_bits(nd[~h]) == 0).all()
                assert (_bits(nd[h][:, :3]) == _bits(surf[..., 0, 4:7][h])).all()        # PTRaySurface.normal
                assert (_bits(nd[h][:, 3]) == _bits(surf[..., 0, 3][h])).all()           # PTRaySurface.t
            else:
                _assert_within_ulp(nd[..., :3], nrm, 1, f"normal S={n * n}")
                _assert_within_ulp(nd[..., 3], depth, 1, f"depth S={n * n}")
            print(f"[guides] {name} S={n * n}: coverage {float(alb[..., 3].mean()):.3f}")
        assert hit.any()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the filter against the numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _upload_guides(pt, albedo, nd):
    for which, a in ((0, albedo), (1, nd)):
        a = np.ascontiguousarray(a, np.float32)
        plugin.hip_memcpy(pt.guide_pointer(which), a.ctypes.data, a.nbytes, plugin.HIP_MEMCPY_H2D)


def _check(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref) / (1.0 + np.abs(ref))
    assert err.max() <= 1e-4, (what, float(err.max()), np.unravel_index(int(err.argmax()), err.shape))


@pytest.mark.parametrize("size", [(67, 45), (257, 131)])
def test_filter_matches_restatement(size):
    import torch
    W, H = size
    rng = np.random.RandomState(W)
    pt = PathTracer(scenes.cornell_box(), width=W, height=H)
    try:
        pt.render_guides(1)
        albedo, nd = random_guides(H, W, rng)
        _upload_guides(pt, albedo, nd)
        color = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
        d_src = torch.from_numpy(color).to("cuda:0")
        torch.cuda.synchronize()
        for demod in (True, False):
            for it in range(1, 7):
                dp = abi.denoise_params(iterations=it, demodulate=demod)
                got = pt.denoise(dp, d_src=d_src.data_ptr())
                ref = denoise_ref(color, albedo, nd, it, demodulate=demod)
                _check(got, ref, (size, demod, it))
                bg = albedo[..., 3] == 0
                assert (_bits(got[bg]) == _bits(color[bg])).all()
                assert (_bits(got[..., 3]) == _bits(color[..., 3])).all()
        # the input is never written; iterations = 0 returns its bits
        assert (_bits(d_src.cpu().numpy()) == _bits(color)).all()
        got = pt.denoise(abi.denoise_params(iterations=0), d_src=d_src.data_ptr())
        assert (_bits(got) == _bits(color)).all()
        # in place
        d_io = d_src.clone()
        torch.cuda.synchronize()
        pt.denoise(abi.denoise_params(iterations=3), d_src=d_io.data_ptr(), d_dst=d_io.data_ptr())
        pt.synchronize()
        _check(d_io.cpu().numpy(), denoise_ref(color, albedo, nd, 3), "in place")
    finally:
        pt.close()


def test_denoise_reads_the_output_frame():
    W, H = 67, 45
    pt = PathTracer(scenes.material_zoo(), width=W, height=H, samplesPerPass=2)
    try:
        p = pt.params(seed=7)
        pt.render_pass(p)
        pt.render_guides(4, p)
        frame = pt.readback(last_output=False)
        alb, nd = pt.guides()
        got = pt.denoise()                                               # PTDenoiseToHost: dSrc = NULL
        _check(got, denoise_ref(frame, alb, nd, 5), "output frame")
        got2 = pt.denoise(d_src=pt.frame_pointer(-1))
        assert (_bits(got) == _bits(got2)).all()
        assert (_bits(pt.readback(last_output=False)) == _bits(frame)).all()      # the Output frame is not modified
        # errors: guides of another size than the frame, bad arguments
        pt.render_guides(1, scenes.frame_params(pt.scene, W + 1, H, seed=0))
        out = np.empty((H, W + 1, 4), np.float32)
        rc = pt.lib.PTDenoiseToHost(pt.ctx, abi.denoise_params(), out.ctypes.data, out.size)
        assert rc == abi.PT_ERR_INVALID_ARG and b"guides" in pt.lib.PTGetLastError()
        for bad in (abi.denoise_params(iterations=9), abi.denoise_params(iterations=-1), abi.denoise_params(sigma_luminance=0.0),
                    abi.denoise_params(sigma_normal=float("nan")), abi.denoise_params(sigma_depth=-1.0)):
            assert pt.lib.PTDenoise(pt.ctx, bad, None, pt.frame_pointer(0)) == abi.PT_ERR_INVALID_ARG
        bad = abi.denoise_params()
        bad.flags = 2
        assert pt.lib.PTDenoise(pt.ctx, bad, None, pt.frame_pointer(0)) == abi.PT_ERR_INVALID_ARG
        for s in (0, 2, 9, 64):
            assert pt.lib.PTRenderGuides(pt.ctx, p, s) == abi.PT_ERR_INVALID_ARG
    finally:
        pt.close()
    import ctypes as C
    lib = plugin.load_library()
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    dummy = (C.c_float * 16)()
    try:
        assert lib.PTRenderGuides(ctx, p, 1) == abi.PT_ERR_NO_SCENE
        assert lib.PTDenoise(ctx, abi.denoise_params(), None, C.addressof(dummy)) == abi.PT_ERR_INVALID_ARG
        assert b"no guides" in lib.PTGetLastError()
        assert lib.PTGetGuidePointer(ctx, 0) is None                    # nothing allocated before first use
    finally:
        lib.PTDestroy(ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: quality against a converged render
# ---------------------------------------------------------------------------------------------------------------------------
def _converged(scene, seed):
    """2048 spp: 32 accumulated passes of 64."""
    pt = PathTracer(scene, width=128, height=128, samplesPerPass=64)
    for k in range(32):
        pt.OnRenderImage(seed + k)
    pt.synchronize()
    ref = pt.readback()
    pt.close()
    return ref


def test_denoising_improves_a_noisy_frame():
    ratios = {}
    for name in ("cornell", "zoo"):
        s = SCENES[name]()
        ref = _converged(s, 1000)
        pt = PathTracer(s, width=128, height=128, samplesPerPass=4)
        try:
            pt.render_pass(pt.params(seed=77))                           # one 4 spp pass into the current Output frame
            noisy = pt.readback(last_output=False)
            pt.render_guides(4)
            den = pt.denoise(abi.denoise_params())
            den_plain = pt.denoise(abi.denoise_params(demodulate=False))
        finally:
            pt.close()

        def mse(a):
            t = lambda x: np.maximum(x[..., :3].astype(np.float64), 0) / (1 + np.maximum(x[..., :3].astype(np.float64), 0))
            return float(np.mean((t(a) - t(ref)) ** 2))
        m_noisy, m_den, m_plain = mse(noisy), mse(den), mse(den_plain)
        ratios[name] = (m_den / m_noisy, m_plain / m_noisy)
        print(f"[quality] {name}: MSE noisy {m_noisy:.3e}, denoised {m_den:.3e} ({m_den / m_noisy:.3f}x), "
              f"not demodulated {m_plain:.3e} ({m_plain / m_noisy:.3f}x)")
        assert m_den <= 0.5 * m_noisy, (name, m_den, m_noisy)
        if name == "zoo":
            assert m_den <= m_plain, (m_den, m_plain)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: no effect on rendering
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_no_effect_on_rendering(name):
    s = SCENES[name]()
    W, H = 64, 48
    frames, stats = [], []
    for interleave in (True, False):
        pt = PathTracer(s, width=W, height=H, samplesPerPass=2)
        pt.set_stats_level(1)
        try:
            for k in range(4):
                pt.OnRenderImage(0xBEEF + k)
                if interleave:
                    pt.render_guides(1 + 3 * (k % 2))
                    before = pt.readback(last_output=False)                 # the frame PTDenoise reads (dSrc = NULL)
                    pt.denoise()
                    assert (_bits(pt.readback(last_output=False)) == _bits(before)).all()
            pt.synchronize()
            frames.append(pt.readback())
            st = pt.stats()
            stats.append(bytes(st))
        finally:
            pt.close()
    assert (_bits(frames[0]) == _bits(frames[1])).all()
    assert stats[0] == stats[1]


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the small-stack build
# ---------------------------------------------------------------------------------------------------------------------------
GUIDE_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from unity_webgpu_pathtracer_amd import scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer
out = {}
for name, s in (("sponza", scenes.sponza_atrium(tex_size=8, detail=0.15)), ("tlas", scenes.instanced_scene(count=60, detail=8))):
    pt = PathTracer(s, width=97, height=61)
    for n in (1, 4):
        pt.render_guides(n)
        a, nd = pt.guides()
        out[f"{name}_{n}_albedo"], out[f"{name}_{n}_nd"] = a, nd
    pt.close()
np.savez(sys.argv[2], **out)
'''


def test_small_stack_build_gives_the_same_guides(tmp_path):
    if not os.path.exists(STRESS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc"), "stress"], stdout=subprocess.DEVNULL)
    res = {}
    for tag, env in (("default", {}), ("stress", {"PT_PLUGIN": STRESS})):
        out = os.path.join(tmp_path, f"{tag}.npz")
        subprocess.check_call([sys.executable, "-c", GUIDE_CHILD, ROOT, out], env=dict(os.environ, **env), timeout=600)
        res[tag] = np.load(out)
    for k in res["default"].files:
        assert res["default"][k].tobytes() == res["stress"][k].tobytes(), k
    assert (res["default"]["sponza_1_albedo"][..., 3] > 0).any()
