"""Per-pixel variance across passes (include/ptmi_plugin.h Part 6) without a GPU: exports, struct layout, argument checks,
kernel resources, and the numpy restatements -- the float32 moment update and noise statistics, bit for bit what the kernels
compute, and the float64 filter with a variance input.  tests/test_gpu_moments.py holds the GPU kernels to
these restatements."""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
import test_denoise
from kernel_resources import resources
from test_denoise import H5, K3, _lum, _shift, random_guides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENTS_SYMBOLS = ["PTAccumulateMoments", "PTAccumulateMomentsTo", "PTGetMomentsInfo", "PTGetMomentsPointer", "PTMeasureNoise",
                   "PTGetNoiseTilePointer", "PTDenoiseMoments", "PTDenoiseMomentsToHost"]
f32 = np.float32
WR, WG, WB = f32(0.2126), f32(0.7152), f32(0.0722)


# ---------------------------------------------------------------------------------------------------------------------------
# the update and the statistics, restated in numpy float32 (one IEEE operation per numpy operation, the header's order)
# ---------------------------------------------------------------------------------------------------------------------------
def lum32(rgb):
    rgb = np.asarray(rgb, np.float32)
    return WR * rgb[..., 0] + WG * rgb[..., 1] + WB * rgb[..., 2]


def moments_update(plane0, plane1, out, acc, n, m):
    """One observation: (plane0, plane1) after the passes that took the running mean from `acc` (n samples) to `out` (n + m)."""
    out = np.asarray(out, np.float32)
    if n == 0:
        return np.zeros(out.shape[:-1] + (4,), np.float32), np.zeros(out.shape[:-1] + (4,), np.float32)
    f = f32(float(n) * float(n + m) / float(m))
    d = out[..., :3] - np.asarray(acc, np.float32)[..., :3]
    dr, dg, db = d[..., 0], d[..., 1], d[..., 2]
    dl = lum32(d)
    p0, p1 = plane0.copy(), plane1.copy()
    p0[..., 0] += (dr * dr) * f
    p0[..., 1] += (dg * dg) * f
    p0[..., 2] += (db * db) * f
    p0[..., 3] += (dl * dl) * f
    p1[..., 0] += (dr * dg) * f
    p1[..., 1] += (dr * db) * f
    p1[..., 2] += (dg * db) * f
    p1[..., 3] = 0
    return p0, p1


def inv_dof(k, samples):
    return f32(1.0 / (float(k - 1) * float(samples)))


def bin_edge(b):
    """Upper edge of histogram bin b (+inf for the last)."""
    if b >= 255:
        return f32(np.inf)
    return np.array([(b + 1 + ((127 - 24) << 3)) << 20], np.uint32).view(np.float32)[0]


def noise_ref(frame, sll, k, samples, rel_floor=0.01, threshold=0.02, percentile=0.95, rank=0, world=1):
    """PTMeasureNoise restated: eps and its bins in float32 / integers exactly as the kernel computes them, the sums in float64."""
    frame = np.asarray(frame, np.float32)
    H, W = frame.shape[:2]
    with np.errstate(all="ignore"):
        eps = np.sqrt(np.asarray(sll, np.float32) * inv_dof(k, samples)) / (lum32(frame) + f32(rel_floor))
    eps = np.where(eps >= 0, eps, f32(np.inf)).astype(np.float32)
    bits = eps.view(np.uint32) & np.uint32(0x7FFFFFFF)
    eps = bits.view(np.float32)
    bins = np.clip((bits >> 20).astype(np.int64) - ((127 - 24) << 3), 0, 255)
    by, bx = np.mgrid[0:H, 0:W] // 16
    owned = (bx + by) % world == rank
    hist = np.bincount(bins[owned], minlength=256).astype(np.uint32)
    pixels = int(owned.sum())
    th, tw = (H + 15) // 16, (W + 15) // 16
    tiles = np.zeros((th, tw))
    with np.errstate(all="ignore"):
        for ty in range(th):
            for tx in range(tw):
                if (tx + ty) % world == rank:
                    tiles[ty, tx] = eps[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].astype(np.float64).mean()
        mean = float(eps[owned].astype(np.float64).mean()) if pixels else 0.0
    edge = f32(0)
    if pixels:
        target = math.ceil(float(f32(percentile)) * pixels)
        b = int(np.argmax(np.cumsum(hist.astype(np.int64)) >= target))
        edge = bin_edge(b)
    return {"eps": eps, "bins": bins, "histogram": hist, "pixels": pixels, "pixelsBelow": int((eps[owned] <= f32(threshold)).sum()),
            "maxBits": int(bits[owned].max()) if pixels else 0, "mean": mean, "tiles": tiles, "percentileError": edge}


def moments_variance(plane0, plane1, albedo, k, samples, demodulate):
    """The v PTDenoiseMoments' prepass uses at covered pixels, in float64."""
    idof = float(inv_dof(k, samples))
    p0, p1 = plane0.astype(np.float64), plane1.astype(np.float64)
    if not demodulate:
        return np.maximum(p0[..., 3] * idof, 0.0)
    q = np.array([0.2126, 0.7152, 0.0722]) / np.maximum(albedo[..., :3].astype(np.float64), 1e-3)
    qr, qg, qb = q[..., 0], q[..., 1], q[..., 2]
    diag = qr * qr * p0[..., 0] + qg * qg * p0[..., 1] + qb * qb * p0[..., 2]
    cross = qr * qg * p1[..., 0] + qr * qb * p1[..., 1] + qg * qb * p1[..., 2]
    return np.maximum((diag + 2.0 * cross) * idof, 0.0)


def denoise_ref(color, albedo, normal_depth, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0, demodulate=True, variance=None):
    """tests/test_denoise.py's float64 a-trous filter with one more input: `variance` (H, W) replaces the prepass's 3x3 spatial
    luminance variance at covered pixels (PTDenoiseMoments); None = PTDenoise."""
    c = color.astype(np.float64)
    if iterations == 0:
        return c.copy()
    a = albedo.astype(np.float64)
    g = normal_depth.astype(np.float64)
    cov = a[..., 3] > 0
    amax = np.maximum(a[..., :3], 1e-3)
    e = c[..., :3] / amax if demodulate else c[..., :3].copy()
    l = _lum(e)
    if variance is None:
        lq = [(_shift(l, dx, dy)[0], _shift(cov, dx, dy, False)[0]) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        cnt = np.maximum(sum(m.astype(np.float64) for _, m in lq), 1)
        mean = sum(np.where(m, v, 0.0) for v, m in lq) / cnt
        var = np.maximum(sum(np.where(m, (v - mean) ** 2, 0.0) for v, m in lq) / cnt, 0.0)
    else:
        var = np.asarray(variance, np.float64)
    z = g[..., 3]
    grad = []
    for dx, dy in ((1, 0), (0, 1)):
        zp, cp = _shift(z, dx, dy)[0], _shift(cov, dx, dy, False)[0]
        zm, cm = _shift(z, -dx, -dy)[0], _shift(cov, -dx, -dy, False)[0]
        grad.append(np.where(cm & cp, (zp - zm) * 0.5, np.where(cp, zp - z, np.where(cm, z - zm, 0.0))))
    gx, gy = grad
    n = g[..., :3]
    v = var
    for k in range(iterations):
        s = 1 << k
        vw = np.zeros_like(v)
        vs = np.zeros_like(v)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, _ = _shift(v, dx, dy)
                cq = _shift(cov, dx, dy, False)[0]
                wk = K3[dx + 1] * K3[dy + 1] * cq
                vw += wk
                vs += wk * vq
        gv = np.maximum(vs / np.maximum(vw, 1e-300), 0.0)
        den_l = sigma_l * np.sqrt(gv) + 1e-6
        sw = np.zeros_like(v)
        sv = np.zeros_like(v)
        se = np.zeros_like(e)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                eq, _ = _shift(e, s * dx, s * dy)
                vq, _ = _shift(v, s * dx, s * dy)
                nq, _ = _shift(n, s * dx, s * dy)
                zq, _ = _shift(z, s * dx, s * dy)
                cq = _shift(cov, s * dx, s * dy, False)[0]
                wl = np.exp(-np.abs(l - _lum(eq)) / den_l)
                wn = np.maximum(0.0, np.sum(n * nq, axis=-1)) ** sigma_n
                dz = np.abs(gx * (s * dx) + gy * (s * dy))
                wz = np.exp(-np.abs(z - zq) / (sigma_z * dz + 1e-3 * z + 1e-6))
                w = H5[dx + 2] * H5[dy + 2] * wl * wn * wz * cq
                sw += w
                sv += w * w * vq
                se += w[..., None] * eq
        ok = cov & (sw > 0)
        swd = np.where(ok, sw, 1.0)
        e = np.where(ok[..., None], se / swd[..., None], e)
        v = np.where(ok, sv / (swd * swd), v)
        l = _lum(e)
    out = c.copy()
    rgb = e * amax if demodulate else e
    out[..., :3] = np.where(cov[..., None], rgb, c[..., :3])
    return out


def resolve32(color_sum, acc, n, m):
    """The resolve's running mean in float32 (PathTracer.compute:89-98): (sum + acc * n) / (n + m); sum / m for the first pass."""
    color_sum = np.asarray(color_sum, np.float32)
    if n == 0:
        return color_sum / f32(m)
    return (color_sum + acc * f32(n)) / (f32(n) + f32(m))


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_moments_symbols_are_exported():
    plugin.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", plugin.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "ptmi_plugin.h")).read()
    for name in MOMENTS_SYMBOLS:
        assert name in exported, name
        assert name in plugin.EXPORTED_SYMBOLS, name
        assert f" {name}(" in header, name
    assert plugin.load_library().PTGetVersion() == (0 << 16) | 2


def test_noise_structs_match_c_header():
    fields = {"PTNoiseParams": ["structSize", "relFloor", "threshold", "percentile"],
              "PTNoiseStats": ["structSize", "observations", "samples", "pixels", "pixelsBelow", "meanError", "maxError",
                               "percentileError", "_pad", "histogram"]}
    lines = []
    for t, fs in fields.items():
        lines.append(f'printf("{t} %zu\\n", sizeof({t}));')
        lines += [f'printf("{t}.{f} %zu\\n", offsetof({t}, {f}));' for f in fs]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ptmi_plugin.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "probe.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(l.split(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["PTNoiseParams"]) == C.sizeof(abi.PTNoiseParams) == 16
    assert int(got["PTNoiseStats"]) == C.sizeof(abi.PTNoiseStats) == 1072
    for t, fs in fields.items():
        for f in fs:
            assert int(got[f"{t}.{f}"]) == getattr(getattr(abi, t), f).offset, (t, f)
    q = abi.noise_params()
    assert (q.structSize, q.relFloor, q.threshold, q.percentile) == (16, f32(0.01), f32(0.02), f32(0.95))
    assert abi.noise_stats().structSize == 1072


def test_moments_argument_errors_without_context():
    lib = plugin.load_library()
    p = abi.PTFrameParams()
    dp = abi.denoise_params()
    q, st = abi.noise_params(), abi.noise_stats()
    buf = (C.c_float * 16)()
    k, n = C.c_uint32(), C.c_uint64()
    for rc in (lib.PTAccumulateMoments(None, C.byref(p), 1),
               lib.PTAccumulateMomentsTo(None, C.byref(p), 1, C.addressof(buf), C.addressof(buf)),
               lib.PTGetMomentsInfo(None, C.byref(k), C.byref(n), None, None),
               lib.PTMeasureNoise(None, C.byref(q), None, C.byref(st)),
               lib.PTDenoiseMoments(None, C.byref(dp), None, C.addressof(buf)),
               lib.PTDenoiseMomentsToHost(None, C.byref(dp), C.addressof(buf), 16)):
        assert rc == abi.PT_ERR_INVALID_ARG
        assert b"ctx == NULL" in lib.PTGetLastError()
    assert lib.PTGetMomentsPointer(None, 0) is None
    assert lib.PTGetNoiseTilePointer(None) is None


# ---------------------------------------------------------------------------------------------------------------------------
# the update against the definition
# ---------------------------------------------------------------------------------------------------------------------------
def test_update_matches_the_definition():
    """20,000 synthetic pixels, 32 observations of 4 samples, Gaussian with known sigma, frames chained through the resolve's
    float32 formula.  Sll from the float32 update must agree with the float64 evaluation of the same sum from the same frames to
    (k + 4) * 2^-24 relative (a sum of k non-negative terms, each a handful of roundings: relative errors do not amplify), and
    S_ll / ((k - 1) sigma_l^2) -- sigma_l^2 the variance of ONE sample's luminance -- must average to 1 within 1 % (standard
    deviation of that mean: sqrt(2 / (k - 1) / P) = 0.18 %)."""
    P, K, m = 20000, 32, 4
    rng = np.random.RandomState(5)
    mu = rng.uniform(0.2, 2.0, (P, 3))
    sigma = 0.3                                                         # per channel, per sample, independent channels
    p0 = p1 = None
    acc = None
    s64 = np.zeros(P)
    n = 0
    for k in range(K):
        pass_mean = mu + rng.normal(0.0, sigma / math.sqrt(m), (P, 3))
        color_sum = (pass_mean * m).astype(np.float32)
        out = np.concatenate([resolve32(color_sum, None if acc is None else acc[:, :3], n, m), np.ones((P, 1), np.float32)], -1)
        p0, p1 = moments_update(p0, p1, out, acc, n, m)
        if n > 0:
            d = out[:, :3].astype(np.float64) - acc[:, :3].astype(np.float64)
            dl = 0.2126 * d[:, 0] + 0.7152 * d[:, 1] + 0.0722 * d[:, 2]
            s64 += dl * dl * (n * (n + m) / m)
        acc, n = out, n + m
    assert p0.dtype == np.float32 and (p1[:, 3] == 0).all()
    rel = np.abs(p0[:, 3].astype(np.float64) - s64) / s64
    print(f"[moments] Sll float32 against float64: max relative difference {rel.max():.2e} (bound {(K + 4) * 2.0 ** -24:.2e})")
    assert rel.max() <= (K + 4) * 2.0 ** -24
    var_l = (0.2126 ** 2 + 0.7152 ** 2 + 0.0722 ** 2) * sigma ** 2
    ratio = float(np.mean(p0[:, 3].astype(np.float64) / ((K - 1) * var_l)))
    print(f"[moments] mean of Sll / ((k - 1) sigma^2) = {ratio:.4f}")
    assert abs(ratio - 1.0) <= 0.01
    # the covariance plane: Srg / sqrt(Srr Sgg) of independent channels averages to 0, Srr to the channel variance
    assert abs(float(np.mean(p0[:, 0].astype(np.float64) / ((K - 1) * sigma ** 2))) - 1.0) <= 0.01
    assert abs(float(np.mean(p1[:, 0].astype(np.float64) / ((K - 1) * sigma ** 2)))) <= 0.01


def test_estimate_matches_true_error_with_the_oracle():
    """Cornell box 48x48 through the CPU oracle: 16 tracked passes of 4 spp against a 2048 spp reference.  The summed true
    squared luminance error over the summed predicted variance of the mean must lie in [0.5, 2]: the geometric middle between 1
    and the smallest mistake this is meant to catch (a dropped factor m = 4; W would be 64)."""
    from oracle import pyoracle
    from unity_webgpu_pathtracer_amd.pathtracer import BVHScene
    s = scenes.cornell_box()
    b = pyoracle.buffers_from_bvhscene(BVHScene(s))

    def run(passes, spp, seed0, track):
        acc, n, p0, p1 = None, 0, None, None
        for k in range(passes):
            p = scenes.frame_params(s, 48, 48, spp=spp, current_sample=n, seed=seed0 + k)
            out, _ = pyoracle.render(b, p, accumulated=acc)
            if track:
                p0, p1 = moments_update(p0, p1, out, acc, n, spp)
            acc, n = out, n + spp
        return acc, p0, n
    out, p0, n = run(16, 4, 77, True)
    ref, _, _ = run(32, 64, 1000, False)
    err = (lum32(out[..., :3]).astype(np.float64) - lum32(ref[..., :3]).astype(np.float64)) ** 2
    pred = p0[..., 3].astype(np.float64) * float(inv_dof(16, n))
    ratio = float(err.sum() / pred.sum())
    print(f"[moments] oracle, Cornell 48x48, 16 x 4 spp against 2048 spp: true / predicted squared error = {ratio:.3f}")
    assert 0.5 <= ratio <= 2.0, ratio


# ---------------------------------------------------------------------------------------------------------------------------
# the statistics restatement's own edges, and the filter restatement against tests/test_denoise.py's
# ---------------------------------------------------------------------------------------------------------------------------
def test_bins_and_edges():
    frame = np.zeros((1, 6, 4), np.float32)
    frame[..., :3] = 1.0
    frame[0, 4, :3] = np.nan                                            # NaN pixel -> +inf -> bin 255
    frame[0, 5, :3] = 0.0                                               # black pixel: the floor alone is the denominator
    sll = np.array([[0.0, 1e30, 1.0, 2.0 ** -60, 1.0, 1.0]], np.float32)
    r = noise_ref(frame, sll, 2, 1, rel_floor=0.01)
    assert list(r["bins"][0, :2]) == [0, 255] and r["bins"][0, 3] == 0 and r["bins"][0, 4] == 255
    assert r["bins"][0, 2] == (int(np.array([1 / 1.01], np.float32).view(np.uint32)[0]) >> 20) - 824
    assert r["bins"][0, 5] == (int(np.array([100.0], np.float32).view(np.uint32)[0]) >> 20) - 824
    assert bin_edge(0) == f32(2.0 ** -24 * 1.125) and bin_edge(254) == f32(240.0) and np.isinf(bin_edge(255))
    assert r["pixels"] == 6 and r["histogram"].sum() == 6 and np.isinf(r["percentileError"])


def test_filter_restatement_with_no_variance_is_test_denoise():
    rng = np.random.RandomState(9)
    albedo, nd = random_guides(29, 37, rng)
    color = rng.uniform(0, 2, (29, 37, 4)).astype(np.float32)
    for demod in (True, False):
        a = denoise_ref(color, albedo, nd, 4, demodulate=demod, variance=None)
        assert (a == test_denoise.denoise_ref(color, albedo, nd, 4, demodulate=demod)).all()
    # and the variance input is used: zero variance with distinct luminances leaves covered pixels alone
    out = denoise_ref(color, albedo, nd, 3, demodulate=False, variance=np.zeros((29, 37)))
    assert np.abs(out - color).max() <= 1e-3 < np.abs(a - color).max()


# ---------------------------------------------------------------------------------------------------------------------------
# kernel resources
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_moments_kernel_resources():
    res = resources("pt_moments.hip")
    for name in ("pt_moments_accumulate", "pt_noise_blocks", "pt_noise_finish"):
        r = res[name]
        print(f"[resources] {name}: {r}")
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    assert res["pt_noise_blocks"]["lds"] <= 2048, res["pt_noise_blocks"]
    assert res["pt_moments_accumulate"]["lds"] == 0
    r = resources("pt_denoise.hip")["pt_denoise_prepass_moments"]
    print(f"[resources] pt_denoise_prepass_moments: {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, r
