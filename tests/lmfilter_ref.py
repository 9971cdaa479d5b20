"""The lightmap denoiser's rule (include/ptmi_plugin.h Part 17) restated in numpy from the header comment of csrc/lmfilter_rule.h:
every operation is one float32 operation in the order the text gives, whole images at a time (a tap is a shifted image, and the
sums run over the taps in the text's order, so every texel sees the sequential sums the rule asks for)."""
import numpy as np

F = np.float32
GOOD, BAD = 1, 2


def luminance(e):
    return (e[..., 0] * F(0.299) + e[..., 1] * F(0.587)) + e[..., 2] * F(0.114)


def entry_variance(rgb, m2, samples):
    """step 1: the variance of the mean luminance behind every entry"""
    S = F(samples)
    l = luminance(rgb)
    with np.errstate(all="ignore"):
        return np.fmax((m2 - (S * l) * l) / (S - F(1.0)), F(0.0)) / S


def _shift(img, ox, oy):
    """out[y, x] = img[y + oy, x + ox] where that lies inside the image; inside tells where"""
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    inside = np.zeros((h, w), bool)
    x0, x1 = max(0, -ox), min(w, w - ox)
    y0, y1 = max(0, -oy), min(h, h - oy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = img[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return out, inside


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def denoise(texels, recv, irr, width, height, samples, iterations=5, sigma_luminance=4.0, sigma_position=4.0, sigma_plane=1.0, normal_power=5,
            details=False):
    """(n, 4) float32 rows: what PTDenoiseLightmap writes.  details: also the images (flags, h2) for the tests' own statements."""
    texels = np.asarray(texels, np.int64).reshape(-1)
    recv = np.ascontiguousarray(recv, F).reshape(-1, 8)
    irr = np.ascontiguousarray(irr, F).reshape(-1, 4)
    w, h = int(width), int(height)
    assert len(np.unique(texels)) == len(texels) and (len(texels) == 0 or texels.max() < w * h)
    # ---- 1. texel state
    v = entry_variance(irr[:, :3], irr[:, 3], samples)
    bad = ~(np.isfinite(irr).all(axis=1) & np.isfinite(recv[:, 0:3]).all(axis=1) & np.isfinite(recv[:, 4:7]).all(axis=1)) | np.isnan(v)
    flags = np.zeros(w * h, np.uint8)
    E, V, P, N = np.zeros((w * h, 3), F), np.zeros(w * h, F), np.zeros((w * h, 3), F), np.zeros((w * h, 3), F)
    flags[texels] = np.where(bad, BAD, GOOD)
    E[texels], V[texels], P[texels], N[texels] = irr[:, :3], v, recv[:, 0:3], recv[:, 4:7]
    flags, E, V, P, N = flags.reshape(h, w), E.reshape(h, w, 3), V.reshape(h, w), P.reshape(h, w, 3), N.reshape(h, w, 3)
    good = flags == GOOD
    # bad texels are never read below; their garbage must not raise warnings either
    E, V, P, N = (np.where(good[..., None] if a.ndim == 3 else good, a, F(0.0)) for a in (E, V, P, N))

    def dist2(Pq):
        d = Pq - P
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    with np.errstate(all="ignore"):
        # ---- 2. footprint
        h2 = np.zeros((h, w), F)
        for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            Pq, inside = _shift(P, ox, oy)
            gq, _ = _shift(good, ox, oy)
            d2 = dist2(Pq)
            take = good & inside & gq & (d2 > 0) & ((h2 == 0) | (d2 < h2))
            h2 = np.where(take, d2, h2)
        active = good & (h2 != 0)
        sp2 = F(sigma_position) * F(sigma_position)

        def tap(ox, oy):
            """the admitted texels of this offset and the tap's images (step 3)"""
            gq, inside = _shift(good, ox, oy)
            Pq = _shift(P, ox, oy)[0]
            adm = inside & gq
            if (ox, oy) != (0, 0):
                adm = adm & (dist2(Pq) <= (sp2 * h2) * F(ox * ox + oy * oy))
            return adm, Pq

        # ---- 4. the levels
        b3 = {-1: F(0.25), 0: F(0.5), 1: F(0.25)}
        h5 = {-2: F(0.0625), -1: F(0.25), 0: F(0.375), 1: F(0.25), 2: F(0.0625)}
        for k in range(int(iterations)):
            s = 1 << k
            gw, gv = np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    adm, _ = tap(dx, dy)
                    c = b3[dx] * b3[dy]
                    Vq = _shift(V, dx, dy)[0]
                    gw = np.where(adm, gw + c, gw)
                    gv = np.where(adm, gv + c * Vq, gv)
            g = gv / gw
            lp = luminance(E)
            zden = (F(sigma_plane) * np.sqrt(h2)) * F(s) + F(1e-12)
            xden = F(sigma_luminance) * np.sqrt(g) + F(1e-6)
            sw, sv, se = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 3), F)
            for dy in (-2, -1, 0, 1, 2):
                for dx in (-2, -1, 0, 1, 2):
                    ox, oy = dx * s, dy * s
                    adm, Pq = tap(ox, oy)
                    if not adm.any():
                        continue
                    Eq, Vq, Nq = _shift(E, ox, oy)[0], _shift(V, ox, oy)[0], _shift(N, ox, oy)[0]
                    wn = np.fmax(_dot(N, Nq), F(0.0))
                    for _ in range(int(normal_power)):
                        wn = wn * wn
                    z = np.abs(_dot(N, Pq - P)) / zden
                    rz = F(1.0) / (F(1.0) + z * z)
                    wz = rz * rz
                    xl = np.abs(lp - luminance(Eq)) / xden
                    rl = F(1.0) / (F(1.0) + xl * xl)
                    wl = rl * rl
                    wt = (((h5[dx] * h5[dy]) * wn) * wz) * wl
                    sw = np.where(adm, sw + wt, sw)
                    se = np.where(adm[..., None], se + wt[..., None] * Eq, se)
                    sv = np.where(adm, sv + (wt * wt) * Vq, sv)
            new = active & (sw > 0)
            E = np.where(new[..., None], se / sw[..., None], E)
            V = np.where(new, sv / (sw * sw), V)
    # ---- 5. output
    out = irr.copy()
    keep = ~bad
    out[keep, :3] = E.reshape(-1, 3)[texels[keep]]
    out[keep, 3] = V.reshape(-1)[texels[keep]]
    assert out.dtype == F
    if details:
        return out, {"flags": flags, "h2": h2, "active": active}
    return out
