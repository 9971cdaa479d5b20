"""The probe-volume rule (include/ptmi_plugin.h Part 16) restated in numpy float32, for tests/test_probe_volume.py and
tests/test_gpu_probe_volume.py: the octahedral texel directions, a texel's sequential sums and its moments, the grid cell of a
point, the corner weights and the blend.  Written from the header's text, not from volume_rule.h; every operation is one float32
operation in the rule's order.  Sample directions and E(N) are Part 15's (plugin.probe_directions, probe_ref.irradiance)."""
import numpy as np

import probe_ref

F = np.float32
U = np.uint32
WRAP, VISIBILITY = 1, 2


def _sgn(x):
    return np.where(x < F(0.0), F(-1.0), F(1.0)).astype(F)


def texel_directions():
    """(64, 3) float32: d_l of texel l = v * 8 + u"""
    l = np.arange(64)
    u, v = (l % 8).astype(F), (l // 8).astype(F)
    a = (u + F(0.5)) * F(0.25) - F(1.0)
    b = (v + F(0.5)) * F(0.25) - F(1.0)
    z = (F(1.0) - np.abs(a)) - np.abs(b)
    x = np.where(z < 0, (F(1.0) - np.abs(b)) * _sgn(a), a).astype(F)
    y = np.where(z < 0, (F(1.0) - np.abs(a)) * _sgn(b), b).astype(F)
    length = np.sqrt((x * x + y * y) + z * z, dtype=F)
    return np.stack([x / length, y / length, z / length], axis=1).astype(F)


def _coord(a):
    t = (F(a) * F(0.5) + F(0.5)) * F(8.0)
    if not t >= 0:                                   # a NaN lands on 0
        return 0
    return min(int(t), 7)


def texel_of(e):
    """the texel the direction e (probe -> point) falls into"""
    e = np.asarray(e, F)
    with np.errstate(all="ignore"):
        s = (np.abs(e[0]) + np.abs(e[1])) + np.abs(e[2])
        a, b = F(e[0] / s), F(e[1] / s)
        if e[2] < 0:
            a, b = F((F(1.0) - np.abs(b)) * _sgn(a)), F((F(1.0) - np.abs(a)) * _sgn(b))
        return _coord(b) * 8 + _coord(a)


def depth_project(directions, distances, max_distance):
    """directions (n, samples, 3), distances (n, samples) float32 -> (moments (n, 64, 2), open (n, 64)): every texel sums over all
    samples in ascending j from +0.0f; open marks the texels no sample reached (sw == 0)"""
    w, dist = np.asarray(directions, F), np.asarray(distances, F)
    n, samples = dist.shape
    d = texel_directions()
    sw, s1, s2 = (np.zeros((n, 64), F) for _ in range(3))
    for j in range(samples):
        wj = w[:, j, None, :]                                                       # (n, 1, 3)
        c = np.maximum((d[None, :, 0] * wj[..., 0] + d[None, :, 1] * wj[..., 1]) + d[None, :, 2] * wj[..., 2], F(0.0)).astype(F)
        c2 = c * c
        c4 = c2 * c2
        c8 = c4 * c4
        c16 = c8 * c8
        wt = c16 * c16
        dj = dist[:, j, None]
        sw = sw + wt
        s1 = s1 + wt * dj
        s2 = s2 + wt * (dj * dj)
    open_ = ~(sw > 0)
    m = F(max_distance)
    with np.errstate(all="ignore"):
        mean = np.where(open_, m, s1 / sw).astype(F)
        mean2 = np.where(open_, m * m, s2 / sw).astype(F)
    return np.stack([mean, mean2], axis=2), open_


def grid_positions(origin, spacing, counts):
    """Q of every probe, x fastest: origin[a] + (float)i_a * spacing[a]"""
    ax = [(F(origin[a]) + np.arange(counts[a]).astype(F) * F(spacing[a])).astype(F) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F)


def lookup(origin, spacing, counts, flags, normal_bias, sh, depth, P, N):
    """one query -> (rgb (3,), sumW), all float32.  sh (n, 9, 3); depth (n, 64, 2) or None"""
    origin, spacing, P, N = (np.asarray(x, F) for x in (origin, spacing, P, N))
    bias = F(normal_bias)
    with np.errstate(all="ignore"):
        Pb = (P + N * bias).astype(F)
        i0, f = [0] * 3, [F(0.0)] * 3
        for a in range(3):
            g = F((P[a] - origin[a]) / spacing[a])
            g = g if g > 0 else F(0.0)
            g = min(g, F(counts[a] - 1))
            if counts[a] > 1:
                i0[a] = min(int(g), counts[a] - 2)
                f[a] = F(g - F(i0[a]))
        acc, sum_w = np.zeros(3, F), F(0.0)
        for o in range(8):
            idx, t = [0] * 3, [F(0.0)] * 3
            for a in range(3):
                bit = (o >> a) & 1
                idx[a] = min(i0[a] + bit, counts[a] - 1)
                t[a] = f[a] if bit else F(F(1.0) - f[a])
            tri = F(F(t[0] * t[1]) * t[2])
            if tri == 0:
                continue
            probe = (idx[2] * counts[1] + idx[1]) * counts[0] + idx[0]
            Q = np.array([F(origin[a] + F(F(idx[a]) * spacing[a])) for a in range(3)], F)
            w = F(1.0)
            v = (Q - Pb).astype(F)
            r = np.sqrt(F(F(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), dtype=F)
            if r > 0:
                d = (v / r).astype(F)
                if flags & WRAP:
                    t_ = F(F(F(F(d[0] * N[0] + d[1] * N[1]) + d[2] * N[2]) + F(1.0)) * F(0.5))
                    w = F(w * F(F(t_ * t_) + F(0.2)))
                if flags & VISIBILITY:
                    mean, mean2 = depth[probe, texel_of(-d)]
                    if r > mean:
                        var = np.abs(F(mean2 - F(mean * mean)))
                        dl = F(r - mean)
                        ch = F(var / F(var + F(dl * dl)))
                        w = F(w * F(F(ch * ch) * ch))
            if w < F(0.2):
                w = F(w * F(F(w * w) * F(25.0)))
            w = F(w * tri)
            E = probe_ref.irradiance(sh[probe], N)
            acc = (acc + w * E).astype(F)
            sum_w = F(sum_w + w)
        rgb = (acc / sum_w).astype(F) if sum_w > 0 else np.zeros(3, F)
    return rgb, F(sum_w)
