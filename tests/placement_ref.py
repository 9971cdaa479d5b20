"""The probe-placement rule (include/ptmi_plugin.h Part 18) restated in numpy float32, for tests/test_probe_placement.py and
tests/test_gpu_probe_placement.py: how a stored offset is read, one step over hit and surface records (sides, counts, the three
selections, the inside test, the move and its limit) and the placed lookup.  Written from the header's text, not from
placement_rule.h; every operation is one float32 operation in the rule's order.  Sample directions and E(N) are Part 15's
(plugin.probe_directions, probe_ref.irradiance); the texel of a direction is Part 16's (volume_ref.texel_of)."""
import numpy as np

import probe_ref
import volume_ref

F = np.float32
U = np.uint32
NONE = 0xFFFFFFFF
INSIDE = 1
STATS_DTYPE = [("back", "<u4"), ("front", "<u4"), ("nearestBack", "<u4"), ("nearestFront", "<u4"), ("farthestFront", "<u4"),
               ("tNearestBack", "<f4"), ("tNearestFront", "<f4"), ("tFarthestFront", "<f4")]


def passes(o, spacing, max_offset):
    """|o[a]| <= maxOffset * spacing[a] on every axis; a NaN fails"""
    o, lim = np.asarray(o, F), (F(max_offset) * np.asarray(spacing, F)).astype(F)
    with np.errstate(invalid="ignore"):
        return bool((np.abs(o) <= lim).all())


def read_offset(stored, spacing, max_offset):
    stored = np.asarray(stored, F)
    return stored.copy() if passes(stored, spacing, max_offset) else np.zeros(3, F)


def step(directions, hits, surfaces, stored, spacing, min_front, share, max_offset, move):
    """One probe, one step.  directions (samples, 3) float32: w_j; hits (samples, 4) and surfaces (samples, 12) float32 rows.
    Returns (offset (3,) float32, state, stats record)."""
    w = np.asarray(directions, F)
    h = np.ascontiguousarray(hits, F)
    s = np.ascontiguousarray(surfaces, F)
    samples = h.shape[0]
    prim = h[:, 3].copy().view(U)
    tbits = h[:, 0].copy().view(U)
    n = s[:, 4:7]
    back, front = [], []
    with np.errstate(invalid="ignore"):
        for j in range(samples):
            if prim[j] == NONE:
                continue
            c = F(F(w[j, 0] * n[j, 0] + w[j, 1] * n[j, 1]) + w[j, 2] * n[j, 2])
            (back if c > 0 else front).append(j)
    st = np.zeros((), STATS_DTYPE)
    st["back"], st["front"] = len(back), len(front)
    st["nearestBack"] = st["nearestFront"] = st["farthestFront"] = NONE
    if back:
        j = min(back, key=lambda k: (int(tbits[k]), k))
        st["nearestBack"], st["tNearestBack"] = j, h[j, 0]
    if front:
        j = min(front, key=lambda k: (int(tbits[k]), k))
        st["nearestFront"], st["tNearestFront"] = j, h[j, 0]
        j = min(front, key=lambda k: (-int(tbits[k]), k))
        st["farthestFront"], st["tFarthestFront"] = j, h[j, 0]
    inside = F(len(back)) > F(F(share) * F(samples))
    o = read_offset(stored, spacing, max_offset)
    if move:
        cand = o.copy()
        mf = F(min_front)
        with np.errstate(all="ignore"):
            if inside:
                length = F(F(st["tNearestBack"]) + F(mf * F(0.5)))
                cand = (o + (w[int(st["nearestBack"])] * length).astype(F)).astype(F)
            elif front and F(st["tNearestFront"]) < mf:
                length = F(mf - F(st["tNearestFront"]))
                cand = (o - (w[int(st["nearestFront"])] * length).astype(F)).astype(F)
        if passes(cand, spacing, max_offset):
            o = cand
    return o, (INSIDE if inside else 0), st


def steps(directions, hits, surfaces, stored, params, move):
    """step() for n probes: directions (n, samples, 3), hits (n * samples, 4), surfaces (n * samples, 12), stored (n, 3);
    params an abi.PTProbePlaceParams.  Returns (offsets (n, 3), states (n,) uint32, stats (n,) records)."""
    d = np.asarray(directions, F)
    n, samples = d.shape[0], d.shape[1]
    h, s = np.asarray(hits, F).reshape(n, samples, 4), np.asarray(surfaces, F).reshape(n, samples, 12)
    spacing = [params.spacing[a] for a in range(3)]
    off, state, stats = np.zeros((n, 3), F), np.zeros(n, U), np.zeros(n, STATS_DTYPE)
    for i in range(n):
        off[i], state[i], stats[i] = step(d[i], h[i], s[i], np.asarray(stored, F).reshape(n, 3)[i], spacing, params.minFrontDistance, params.backfaceShare,
                                          params.maxOffset, move)
    return off, state, stats


def lookup(origin, spacing, counts, flags, normal_bias, sh, depth, placement, P, N):
    """Part 16's lookup (volume_ref.lookup, step for step) with Part 18's two changes: placement (n, 4) float32 rows -- offset xyz,
    state bits.  A corner whose state has INSIDE is skipped as one with tri == 0 is; a live one stands at Q + offset for step 4.
    -> (rgb (3,), sumW), all float32"""
    origin, spacing, P, N = (np.asarray(x, F) for x in (origin, spacing, P, N))
    pl = np.ascontiguousarray(placement, F).reshape(-1, 4)
    states = pl[:, 3].copy().view(U)
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
            if states[probe] & INSIDE:
                continue
            Q = np.array([F(origin[a] + F(F(idx[a]) * spacing[a])) for a in range(3)], F)
            Q = (Q + pl[probe, 0:3]).astype(F)
            w = F(1.0)
            v = (Q - Pb).astype(F)
            r = np.sqrt(F(F(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), dtype=F)
            if r > 0:
                d = (v / r).astype(F)
                if flags & volume_ref.WRAP:
                    t_ = F(F(F(F(d[0] * N[0] + d[1] * N[1]) + d[2] * N[2]) + F(1.0)) * F(0.5))
                    w = F(w * F(F(t_ * t_) + F(0.2)))
                if flags & volume_ref.VISIBILITY:
                    mean, mean2 = depth[probe, volume_ref.texel_of(-d)]
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
