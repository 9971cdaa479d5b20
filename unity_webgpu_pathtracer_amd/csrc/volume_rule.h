// volume_rule.h — probe volumes (include/ptmi_plugin.h Part 16): the one definition of the rule -- the octahedral
// texel directions, a texel's accumulation step and its moments, the grid cell of a point, the corner weights (trilinear, wrap,
// Chebyshev visibility, crush) and the blend -- shared by the kernels (pt_volume.hip) and the host twins (volume_host.cpp).  Every
// fp32 operator is one IEEE binary32 operation in the order written, and both sides are compiled with -ffp-contract=off, so both
// give the same bits.  tests/volume_ref.py restates it.  Seeding, sphere direction and E(N) are sh_rule.h's.
#pragma once
#include "sh_rule.h"
#include <type_traits>

#define PT_VOL_HD PT_SH_HD

namespace ptvol {

constexpr uint32_t kRes = 8u;               // the octahedral map is 8 x 8
constexpr uint32_t kTexels = 64u;           // texel l = v * 8 + u: lane l of the resolve's wave
constexpr uint64_t kChunkSamples = 1ull << 21;      // PTProbeDepth: a chunk holds floor(2^21 / samples) whole probes
constexpr uint32_t kMaxAxis = 1024u;

PT_VOL_HD float sgn(float x) { return x < 0.0f ? -1.0f : 1.0f; }        // sgn(0) = +1

// the direction of texel l's centre
PT_VOL_HD void texel_direction(uint32_t l, float d[3])
{
    const uint32_t u = l & 7u, v = l >> 3;
    const float a = ((float)u + 0.5f) * 0.25f - 1.0f;
    const float b = ((float)v + 0.5f) * 0.25f - 1.0f;
    const float z = (1.0f - pt_abs(a)) - pt_abs(b);
    float x = a, y = b;
    if (z < 0.0f) {
        x = (1.0f - pt_abs(b)) * sgn(a);
        y = (1.0f - pt_abs(a)) * sgn(b);
    }
    const float len = pt_sqrt((x * x + y * y) + z * z);
    d[0] = x / len;
    d[1] = y / len;
    d[2] = z / len;
}

// [0, 1] -> a texel coordinate: min((uint32_t)t, 7) for every t a unit vector gives; a NaN lands on 0
PT_VOL_HD uint32_t texel_coord(float a)
{
    const float t = (a * 0.5f + 0.5f) * 8.0f;
    return t >= 0.0f ? (t < 8.0f ? (uint32_t)t : 7u) : 0u;
}

// the texel a direction e (from the probe to the point) falls into: nearest texel
PT_VOL_HD uint32_t texel_of(const float e[3])
{
    const float s = (pt_abs(e[0]) + pt_abs(e[1])) + pt_abs(e[2]);
    float a = e[0] / s, b = e[1] / s;
    if (e[2] < 0.0f) {
        const float a2 = (1.0f - pt_abs(b)) * sgn(a);
        const float b2 = (1.0f - pt_abs(a)) * sgn(b);
        a = a2;
        b = b2;
    }
    return texel_coord(b) * kRes + texel_coord(a);
}

// one sample {w, dist} into a texel's three sums: the lobe is cos^32 by squaring
PT_VOL_HD void accumulate(float& sw, float& s1, float& s2, const float d[3], const float w[3], float dist)
{
    const float c = pt_max((d[0] * w[0] + d[1] * w[1]) + d[2] * w[2], 0.0f);
    const float c2 = c * c, c4 = c2 * c2, c8 = c4 * c4, c16 = c8 * c8, wt = c16 * c16;
    sw = sw + wt;
    s1 = s1 + wt * dist;
    s2 = s2 + wt * (dist * dist);
}

// a texel no sample reached counts as open
PT_VOL_HD void moments(float sw, float s1, float s2, float maxDistance, float& mean, float& mean2)
{
    if (sw > 0.0f) {
        mean = s1 / sw;
        mean2 = s2 / sw;
    } else {
        mean = maxDistance;
        mean2 = maxDistance * maxDistance;
    }
}

// the lower probe i0 and the fraction f of a point on one axis
PT_VOL_HD void cell(float p, float origin, float spacing, uint32_t count, uint32_t& i0, float& f)
{
    float g = (p - origin) / spacing;
    g = g > 0.0f ? g : 0.0f;                                    // a NaN lands on 0
    g = pt_min(g, (float)(count - 1u));
    if (count > 1u) {
        const uint32_t i = (uint32_t)g;
        i0 = i < count - 2u ? i : count - 2u;
        f = g - (float)i0;
    } else {
        i0 = 0u;
        f = 0.0f;
    }
}

struct Cell { uint32_t i0[3]; float f[3]; };

PT_VOL_HD Cell cell_of(const PTProbeGrid& G, const float P[3])
{
    Cell c;
    for (uint32_t a = 0; a < 3u; ++a) cell(P[a], G.origin[a], G.spacing[a], G.counts[a], c.i0[a], c.f[a]);
    return c;
}

// corner o of the cell: its probe index, its position Q and its trilinear weight
PT_VOL_HD float corner(const PTProbeGrid& G, const Cell& c, uint32_t o, uint32_t& probe, float Q[3])
{
    uint32_t i[3];
    float t[3];
    for (uint32_t a = 0; a < 3u; ++a) {
        const uint32_t bit = (o >> a) & 1u;
        const uint32_t up = c.i0[a] + bit;
        i[a] = up < G.counts[a] - 1u ? up : G.counts[a] - 1u;
        t[a] = bit ? c.f[a] : 1.0f - c.f[a];
        Q[a] = G.origin[a] + (float)i[a] * G.spacing[a];
    }
    probe = (i[2] * G.counts[1] + i[1]) * G.counts[0] + i[0];
    return (t[0] * t[1]) * t[2];
}

// The weight of a live corner before the moments are known: w after the wrap term, the distance r to the biased point and the
// texel the visibility term reads.  false: the visibility term does not apply (flag off, or r is not > 0)
PT_VOL_HD bool corner_weight(uint32_t flags, const float Q[3], const float Pb[3], const float N[3], float& w, float& r, uint32_t& texel)
{
    w = 1.0f;
    const float v[3] = {Q[0] - Pb[0], Q[1] - Pb[1], Q[2] - Pb[2]};
    r = pt_sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(r > 0.0f)) return false;
    const float dir[3] = {v[0] / r, v[1] / r, v[2] / r};
    if (flags & PT_GRID_WRAP) {
        const float t = (((dir[0] * N[0] + dir[1] * N[1]) + dir[2] * N[2]) + 1.0f) * 0.5f;
        w = w * (t * t + 0.2f);
    }
    if (!(flags & PT_GRID_VISIBILITY)) return false;
    const float e[3] = {-dir[0], -dir[1], -dir[2]};
    texel = texel_of(e);
    return true;
}

// Chebyshev's bound on the share of the texel's distances that reach r
PT_VOL_HD float visibility(float w, float r, float mean, float mean2)
{
    if (r > mean) {
        const float var = pt_abs(mean2 - mean * mean);
        const float dl = r - mean;
        const float ch = var / (var + dl * dl);
        w = w * ((ch * ch) * ch);
    }
    return w;
}

PT_VOL_HD float crush(float w)
{
    if (w < 0.2f) w = w * ((w * w) * 25.0f);
    return w;
}

// One query, whole: sh and depth are read through the callables, so that the kernel can use 16- and 8-byte loads.
//   loadSH(probe, float co[27]); loadDepth(probe, texel, float& mean, float& mean2)
//   loadPlacement(probe, float off[3], uint32_t& state): Part 18's placed lookup -- a corner that is PT_PROBE_INSIDE is skipped as
//   one with tri == 0 is, a live one stands at Q + off for the weights.  With NoPlacement the switch is made at compile time: that
//   path neither loads nor adds ((-0) + 0 would change a sign bit), so Part 16's lookup keeps its bits.
struct NoPlacement {};

template <class LoadSH, class LoadDepth, class LoadPlacement>
PT_VOL_HD void lookup(const PTProbeGrid& G, const float P[3], const float N[3], LoadSH loadSH, LoadDepth loadDepth, LoadPlacement loadPlacement, float out[4])
{
    const float Pb[3] = {P[0] + N[0] * G.normalBias, P[1] + N[1] * G.normalBias, P[2] + N[2] * G.normalBias};
    const Cell c = cell_of(G, P);
    float acc[3] = {0.0f, 0.0f, 0.0f}, sumW = 0.0f;
    for (uint32_t o = 0; o < 8u; ++o) {
        uint32_t probe, texel = 0u;
        float Q[3], w, r;
        const float tri = corner(G, c, o, probe, Q);
        if (tri == 0.0f) continue;                              // reads nothing
        if constexpr (!std::is_same<LoadPlacement, NoPlacement>::value) {
            float off[3];
            uint32_t state;
            loadPlacement(probe, off, state);
            if (state & PT_PROBE_INSIDE) continue;              // reads nothing more
            for (uint32_t a = 0; a < 3u; ++a) Q[a] = Q[a] + off[a];
        }
        if (corner_weight(G.flags, Q, Pb, N, w, r, texel)) {
            float mean, mean2;
            loadDepth(probe, texel, mean, mean2);
            w = visibility(w, r, mean, mean2);
        }
        w = crush(w);
        w = w * tri;
        float co[27], E[3];
        loadSH(probe, co);
        ptsh::irradiance(co, N, E);
        for (uint32_t ch = 0; ch < 3u; ++ch) acc[ch] = acc[ch] + w * E[ch];
        sumW = sumW + w;
    }
    for (uint32_t ch = 0; ch < 3u; ++ch) out[ch] = sumW > 0.0f ? acc[ch] / sumW : 0.0f;
    out[3] = sumW;
}

template <class LoadSH, class LoadDepth>
PT_VOL_HD void lookup(const PTProbeGrid& G, const float P[3], const float N[3], LoadSH loadSH, LoadDepth loadDepth, float out[4])
{
    lookup(G, P, N, loadSH, loadDepth, NoPlacement{}, out);
}

// ---- the host twins and the checks the entry points share (volume_host.cpp); false: err says why ----
bool check_grid(const PTProbeGrid* grid, std::string& err);
bool check_max_distance(float maxDistance, std::string& err);
bool check_samples(uint32_t samples, std::string& err);
bool depth_project_host(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const float* distances, float maxDistance,
                        PTProbeDepthMap* out, std::string& err);
bool grid_irradiance_host(const PTProbeGrid* grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTReceiver* queries, uint64_t count,
                          PTIrradiance* out, std::string& err);

} // namespace ptvol
