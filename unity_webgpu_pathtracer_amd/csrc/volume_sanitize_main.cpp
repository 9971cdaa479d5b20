// volume_sanitize_main.cpp — the host twins of the probe-volume kernels (volume_host.cpp) in a stand-alone program for
// `make volume-sanitize` (AddressSanitizer + UBSan, host code only, no GPU): projects constant and random distances into exactly
// sized heap arrays at sample counts on both sides of 64, checks that every texel direction encodes to its own texel, looks up
// grids with one, two and three probes on an axis from inside, outside, on a probe and at a NaN, and makes the refusals.  Prints
// "volume ok" and returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "volume_rule.h"

namespace {

uint32_t g_state = 4242u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("volume-sanitize: %s\n", what); return 1; }

} // namespace

int main()
{
    using namespace ptvol;
    std::string err;
    for (uint32_t l = 0; l < kTexels; ++l) {
        float d[3];
        texel_direction(l, d);
        const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(std::fabs(len - 1.0f) < 4e-7f)) return bad("a texel direction is not of unit length");
        if (texel_of(d) != l) return bad("a texel direction does not encode to its own texel");
    }
    const uint32_t counts[] = {1u, 63u, 64u, 70u, 4096u};
    const float maxDistance = 2.5f;
    for (uint32_t samples : counts) {
        const uint64_t n = 3;
        std::vector<PTProbe> probes(n);
        for (uint64_t i = 0; i < n; ++i) probes[i] = PTProbe{{rnd(), rnd(), rnd()}, 0xFFFFFFF0u + (uint32_t)i};
        std::vector<float> same(n * samples, 0.75f), dist(n * samples);
        for (float& t : dist) t = rnd() < 0.3f ? maxDistance : rnd() * maxDistance;
        std::vector<PTProbeDepthMap> flat(n), rec(n);
        if (!depth_project_host(probes.data(), n, 0xFFFFFFFEu, samples, same.data(), maxDistance, flat.data(), err)) return bad(err.c_str());
        if (!depth_project_host(probes.data(), n, 0xFFFFFFFEu, samples, dist.data(), maxDistance, rec.data(), err)) return bad(err.c_str());
        const float tol = (2.0f * (float)samples + 2.0f) * 5.9604645e-8f;
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t l = 0; l < kTexels; ++l) {
                const float m = flat[i].moments[l][0], m2 = flat[i].moments[l][1];
                const bool open = m == maxDistance && m2 == maxDistance * maxDistance;
                // (with a single sample a texel's only weight may be subnormal, and its products keep few bits: the bound is for
                // sums that normal terms dominate)
                const bool fits = samples < 63u ? m >= 0.0f && m <= 1.5f && m2 >= 0.0f && m2 <= 1.5f
                                                : std::fabs(m - 0.75f) <= 0.75f * tol && std::fabs(m2 - 0.5625f) <= 0.5625f * tol;
                if (!open && !fits) {
                    std::printf("samples %u probe %u texel %u: mean %g mean2 %g\n", samples, (unsigned)i, l, m, m2);
                    return bad("the moments of a constant distance are off");
                }
                if (!(rec[i].moments[l][0] > 0.0f && rec[i].moments[l][0] <= maxDistance * (1.0f + tol))) return bad("a mean distance is out of range");
            }
    }
    // lookups
    const uint32_t grids[][3] = {{3u, 2u, 2u}, {1u, 1u, 1u}, {2u, 1u, 3u}};
    for (const auto& cnt : grids) {
        const uint64_t probes = (uint64_t)cnt[0] * cnt[1] * cnt[2];
        std::vector<PTProbeCoeffs> sh(probes);
        std::vector<PTProbeDepthMap> depth(probes);
        for (auto& s : sh) { for (int k = 0; k < 9; ++k) for (int c = 0; c < 3; ++c) s.sh[k][c] = rnd() - 0.3f; s.m2 = 0.0f; }
        for (auto& d : depth) for (uint32_t l = 0; l < kTexels; ++l) { const float m = 0.2f + rnd(); d.moments[l][0] = m; d.moments[l][1] = m * m + 0.05f * rnd(); }
        std::vector<PTReceiver> q;
        for (int k = 0; k < 40; ++k) q.push_back(PTReceiver{{rnd() * 4.0f - 1.5f, rnd() * 3.0f - 1.0f, rnd() * 4.0f - 1.5f}, 0u, {0.0f, 0.6f, 0.8f}, 0u});
        q.push_back(PTReceiver{{-0.5f, 0.25f, -0.5f}, 0u, {1.0f, 0.0f, 0.0f}, 0u});                     // on probe 0 with no bias below
        q.push_back(PTReceiver{{std::numeric_limits<float>::quiet_NaN(), 0.0f, 0.0f}, 0u, {0.0f, 1.0f, 0.0f}, 0u});
        q.push_back(PTReceiver{{1e30f, -1e30f, 1e30f}, 0u, {0.0f, 1.0f, 0.0f}, 0u});
        for (uint32_t flags = 0; flags < 4u; ++flags) {
            PTProbeGrid G = {{-0.5f, 0.25f, -0.5f}, flags, {0.5f, 0.75f, 0.5f}, flags & 1u ? 0.0f : 0.02f, {cnt[0], cnt[1], cnt[2]}, 0u};
            std::vector<PTIrradiance> out(q.size());
            if (!grid_irradiance_host(&G, sh.data(), depth.data(), q.data(), q.size(), out.data(), err)) return bad(err.c_str());
            for (size_t k = 0; k < 41; ++k)
                if (!std::isfinite(out[k].rgb[0]) || !(out[k].m2 >= 0.0f)) return bad("a lookup is not finite");
            if (flags == 0u && !(std::fabs(out[3].m2 - 1.0f) <= 4.0f * 1.1920929e-7f)) return bad("the support without flags is not 1");
            // without the visibility flag the depth is never read
            if (!(flags & PT_GRID_VISIBILITY) && !grid_irradiance_host(&G, sh.data(), nullptr, q.data(), q.size(), out.data(), err)) return bad(err.c_str());
        }
    }
    // refusals
    {
        PTProbe p = {{0, 0, 0}, 1u};
        PTProbeDepthMap o;
        PTProbeCoeffs s = {};
        PTReceiver r = {{0, 0, 0}, 0u, {0, 1, 0}, 0u};
        PTIrradiance e;
        float t = 1.0f;
        const float inf = std::numeric_limits<float>::infinity();
        if (depth_project_host(&p, 1, 0, 0, &t, 1.0f, &o, err)) return bad("samples 0 was not refused");
        if (depth_project_host(&p, 1, 0, 65537u, &t, 1.0f, &o, err)) return bad("samples 65537 was not refused");
        if (depth_project_host(&p, 1, 0, 1, &t, 0.0f, &o, err)) return bad("maxDistance 0 was not refused");
        if (depth_project_host(&p, 1, 0, 1, &t, inf, &o, err)) return bad("an infinite maxDistance was not refused");
        if (depth_project_host(&p, 1, 0, 1, &t, PT_FAR_PLANE, &o, err)) return bad("maxDistance = PT_FAR_PLANE was not refused");
        if (depth_project_host(nullptr, 1, 0, 1, &t, 1.0f, &o, err)) return bad("probes == NULL was not refused");
        if (!depth_project_host(nullptr, 0, 0, 1, nullptr, 1.0f, nullptr, err)) return bad("count 0 was refused");
        const PTProbeGrid ok = {{0, 0, 0}, 0u, {1, 1, 1}, 0.0f, {1u, 1u, 1u}, 0u};
        if (!grid_irradiance_host(&ok, &s, nullptr, &r, 1, &e, err)) return bad(err.c_str());
        PTProbeGrid g = ok; g.flags = 4u;
        if (grid_irradiance_host(&g, &s, nullptr, &r, 1, &e, err)) return bad("an unknown flag was not refused");
        g = ok; g.flags = PT_GRID_VISIBILITY;
        if (grid_irradiance_host(&g, &s, nullptr, &r, 1, &e, err)) return bad("visibility without depth was not refused");
        g = ok; g.reserved = 1u;
        if (grid_irradiance_host(&g, &s, nullptr, &r, 1, &e, err)) return bad("reserved != 0 was not refused");
        g = ok; g.counts[1] = 0u;
        if (grid_irradiance_host(&g, &s, nullptr, &r, 1, &e, err)) return bad("a count of 0 was not refused");
        g = ok; g.counts[2] = 1025u;
        if (grid_irradiance_host(&g, &s, nullptr, &r, 1, &e, err)) return bad("a count of 1025 was not refused");
        g = ok; g.spacing[0] = 0.0f;
        if (grid_irradiance_host(&g, &s, nullptr, &r, 1, &e, err)) return bad("a spacing of 0 was not refused");
        g = ok; g.spacing[2] = inf;
        if (grid_irradiance_host(&g, &s, nullptr, &r, 1, &e, err)) return bad("an infinite spacing was not refused");
        g = ok; g.normalBias = -1.0f;
        if (grid_irradiance_host(&g, &s, nullptr, &r, 1, &e, err)) return bad("a negative normalBias was not refused");
        if (grid_irradiance_host(nullptr, &s, nullptr, &r, 1, &e, err)) return bad("grid == NULL was not refused");
        if (grid_irradiance_host(&ok, nullptr, nullptr, &r, 1, &e, err)) return bad("sh == NULL was not refused");
    }
    std::printf("volume ok\n");
    return 0;
}
