// placement_sanitize_main.cpp — the host twins of the probe-placement kernels (placement_host.cpp) in a stand-alone program for
// `make placement-sanitize` (AddressSanitizer + UBSan, host code only, no GPU): runs steps over random hit and surface records in
// exactly sized heap arrays at sample counts on both sides of 64, with and without a move and statistics, checks the counts and
// that every offset keeps its limit, looks up a placed grid with live, moved and buried probes, and makes the refusals.  Prints
// "placement ok" and returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "placement_rule.h"

namespace {

uint32_t g_state = 1818u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("placement-sanitize: %s\n", what); return 1; }

} // namespace

int main()
{
    using namespace ptplace;
    std::string err;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const PTProbePlaceParams Q = {{0.5f, 0.75f, 0.5f}, 1.5f, 0.1f, 0.25f, 0.45f, 4u};
    const uint32_t counts[] = {1u, 2u, 63u, 64u, 65u, 70u, 4096u};
    for (uint32_t samples : counts) {
        const uint64_t n = 5;
        std::vector<PTProbe> probes(n);
        for (uint64_t i = 0; i < n; ++i) probes[i] = PTProbe{{rnd(), rnd(), rnd()}, 0xFFFFFFF0u + (uint32_t)i};
        std::vector<PTRayHit> hits(n * samples);
        std::vector<PTRaySurface> surf(n * samples);
        for (uint64_t k = 0; k < n * samples; ++k) {
            const bool miss = rnd() < 0.33f;
            hits[k] = PTRayHit{miss ? Q.maxDistance : 0.001f + rnd() * 0.3f, rnd(), rnd(), miss ? kNone : (uint32_t)k};
            const float z = rnd() < 0.02f ? nan : rnd() * 2.0f - 1.0f;
            surf[k] = PTRaySurface{{0, 0, 0}, hits[k].t, {rnd() * 2.0f - 1.0f, rnd() * 2.0f - 1.0f, z}, 0, {0, 0}, kNone, (uint32_t)k};
        }
        for (int move = 0; move < 2; ++move) {
            std::vector<PTProbePlacement> pl(n);
            for (uint64_t i = 0; i < n; ++i) pl[i] = PTProbePlacement{{0.0f, 0.0f, 0.0f}, 7u};
            pl[1] = PTProbePlacement{{0.1f, -0.2f, 0.05f}, 0u};
            pl[2] = PTProbePlacement{{nan, 0.0f, 0.0f}, 0u};
            pl[3] = PTProbePlacement{{0.0f, 0.0f, 0.3f}, 0u};                                   // past 0.45 * 0.5
            std::vector<PTProbePlaceStats> st(n);
            if (!place_step_host(probes.data(), n, 0xFFFFFFF0u, samples, &Q, hits.data(), surf.data(), move, pl.data(), st.data(), err)) return bad(err.c_str());
            if (!place_step_host(probes.data(), n, 0xFFFFFFF0u, samples, &Q, hits.data(), surf.data(), move, pl.data(), nullptr, err)) return bad(err.c_str());
            for (uint64_t i = 0; i < n; ++i) {
                uint32_t hit = 0;
                for (uint32_t j = 0; j < samples; ++j) hit += hits[i * samples + j].prim != kNone;
                if (st[i].back + st[i].front != hit) return bad("back + front is not the number of hits");
                if ((st[i].back == 0u) != (st[i].nearestBack == kNone) || (st[i].front == 0u) != (st[i].nearestFront == kNone)) return bad("a nearest index and its count disagree");
                if (st[i].front && !(st[i].tFarthestFront >= st[i].tNearestFront)) return bad("the farthest front sample is nearer than the nearest");
                if (pl[i].state > PT_PROBE_INSIDE) return bad("a state is neither live nor inside");
                if (!passes(Q, pl[i].offset)) return bad("an offset is past its limit");
            }
            if (!move && (pl[2].offset[0] != 0.0f || pl[3].offset[2] != 0.0f || pl[1].offset[1] != -0.2f)) return bad("a stored offset was not read as the rule reads it");
        }
    }
    // the placed lookup
    {
        const uint32_t cnt[3] = {3u, 2u, 2u};
        const uint64_t probes = 12;
        std::vector<PTProbeCoeffs> sh(probes);
        std::vector<PTProbeDepthMap> depth(probes);
        std::vector<PTProbePlacement> pl(probes);
        for (auto& s : sh) { for (int k = 0; k < 9; ++k) for (int c = 0; c < 3; ++c) s.sh[k][c] = rnd() - 0.3f; s.m2 = 0.0f; }
        for (auto& d : depth) for (uint32_t l = 0; l < ptvol::kTexels; ++l) { const float m = 0.2f + rnd(); d.moments[l][0] = m; d.moments[l][1] = m * m + 0.05f * rnd(); }
        for (uint64_t i = 0; i < probes; ++i) pl[i] = PTProbePlacement{{(rnd() - 0.5f) * 0.4f, (rnd() - 0.5f) * 0.4f, (rnd() - 0.5f) * 0.4f}, i % 3u == 0u ? PT_PROBE_INSIDE : 0u};
        std::vector<PTReceiver> q;
        for (int k = 0; k < 40; ++k) q.push_back(PTReceiver{{rnd() * 4.0f - 1.5f, rnd() * 3.0f - 1.0f, rnd() * 4.0f - 1.5f}, 0u, {0.0f, 0.6f, 0.8f}, 0u});
        q.push_back(PTReceiver{{nan, 0.0f, 0.0f}, 0u, {0.0f, 1.0f, 0.0f}, 0u});
        for (uint32_t flags = 0; flags < 4u; ++flags) {
            PTProbeGrid G = {{-0.5f, 0.25f, -0.5f}, flags, {0.5f, 0.75f, 0.5f}, 0.02f, {cnt[0], cnt[1], cnt[2]}, 0u};
            std::vector<PTIrradiance> out(q.size()), plain(q.size()), same(q.size());
            if (!grid_irradiance_placed_host(&G, sh.data(), depth.data(), pl.data(), q.data(), q.size(), out.data(), err)) return bad(err.c_str());
            for (size_t k = 0; k < 40; ++k)
                if (!std::isfinite(out[k].rgb[0]) || !(out[k].m2 >= 0.0f)) return bad("a placed lookup is not finite");
            if (!grid_irradiance_placed_host(&G, sh.data(), depth.data(), nullptr, q.data(), q.size(), same.data(), err)) return bad(err.c_str());
            if (!ptvol::grid_irradiance_host(&G, sh.data(), depth.data(), q.data(), q.size(), plain.data(), err)) return bad(err.c_str());
            for (size_t k = 0; k < 40; ++k)
                if (same[k].rgb[1] != plain[k].rgb[1] || same[k].m2 != plain[k].m2) return bad("placement == NULL is not the plain lookup");
        }
        for (auto& p : pl) p.state = PT_PROBE_INSIDE;
        PTProbeGrid G = {{-0.5f, 0.25f, -0.5f}, 0u, {0.5f, 0.75f, 0.5f}, 0.0f, {cnt[0], cnt[1], cnt[2]}, 0u};
        std::vector<PTIrradiance> out(q.size());
        if (!grid_irradiance_placed_host(&G, sh.data(), nullptr, pl.data(), q.data(), q.size(), out.data(), err)) return bad(err.c_str());
        for (const auto& o : out)
            if (o.rgb[0] != 0.0f || o.rgb[1] != 0.0f || o.rgb[2] != 0.0f || o.m2 != 0.0f) return bad("a lookup among buried probes is not 0");
    }
    // refusals
    {
        PTProbe p = {{0, 0, 0}, 1u};
        PTRayHit h = {1.0f, 0, 0, kNone};
        PTRaySurface s = {};
        PTProbePlacement o = {};
        const PTProbePlaceParams ok = {{1, 1, 1}, 1.0f, 0.1f, 0.25f, 0.45f, 0u};
        if (!place_step_host(&p, 1, 0, 1, &ok, &h, &s, 1, &o, nullptr, err)) return bad(err.c_str());
        if (place_step_host(&p, 1, 0, 0, &ok, &h, &s, 1, &o, nullptr, err)) return bad("samples 0 was not refused");
        if (place_step_host(&p, 1, 0, 65537u, &ok, &h, &s, 1, &o, nullptr, err)) return bad("samples 65537 was not refused");
        if (place_step_host(&p, 1, 0, 1, nullptr, &h, &s, 1, &o, nullptr, err)) return bad("params == NULL was not refused");
        if (place_step_host(nullptr, 1, 0, 1, &ok, &h, &s, 1, &o, nullptr, err)) return bad("probes == NULL was not refused");
        if (!place_step_host(nullptr, 0, 0, 1, &ok, nullptr, nullptr, 1, nullptr, nullptr, err)) return bad("count 0 was refused");
        PTProbePlaceParams q = ok; q.spacing[1] = 0.0f;
        if (check_params(&q, err)) return bad("a spacing of 0 was not refused");
        q = ok; q.spacing[2] = inf;
        if (check_params(&q, err)) return bad("an infinite spacing was not refused");
        q = ok; q.maxDistance = PT_FAR_PLANE;
        if (check_params(&q, err)) return bad("maxDistance = PT_FAR_PLANE was not refused");
        q = ok; q.minFrontDistance = -0.1f;
        if (check_params(&q, err)) return bad("a negative minFrontDistance was not refused");
        q = ok; q.minFrontDistance = nan;
        if (check_params(&q, err)) return bad("a NaN minFrontDistance was not refused");
        q = ok; q.backfaceShare = 1.5f;
        if (check_params(&q, err)) return bad("a backfaceShare of 1.5 was not refused");
        q = ok; q.backfaceShare = nan;
        if (check_params(&q, err)) return bad("a NaN backfaceShare was not refused");
        q = ok; q.maxOffset = 0.5f;
        if (check_params(&q, err)) return bad("a maxOffset of 0.5 was not refused");
        q = ok; q.maxOffset = -0.1f;
        if (check_params(&q, err)) return bad("a negative maxOffset was not refused");
        q = ok; q.iterations = 17u;
        if (check_params(&q, err)) return bad("17 iterations were not refused");
        q = ok; q.iterations = 16u;
        if (!check_params(&q, err)) return bad("16 iterations were refused");
        if (check_flags(2u, err) || !check_flags(PT_PLACE_KEEP_OFFSETS, err)) return bad("the flag check is off");
    }
    std::printf("placement ok\n");
    return 0;
}
