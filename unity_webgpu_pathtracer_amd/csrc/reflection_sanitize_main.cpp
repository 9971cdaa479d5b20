// reflection_sanitize_main.cpp — the host twins of the reflection-probe kernels (reflection_host.cpp) in a stand-alone program for
// `make reflection-sanitize` (AddressSanitizer + UBSan, host code only, no GPU): makes the directions of 8 x 8 and 16 x 16 maps at
// both ends of the sample range into exactly sized heap arrays, folds random radiance, prefilters random, constant and single-texel
// maps at 8 / 2, 16 / 3 and 32 / 4, looks up random and edge directions -- the axes, the fold line, the -z pole, a NaN, a zero
// vector, every roughness case, a probe index out of range -- with and without boxes, and makes the refusals.  Prints
// "reflection ok" and returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "reflection_rule.h"

namespace {

uint32_t g_state = 2020u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("reflection-sanitize: %s\n", what); return 1; }

} // namespace

int main()
{
    using namespace ptrefl;
    std::string err;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // directions and fold
    for (uint32_t res : {8u, 16u})
        for (uint32_t samples : {1u, 3u})
            for (uint32_t first : {0u, 0xFFFFFFF0u}) {
                const uint64_t n = 2, slots = n * res * res * samples;
                std::vector<PTProbe> probes(n);
                for (uint64_t i = 0; i < n; ++i) probes[i] = PTProbe{{rnd(), rnd(), rnd()}, 0xFFFFFFF6u + (uint32_t)i * 15u};
                std::vector<PTRadianceRay> rays(slots);
                if (!directions_host(probes.data(), n, res, first, samples, rays.data(), err)) return bad(err.c_str());
                for (uint64_t s = 0; s < slots; ++s) {
                    const float* d = rays[s].direction;
                    const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                    if (!(std::fabs(len - 1.0f) < 4e-7f)) return bad("a sample direction is not of unit length");
                    float a, b;
                    oct_coords(d, a, b);
                    const uint32_t t = (uint32_t)((s / samples) % (res * res));
                    const float x = (a * 0.5f + 0.5f) * (float)res, y = (b * 0.5f + 0.5f) * (float)res, tol = 1e-5f * (float)res;
                    if (!(x >= (float)(t % res) - tol && x <= (float)(t % res + 1u) + tol && y >= (float)(t / res) - tol && y <= (float)(t / res + 1u) + tol))
                        return bad("a sample direction lies outside its texel");
                }
                std::vector<PTRadiance> rad(slots);
                for (auto& r : rad) r = PTRadiance{{rnd() * 4.0f, rnd() < 0.3f ? 0.0f : rnd(), rnd()}, 0u};
                std::vector<PTReflectionTexel> base(n * res * res);
                if (!fold_host(rad.data(), n, res, samples, base.data(), err)) return bad(err.c_str());
                for (const auto& t : base)
                    if (!(t.rgb[0] >= 0.0f && t.rgb[0] <= 4.0f && t.aux >= 0.0f)) return bad("a folded texel is out of range");
            }
    // prefilter and lookup
    const uint32_t shapes[][2] = {{8u, 2u}, {16u, 3u}, {32u, 4u}};
    for (const auto& sh : shapes) {
        const uint32_t res = sh[0], levels = sh[1], baseTexels = res * res, mapTexels = level_offset(res, levels);
        const uint64_t n = 2;
        std::vector<PTReflectionTexel> base(n * baseTexels), maps(n * mapTexels), flat(baseTexels, PTReflectionTexel{{0.25f, 0.25f, 0.25f}, 0.25f}), flatMap(mapTexels);
        for (auto& t : base) t = PTReflectionTexel{{0.05f + rnd() * 4.0f, 0.05f + rnd() * 4.0f, 0.05f + rnd() * 4.0f}, rnd()};
        if (!prefilter_host(base.data(), n, res, levels, maps.data(), err)) return bad(err.c_str());
        if (!prefilter_host(flat.data(), 1, res, levels, flatMap.data(), err)) return bad(err.c_str());
        for (const auto& t : maps)
            if (!(t.rgb[0] > 0.04f && t.rgb[0] < 4.1f && t.aux >= 0.0f)) return bad("a prefiltered texel left the range of its base");
        for (const auto& t : flatMap)
            if (t.rgb[0] != 0.25f || t.rgb[1] != 0.25f || t.rgb[2] != 0.25f) return bad("a constant map did not come out exactly");
        std::vector<PTReflectionTexel> spike(baseTexels, PTReflectionTexel{{0.0f, 0.0f, 0.0f}, 0.0f}), spikeMap(mapTexels);
        spike[baseTexels / 3u].rgb[0] = 1000.0f;
        if (!prefilter_host(spike.data(), 1, res, levels, spikeMap.data(), err)) return bad(err.c_str());
        float last = std::numeric_limits<float>::infinity();
        for (uint32_t k = 0; k < levels; ++k) {
            float peak = 0.0f;
            for (uint32_t t = level_offset(res, k); t < level_offset(res, k + 1u); ++t) peak = std::fmax(peak, spikeMap[t].rgb[0]);
            if (!(peak < last && peak > 0.0f)) return bad("a bright texel's peak does not fall with the level");
            last = peak;
        }
        // queries
        std::vector<PTReflectionQuery> q;
        const float rough[] = {0.0f, 1.0f, 0.5f, 1.0f / 3.0f, -1.0f, 2.0f, nan};
        const float edges[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {0.6f, 0.8f, 0}, {-0.6f, 0.8f, 0}, {0, 0.6f, -0.8f},
                                  {0.8f, 0, -0.6f}, {1e-5f, 1e-5f, -1}, {-1e-5f, 1e-5f, -1}, {1e-5f, -1e-5f, -1}, {-1e-5f, -1e-5f, -1}, {0, 0, 0}, {nan, 0, 1},
                                  {3.0f, -4.0f, 12.0f}};
        for (const auto& e : edges)
            for (float r : rough) q.push_back(PTReflectionQuery{{rnd() - 0.5f, rnd() - 0.5f, rnd() - 0.5f}, r, {e[0], e[1], e[2]}, (uint32_t)(q.size() % n)});
        for (int k = 0; k < 2000; ++k) {
            float d[3] = {rnd() - 0.5f, rnd() - 0.5f, rnd() - 0.5f};
            const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-9f;
            const float s = k % 7 == 0 ? 2.0f : 0.9f;                // some positions outside the boxes
            q.push_back(PTReflectionQuery{{(rnd() - 0.5f) * s, (rnd() - 0.5f) * s, (rnd() - 0.5f) * s}, rnd() * 1.2f - 0.1f, {d[0] / len, d[1] / len, d[2] / len},
                                          (uint32_t)(k % n)});
        }
        q[5].probe = (uint32_t)n;
        q[6].probe = 0xFFFFFFFFu;
        std::vector<PTProbe> probes = {PTProbe{{0.2f, -0.1f, 0.15f}, 0u}, PTProbe{{-0.3f, 0.25f, 0.0f}, 1u}};
        std::vector<PTReflectionBox> boxes = {PTReflectionBox{{-0.5f, -0.5f, -0.5f}, 0.0f, {0.5f, 0.5f, 0.5f}, 0.0f},
                                              PTReflectionBox{{-0.6f, -0.5f, -0.7f}, 0.0f, {0.5f, 0.55f, 0.5f}, 0.0f}};
        std::vector<PTReflectionTexel> out(q.size()), outBox(q.size()), outFlat(q.size());
        if (!lookup_host(maps.data(), n, res, levels, nullptr, nullptr, q.data(), q.size(), out.data(), err)) return bad(err.c_str());
        if (!lookup_host(maps.data(), n, res, levels, probes.data(), nullptr, q.data(), q.size(), outBox.data(), err)) return bad(err.c_str());
        for (size_t k = 0; k < q.size(); ++k)
            if (std::memcmp(&out[k], &outBox[k], sizeof(out[k])) != 0) return bad("probes without boxes changed a lookup");
        if (!lookup_host(maps.data(), n, res, levels, probes.data(), boxes.data(), q.data(), q.size(), outBox.data(), err)) return bad(err.c_str());
        if (!lookup_host(flatMap.data(), 1, res, levels, nullptr, nullptr, q.data(), q.size(), outFlat.data(), err)) return bad(err.c_str());
        for (size_t k = 0; k < q.size(); ++k) {
            const bool finiteDir = std::isfinite(q[k].direction[0]) && (q[k].direction[0] != 0.0f || q[k].direction[1] != 0.0f || q[k].direction[2] != 0.0f);
            if (q[k].probe >= n) {
                if (out[k].rgb[0] != 0.0f || out[k].aux != 0.0f || outBox[k].rgb[1] != 0.0f) return bad("a probe index out of range did not give zeros");
                continue;
            }
            if (!finiteDir) continue;           // a NaN or zero direction reads NaN, from inside the map: the sanitizers watch the taps
            if (!(out[k].rgb[0] > 0.04f && out[k].rgb[0] < 4.1f && out[k].aux == 1.0f)) return bad("a lookup left the range of its map");
            if (!(outBox[k].rgb[0] > 0.04f && outBox[k].rgb[0] < 4.1f)) return bad("a box-projected lookup left the range of its map");
            if (q[k].probe == 0u && outFlat[k].rgb[2] != 0.25f) return bad("a constant map was not looked up exactly");
        }
    }
    // refusals
    {
        PTProbe p = {{0, 0, 0}, 1u};
        std::vector<PTRadianceRay> rays(64);
        std::vector<PTRadiance> rad(64);
        std::vector<PTReflectionTexel> base(64), map(80);
        PTReflectionQuery q = {{0, 0, 0}, 0.5f, {0, 0, 1}, 0u};
        PTReflectionBox box = {{-1, -1, -1}, 0.0f, {1, 1, 1}, 0.0f};
        PTReflectionTexel o;
        if (directions_host(&p, 1, 8, 0, 0, rays.data(), err)) return bad("samples 0 was not refused");
        if (directions_host(&p, 1, 8, 0, 65537u, rays.data(), err)) return bad("samples 65537 was not refused");
        if (directions_host(&p, 1, 12, 0, 1, rays.data(), err)) return bad("res 12 was not refused");
        if (directions_host(&p, 1, 4, 0, 1, rays.data(), err)) return bad("res 4 was not refused");
        if (directions_host(&p, 1, 512, 0, 1, rays.data(), err)) return bad("res 512 was not refused");
        if (directions_host(nullptr, 1, 8, 0, 1, rays.data(), err)) return bad("probes == NULL was not refused");
        if (!directions_host(nullptr, 0, 8, 0, 1, nullptr, err)) return bad("count 0 was refused");
        if (fold_host(rad.data(), 1, 8, 0, base.data(), err)) return bad("fold: samples 0 was not refused");
        if (fold_host(nullptr, 1, 8, 1, base.data(), err)) return bad("fold: radiance == NULL was not refused");
        if (prefilter_host(base.data(), 1, 8, 1, map.data(), err)) return bad("levels 1 was not refused");
        if (prefilter_host(base.data(), 1, 8, 3, map.data(), err)) return bad("levels 3 at res 8 was not refused");
        if (prefilter_host(base.data(), 1, 8, 2, base.data(), err)) return bad("out == base was not refused");
        if (prefilter_host(nullptr, 1, 8, 2, map.data(), err)) return bad("base == NULL was not refused");
        if (!prefilter_host(base.data(), 1, 8, 2, map.data(), err)) return bad(err.c_str());
        if (lookup_host(map.data(), 1, 8, 2, nullptr, &box, &q, 1, &o, err)) return bad("boxes without probes were not refused");
        if (lookup_host(nullptr, 1, 8, 2, nullptr, nullptr, &q, 1, &o, err)) return bad("maps == NULL was not refused");
        if (lookup_host(map.data(), 1, 16, 4, nullptr, nullptr, &q, 1, &o, err)) return bad("levels 4 at res 16 was not refused");
        if (!lookup_host(map.data(), 1, 8, 2, &p, &box, &q, 1, &o, err)) return bad(err.c_str());
    }
    std::printf("reflection ok\n");
    return 0;
}
