// reflection_host.cpp — the host twins of the reflection-probe kernels (include/ptmi_plugin.h Part 20): the rule of
// reflection_rule.h in plain loops, and the argument checks the context's entry points share with them.  No GPU involved.
#include "reflection_rule.h"

#include <vector>

namespace ptrefl {

bool check_samples(uint32_t samples, std::string& err)
{
    if (samples >= 1u && samples <= PT_GATHER_MAX_SAMPLES) return true;
    err = "samples = " + std::to_string(samples) + " (1 ... " + std::to_string(PT_GATHER_MAX_SAMPLES) + ")";
    return false;
}

bool check_layout(uint32_t res, uint32_t levels, bool needLevels, std::string& err)
{
    if (res < kMinRes || res > kMaxRes || (res & (res - 1u)) != 0u) {
        err = "res = " + std::to_string(res) + " is not a power of two in [" + std::to_string(kMinRes) + ", " + std::to_string(kMaxRes) + "]";
        return false;
    }
    if (needLevels && (levels < 2u || levels > log2_res(res) - 1u)) {
        err = "levels = " + std::to_string(levels) + " (2 ... " + std::to_string(log2_res(res) - 1u) + " at res " + std::to_string(res) +
              ": the coarsest level is at least 4 x 4)";
        return false;
    }
    return true;
}

bool directions_host(const PTProbe* probes, uint64_t count, uint32_t res, uint32_t firstSample, uint32_t samples, PTRadianceRay* rays, std::string& err)
{
    if (!check_samples(samples, err) || !check_layout(res, 0u, false, err)) return false;
    if (count && (!probes || !rays)) { err = "probes / rays == NULL"; return false; }
    const uint32_t texels = res * res;
    for (uint64_t i = 0; i < count; ++i)
        for (uint32_t t = 0; t < texels; ++t)
            for (uint32_t j = 0; j < samples; ++j) {
                uint32_t rng = sample_rng(probes[i].seed, t, firstSample, j);
                PTRadianceRay& r = rays[(i * texels + t) * samples + j];
                for (uint32_t a = 0; a < 3u; ++a) r.origin[a] = probes[i].position[a];
                sample_direction(res, t % res, t / res, rng, r.direction);
                r.rng = rng;
                r.reserved = 0u;
            }
    return true;
}

bool fold_host(const PTRadiance* radiance, uint64_t count, uint32_t res, uint32_t samples, PTReflectionTexel* out, std::string& err)
{
    if (!check_samples(samples, err) || !check_layout(res, 0u, false, err)) return false;
    if (count && (!radiance || !out)) { err = "radiance / out == NULL"; return false; }
    const uint64_t texels = count * res * res;
    for (uint64_t t = 0; t < texels; ++t) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t j = 0; j < samples; ++j) fold_step(acc, radiance[t * samples + j].rgb);
        for (uint32_t c = 0; c < 3u; ++c) out[t].rgb[c] = acc[c] / (float)samples;
        out[t].aux = acc[3];
    }
    return true;
}

bool prefilter_host(const PTReflectionTexel* base, uint64_t count, uint32_t res, uint32_t levels, PTReflectionTexel* out, std::string& err)
{
    if (!check_layout(res, levels, true, err)) return false;
    if (count && (!base || !out)) { err = "base / out == NULL"; return false; }
    const uint32_t baseTexels = res * res, mapTexels = level_offset(res, levels);
    if (count) {
        const char *b0 = (const char*)base, *b1 = b0 + count * baseTexels * sizeof(PTReflectionTexel);
        const char *o0 = (const char*)out, *o1 = o0 + count * mapTexels * sizeof(PTReflectionTexel);
        if (b0 < o1 && o0 < b1) { err = "out aliases base"; return false; }
    }
    struct Source { float l[3], J; };
    std::vector<Source> src(baseTexels);
    for (uint32_t s = 0; s < baseTexels; ++s) source(res, s, src[s].l, src[s].J);
    for (uint64_t i = 0; i < count; ++i) {
        const PTReflectionTexel* in = base + i * baseTexels;
        PTReflectionTexel* map = out + i * mapTexels;
        for (uint32_t s = 0; s < baseTexels; ++s) map[s] = in[s];
        for (uint32_t k = 1; k < levels; ++k) {
            const uint32_t Rk = res >> k;
            const float g = lobe_g(k, levels);
            PTReflectionTexel* level = map + level_offset(res, k);
            for (uint32_t o = 0; o < Rk * Rk; ++o) {
                float n[3], len;
                direction(Rk, o % Rk, o / Rk, 0.5f, 0.5f, n, len);
                float acc[3] = {0.0f, 0.0f, 0.0f}, sw = 0.0f;
                for (uint32_t s = 0; s < baseTexels; ++s) {
                    float w;
                    if (!weight(n, src[s].l, src[s].J, g, w)) continue;
                    for (uint32_t c = 0; c < 3u; ++c) acc[c] = acc[c] + w * in[s].rgb[c];
                    sw = sw + w;
                }
                for (uint32_t c = 0; c < 3u; ++c) level[o].rgb[c] = acc[c] / sw;
                level[o].aux = sw;
            }
        }
    }
    return true;
}

bool lookup_host(const PTReflectionTexel* maps, uint64_t probeCount, uint32_t res, uint32_t levels, const PTProbe* probes, const PTReflectionBox* boxes,
                 const PTReflectionQuery* queries, uint64_t count, PTReflectionTexel* out, std::string& err)
{
    if (!check_layout(res, levels, true, err)) return false;
    if ((probeCount && !maps) || (count && (!queries || !out))) { err = "maps / queries / out == NULL"; return false; }
    if (boxes && !probes) { err = "boxes without probes (the projection needs the probes' positions)"; return false; }
    const uint32_t mapTexels = level_offset(res, levels);
    for (uint64_t q = 0; q < count; ++q) {
        const PTReflectionQuery& Q = queries[q];
        if (Q.probe >= probeCount) { out[q] = PTReflectionTexel{{0.0f, 0.0f, 0.0f}, 0.0f}; continue; }
        const PTReflectionTexel* map = maps + (uint64_t)Q.probe * mapTexels;
        float o[4];
        lookup(res, levels, Q.position, Q.roughness, Q.direction, boxes ? probes[Q.probe].position : nullptr, boxes ? boxes[Q.probe].bmin : nullptr,
               boxes ? boxes[Q.probe].bmax : nullptr, [&](uint32_t t, float rgb[3]) { for (uint32_t c = 0; c < 3u; ++c) rgb[c] = map[t].rgb[c]; }, o);
        out[q] = PTReflectionTexel{{o[0], o[1], o[2]}, o[3]};
    }
    return true;
}

} // namespace ptrefl
