// probe_host.cpp — the host twins of the probe kernels (include/ptmi_plugin.h Part 15): the rule of sh_rule.h in
// plain loops, with the 64 lane partials of the wave kept in an array and folded by the rule's tree.  No GPU involved.
#include "sh_rule.h"

#include <cstring>

namespace ptsh {

namespace {
bool check_samples(uint32_t samples, std::string& err)
{
    if (samples >= 1u && samples <= PT_GATHER_MAX_SAMPLES) return true;
    err = "samples = " + std::to_string(samples) + " (1 ... " + std::to_string(PT_GATHER_MAX_SAMPLES) + ")";
    return false;
}
} // namespace

bool probe_directions_host(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, PTRadianceRay* rays, std::string& err)
{
    if (!check_samples(samples, err)) return false;
    if (count && (!probes || !rays)) { err = "probes / rays == NULL"; return false; }
    for (uint64_t i = 0; i < count; ++i)
        for (uint32_t j = 0; j < samples; ++j) {
            PTRadianceRay& r = rays[i * samples + j];
            uint32_t rng = sample_rng(probes[i].seed, firstSample, j);
            direction(rng, r.direction);
            memcpy(r.origin, probes[i].position, sizeof(r.origin));
            r.rng = rng;
            r.reserved = 0u;
        }
    return true;
}

bool probe_project_host(const float* directions, const float* colours, uint64_t count, uint32_t samples, PTProbeCoeffs* out, std::string& err)
{
    if (!check_samples(samples, err)) return false;
    if (count && (!directions || !colours || !out)) { err = "directions / colours / out == NULL"; return false; }
    for (uint64_t i = 0; i < count; ++i) {
        float acc[kLanes][kSums] = {};                   // +0.0f
        for (uint32_t j = 0; j < samples; ++j) {
            const size_t s = ((size_t)i * samples + j) * 3u;
            accumulate(acc[j % kLanes], colours + s, directions + s);
        }
        float* o = &out[i].sh[0][0];
        for (uint32_t t = 0; t < kSums; ++t) {
            float v[kLanes];
            for (uint32_t l = 0; l < kLanes; ++l) v[l] = acc[l][t];
            const float v0 = fold(v);
            if (t < 27u) o[t] = scale(v0, samples);
            else out[i].m2 = v0;
        }
    }
    return true;
}

bool probe_irradiance_host(const PTProbeCoeffs* sh, uint64_t probeCount, const PTProbeQuery* queries, uint64_t count, PTIrradiance* out, std::string& err)
{
    if (count && (!queries || !out || (probeCount && !sh))) { err = "sh / queries / out == NULL"; return false; }
    for (uint64_t q = 0; q < count; ++q) {
        float E[3] = {0.0f, 0.0f, 0.0f};
        if (queries[q].probe < probeCount) irradiance(&sh[queries[q].probe].sh[0][0], queries[q].normal, E);
        out[q] = PTIrradiance{{E[0], E[1], E[2]}, 0.0f};
    }
    return true;
}

} // namespace ptsh
