// volume_host.cpp — the host twins of the probe-volume kernels (include/ptmi_plugin.h Part 16): the rule of
// volume_rule.h in plain loops, and the argument checks the context's entry points share with them.  No GPU involved.
#include "volume_rule.h"

#include <cmath>

namespace ptvol {

bool check_samples(uint32_t samples, std::string& err)
{
    if (samples >= 1u && samples <= PT_GATHER_MAX_SAMPLES) return true;
    err = "samples = " + std::to_string(samples) + " (1 ... " + std::to_string(PT_GATHER_MAX_SAMPLES) + ")";
    return false;
}

bool check_max_distance(float maxDistance, std::string& err)
{
    if (std::isfinite(maxDistance) && maxDistance > 0.0f && maxDistance < PT_FAR_PLANE) return true;
    err = "maxDistance = " + std::to_string(maxDistance) + " is not finite, positive and below PT_FAR_PLANE";
    return false;
}

bool check_grid(const PTProbeGrid* grid, std::string& err)
{
    if (!grid) { err = "grid == NULL"; return false; }
    if (grid->flags & ~(PT_GRID_WRAP | PT_GRID_VISIBILITY)) { err = "unknown flag bits " + std::to_string(grid->flags); return false; }
    if (grid->reserved != 0u) { err = "grid.reserved != 0"; return false; }
    for (int a = 0; a < 3; ++a) {
        if (grid->counts[a] == 0u || grid->counts[a] > kMaxAxis) {
            err = "grid.counts[" + std::to_string(a) + "] = " + std::to_string(grid->counts[a]) + " (1 ... " + std::to_string(kMaxAxis) + ")";
            return false;
        }
        if (!(std::isfinite(grid->spacing[a]) && grid->spacing[a] > 0.0f)) {
            err = "grid.spacing[" + std::to_string(a) + "] is not finite and positive";
            return false;
        }
        if (!std::isfinite(grid->origin[a])) { err = "grid.origin[" + std::to_string(a) + "] is not finite"; return false; }
    }
    if (!(std::isfinite(grid->normalBias) && grid->normalBias >= 0.0f)) { err = "grid.normalBias is not finite and non-negative"; return false; }
    return true;
}

bool depth_project_host(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const float* distances, float maxDistance,
                        PTProbeDepthMap* out, std::string& err)
{
    if (!check_samples(samples, err) || !check_max_distance(maxDistance, err)) return false;
    if (count && (!probes || !distances || !out)) { err = "probes / distances / out == NULL"; return false; }
    float d[kTexels][3];
    for (uint32_t l = 0; l < kTexels; ++l) texel_direction(l, d[l]);
    for (uint64_t i = 0; i < count; ++i) {
        float sw[kTexels] = {}, s1[kTexels] = {}, s2[kTexels] = {};      // +0.0f
        for (uint32_t j = 0; j < samples; ++j) {
            uint32_t rng = ptsh::sample_rng(probes[i].seed, firstSample, j);
            float w[3];
            ptsh::direction(rng, w);
            const float dist = distances[i * samples + j];
            for (uint32_t l = 0; l < kTexels; ++l) accumulate(sw[l], s1[l], s2[l], d[l], w, dist);
        }
        for (uint32_t l = 0; l < kTexels; ++l) moments(sw[l], s1[l], s2[l], maxDistance, out[i].moments[l][0], out[i].moments[l][1]);
    }
    return true;
}

bool grid_irradiance_host(const PTProbeGrid* grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTReceiver* queries, uint64_t count,
                          PTIrradiance* out, std::string& err)
{
    if (!check_grid(grid, err)) return false;
    if (!sh || (count && (!queries || !out))) { err = "sh / queries / out == NULL"; return false; }
    if ((grid->flags & PT_GRID_VISIBILITY) && !depth) { err = "PT_GRID_VISIBILITY with depth == NULL"; return false; }
    for (uint64_t q = 0; q < count; ++q) {
        float o[4];
        lookup(*grid, queries[q].position, queries[q].normal,
               [&](uint32_t probe, float co[27]) { for (uint32_t t = 0; t < 27u; ++t) co[t] = (&sh[probe].sh[0][0])[t]; },
               [&](uint32_t probe, uint32_t texel, float& mean, float& mean2) { mean = depth[probe].moments[texel][0]; mean2 = depth[probe].moments[texel][1]; },
               o);
        out[q] = PTIrradiance{{o[0], o[1], o[2]}, o[3]};
    }
    return true;
}

} // namespace ptvol
