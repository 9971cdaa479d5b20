// placement_host.cpp — the host twins of the probe-placement kernels (include/ptmi_plugin.h Part 18): the rule of
// placement_rule.h in plain loops, and the argument checks the context's entry points share with them.  No GPU involved.
#include "placement_rule.h"

#include <cmath>

namespace ptplace {

bool check_flags(uint32_t flags, std::string& err)
{
    if (!(flags & ~PT_PLACE_KEEP_OFFSETS)) return true;
    err = "unknown flag bits " + std::to_string(flags);
    return false;
}

bool check_params(const PTProbePlaceParams* p, std::string& err)
{
    if (!p) { err = "params == NULL"; return false; }
    for (int a = 0; a < 3; ++a)
        if (!(std::isfinite(p->spacing[a]) && p->spacing[a] > 0.0f)) {
            err = "params.spacing[" + std::to_string(a) + "] is not finite and positive";
            return false;
        }
    if (!ptvol::check_max_distance(p->maxDistance, err)) return false;
    if (!(std::isfinite(p->minFrontDistance) && p->minFrontDistance >= 0.0f)) { err = "params.minFrontDistance is not finite and non-negative"; return false; }
    if (!(p->backfaceShare >= 0.0f && p->backfaceShare <= 1.0f)) { err = "params.backfaceShare is not in [0, 1]"; return false; }
    if (!(p->maxOffset >= 0.0f && p->maxOffset < 0.5f)) { err = "params.maxOffset is not in [0, 0.5)"; return false; }
    if (p->iterations > PT_PLACE_MAX_ITERATIONS) {
        err = "params.iterations = " + std::to_string(p->iterations) + " (0 ... " + std::to_string(PT_PLACE_MAX_ITERATIONS) + ")";
        return false;
    }
    return true;
}

bool place_step_host(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const PTProbePlaceParams* params, const PTRayHit* hits,
                     const PTRaySurface* surfaces, int move, PTProbePlacement* inout, PTProbePlaceStats* stats, std::string& err)
{
    if (!check_params(params, err) || !ptvol::check_samples(samples, err)) return false;
    if (count && (!probes || !hits || !surfaces || !inout)) { err = "probes / hits / surfaces / inout == NULL"; return false; }
    for (uint64_t i = 0; i < count; ++i) {
        Tally T = empty();
        for (uint32_t j = 0; j < samples; ++j) {
            const PTRayHit& h = hits[i * samples + j];
            if (h.prim == kNone) continue;                      // a miss: its surface record is not read
            uint32_t rng = ptsh::sample_rng(probes[i].seed, firstSample, j);
            float w[3];
            ptsh::direction(rng, w);
            add_hit(T, j, h.t, w, surfaces[i * samples + j].normal);
        }
        const PTProbePlaceStats s = stats_of(T);
        float o[3];
        read_offset(*params, inout[i].offset, o);
        inout[i].state = finish(*params, probes[i].seed, firstSample, samples, s, move != 0, o);
        for (uint32_t a = 0; a < 3u; ++a) inout[i].offset[a] = o[a];
        if (stats) stats[i] = s;
    }
    return true;
}

bool grid_irradiance_placed_host(const PTProbeGrid* grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTProbePlacement* placement,
                                 const PTReceiver* queries, uint64_t count, PTIrradiance* out, std::string& err)
{
    if (!placement) return ptvol::grid_irradiance_host(grid, sh, depth, queries, count, out, err);
    if (!ptvol::check_grid(grid, err)) return false;
    if (!sh || (count && (!queries || !out))) { err = "sh / queries / out == NULL"; return false; }
    if ((grid->flags & PT_GRID_VISIBILITY) && !depth) { err = "PT_GRID_VISIBILITY with depth == NULL"; return false; }
    for (uint64_t q = 0; q < count; ++q) {
        float o[4];
        ptvol::lookup(*grid, queries[q].position, queries[q].normal,
                      [&](uint32_t probe, float co[27]) { for (uint32_t t = 0; t < 27u; ++t) co[t] = (&sh[probe].sh[0][0])[t]; },
                      [&](uint32_t probe, uint32_t texel, float& mean, float& mean2) { mean = depth[probe].moments[texel][0]; mean2 = depth[probe].moments[texel][1]; },
                      [&](uint32_t probe, float off[3], uint32_t& state) {
                          for (uint32_t a = 0; a < 3u; ++a) off[a] = placement[probe].offset[a];
                          state = placement[probe].state;
                      },
                      o);
        out[q] = PTIrradiance{{o[0], o[1], o[2]}, o[3]};
    }
    return true;
}

} // namespace ptplace
