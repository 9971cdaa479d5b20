// pt_api_placement.hip — probe placement: relocation and classification of a grid's probes through the closest-hit query with
// surface records, and the lookup that honours the result (include/ptmi_plugin.h Part 18).
#include "pt_context.h"
#include "placement_rule.h"

namespace {

int check_place_args(uint32_t samples, const PTProbePlaceParams* params, uint32_t flags, const char* who)
{
    std::string err;
    if (!ptplace::check_params(params, err) || !ptplace::check_flags(flags, err)) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": " + err);
    if (!ptvol::check_samples(samples, err)) return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": " + err);
    return PT_OK;
}

// One chunk of floor(2^20 / samples) whole probes after another on the context stream, all through the same scratch; a chunk goes
// through its iterations + 1 steps -- rays, closest-hit query with surface records, step -- before the next one starts.  No state
// sets are involved.  dOut holds the offsets between the steps.
int probe_place(PTContext* c, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples, const PTProbePlaceParams& Q, uint32_t flags,
                PTProbePlacement* dOut, PTProbePlaceStats* dStats)
{
    RoctxRange range("PT probe placement (enqueue)");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = query_prepare(c))) return rc;
    const uint64_t perChunk = ptplace::kChunkSamples / samples;     // >= 16 probes (samples <= 65536)
    const uint64_t slots = (count < perChunk ? count : perChunk) * samples;
    PTContext::Placement& W = c->placement;
    // growing drains the context stream, which every earlier call's chunks ran on
    if ((rc = W.rays.reserve(slots * 2u * sizeof(float4), c->stream))) return rc;
    if ((rc = W.hits.reserve(slots * sizeof(float4), c->stream))) return rc;
    if ((rc = W.surfaces.reserve(slots * 3u * sizeof(float4), c->stream))) return rc;
    const bool stats = c->statsLevel > 0;
    const uint32_t cap = c->query.caps[pt_query_kernel_index(c->scene.hasTlas != 0u, 2u, stats)];
    if (!(flags & PT_PLACE_KEEP_OFFSETS)) HIP_TRY(hipMemsetAsync(dOut, 0, count * sizeof(PTProbePlacement), c->stream));       // o = 0, live
    return for_each_launch(count, perChunk, [&](uint64_t first, uint32_t n) {
        for (uint32_t step = 0; step <= Q.iterations; ++step) {
            const bool last = step == Q.iterations;
            HIP_TRY(pt_launch_probe_place_rays(dProbes + first, n, samples, firstSample, Q, dOut + first, (float4*)W.rays.ptr, c->stream));
            HIP_TRY(pt_launch_query(c->scene, (const float4*)W.rays.ptr, n * samples, 2u, stats, (float4*)W.hits.ptr, (float4*)W.surfaces.ptr,
                                    (uint2*)c->query.slab.ptr, cap, (unsigned long long*)c->dStats.ptr, c->stream));
            HIP_TRY(pt_launch_probe_place_step(dProbes + first, n, samples, firstSample, Q, (const float4*)W.hits.ptr, (const float4*)W.surfaces.ptr, !last,
                                               dOut + first, last && dStats ? dStats + first : nullptr, c->stream));
        }
        return PT_OK;
    });
}

} // namespace

extern "C" {

PT_API int PTProbePlace(PTContext* c, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples, const PTProbePlaceParams* params,
                        uint32_t flags, PTProbePlacement* dOut, PTProbePlaceStats* dStats)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbePlace: ctx == NULL");
    if (int rc = check_place_args(samples, params, flags, "PTProbePlace")) return rc;
    if (!dProbes || !dOut) return fail(PT_ERR_INVALID_ARG, "PTProbePlace: probes/out == NULL");
    if (misaligned(dProbes) || misaligned(dOut) || misaligned(dStats)) return fail(PT_ERR_INVALID_ARG, "PTProbePlace: probes/out/stats is not 16-byte aligned");
    return probe_place(c, dProbes, count, firstSample, samples, *params, flags, dOut, dStats);
}

PT_API int PTProbePlaceHost(PTContext* c, const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const PTProbePlaceParams* params,
                            uint32_t flags, PTProbePlacement* out, PTProbePlaceStats* stats)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbePlaceHost: ctx == NULL");
    if (int rc = check_place_args(samples, params, flags, "PTProbePlaceHost")) return rc;
    if (!probes || !out) return fail(PT_ERR_INVALID_ARG, "PTProbePlaceHost: probes/out == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    // the statistics are a second result: their copy back is enqueued behind the steps and ends in the round trip's synchronise,
    // which is also why hostStats may regrow here without a drain (no earlier call's use of it is still in flight)
    if (stats)
        if (int rc = c->placement.hostStats.reserve(count * sizeof(PTProbePlaceStats))) return rc;
    return host_round_trip(c, c->placement.host, probes, count, out, [&](const PTProbe* dProbes, PTProbePlacement* dOut) {
        if (flags & PT_PLACE_KEEP_OFFSETS) HIP_TRY(hipMemcpyAsync(dOut, out, count * sizeof(PTProbePlacement), hipMemcpyHostToDevice, c->stream));
        PTProbePlaceStats* dStats = stats ? (PTProbePlaceStats*)c->placement.hostStats.ptr : nullptr;
        if (int rc = probe_place(c, dProbes, count, firstSample, samples, *params, flags, dOut, dStats)) return rc;
        if (stats) HIP_TRY(hipMemcpyAsync(stats, dStats, count * sizeof(PTProbePlaceStats), hipMemcpyDeviceToHost, c->stream));
        return (int)PT_OK;
    });
}

PT_API int PTProbeGridIrradiancePlaced(PTContext* c, const PTProbeGrid* grid, const PTProbeCoeffs* dSH, const PTProbeDepthMap* dDepth,
                                       const PTProbePlacement* dPlacement, const PTReceiver* dQueries, uint64_t count, PTIrradiance* dOut)
{
    if (!dPlacement) return PTProbeGridIrradiance(c, grid, dSH, dDepth, dQueries, count, dOut);
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiancePlaced: ctx == NULL");
    std::string err;
    if (!ptvol::check_grid(grid, err)) return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiancePlaced: " + err);
    if (!dSH || !dQueries || !dOut) return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiancePlaced: sh/queries/out == NULL");
    if ((grid->flags & PT_GRID_VISIBILITY) && !dDepth) return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiancePlaced: PT_GRID_VISIBILITY with depth == NULL");
    if (misaligned(dSH) || misaligned(dDepth) || misaligned(dPlacement) || misaligned(dQueries) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiancePlaced: sh/depth/placement/queries/out is not 16-byte aligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_probe_grid_irradiance_placed(*grid, dSH, dDepth, dPlacement, dQueries + first, n, dOut + first, c->stream));
        return PT_OK;
    });
}

} // extern "C"
