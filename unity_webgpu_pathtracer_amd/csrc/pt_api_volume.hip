// pt_api_volume.hip — probe volumes: a per-probe octahedral depth record baked through the closest-hit query, and depth-aware
// trilinear lookups of an SH probe grid (include/ptmi_plugin.h Part 16).
#include "pt_context.h"
#include "volume_rule.h"

namespace {

int check_depth_args(uint32_t samples, float maxDistance, const char* who)
{
    std::string err;
    if (!ptvol::check_max_distance(maxDistance, err)) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": " + err);
    if (!ptvol::check_samples(samples, err)) return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": " + err);
    return PT_OK;
}

// One chunk of floor(2^21 / samples) whole probes after another on the context stream, all through the same scratch: rays,
// closest-hit query, resolve.  No state sets are involved.
int probe_depth(PTContext* c, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples, float maxDistance, PTProbeDepthMap* dOut)
{
    RoctxRange range("PT probe depth (enqueue)");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = query_prepare(c))) return rc;
    const uint64_t perChunk = ptvol::kChunkSamples / samples;       // >= 32 probes (samples <= 65536)
    const uint64_t slots = (count < perChunk ? count : perChunk) * samples;
    PTContext::Volume& W = c->volume;
    // growing drains the context stream, which every earlier call's chunks ran on
    if ((rc = W.rays.reserve(slots * 2u * sizeof(float4), c->stream))) return rc;
    if ((rc = W.hits.reserve(slots * sizeof(float4), c->stream))) return rc;
    const bool stats = c->statsLevel > 0;
    const uint32_t cap = c->query.caps[pt_query_kernel_index(c->scene.hasTlas != 0u, PT_QUERY_CLOSEST, stats)];
    return for_each_launch(count, perChunk, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_probe_depth_rays(dProbes + first, n, samples, firstSample, maxDistance, (float4*)W.rays.ptr, c->stream));
        HIP_TRY(pt_launch_query(c->scene, (const float4*)W.rays.ptr, n * samples, PT_QUERY_CLOSEST, stats, (float4*)W.hits.ptr, nullptr,
                                (uint2*)c->query.slab.ptr, cap, (unsigned long long*)c->dStats.ptr, c->stream));
        HIP_TRY(pt_launch_probe_depth_resolve(dProbes + first, n, samples, firstSample, maxDistance, (const float4*)W.hits.ptr, dOut + first, c->stream));
        return PT_OK;
    });
}

} // namespace

extern "C" {

PT_API int PTProbeDepth(PTContext* c, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples, float maxDistance, PTProbeDepthMap* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeDepth: ctx == NULL");
    if (int rc = check_depth_args(samples, maxDistance, "PTProbeDepth")) return rc;
    if (!dProbes || !dOut) return fail(PT_ERR_INVALID_ARG, "PTProbeDepth: probes/out == NULL");
    if (misaligned(dProbes) || misaligned(dOut)) return fail(PT_ERR_INVALID_ARG, "PTProbeDepth: probes/out is not 16-byte aligned");
    return probe_depth(c, dProbes, count, firstSample, samples, maxDistance, dOut);
}

PT_API int PTProbeDepthHost(PTContext* c, const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, float maxDistance, PTProbeDepthMap* out)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeDepthHost: ctx == NULL");
    if (int rc = check_depth_args(samples, maxDistance, "PTProbeDepthHost")) return rc;
    if (!probes || !out) return fail(PT_ERR_INVALID_ARG, "PTProbeDepthHost: probes/out == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    return host_round_trip(c, c->volume.host, probes, count, out, [&](const PTProbe* dProbes, PTProbeDepthMap* dOut) {
        return probe_depth(c, dProbes, count, firstSample, samples, maxDistance, dOut);
    });
}

PT_API int PTProbeGridIrradiance(PTContext* c, const PTProbeGrid* grid, const PTProbeCoeffs* dSH, const PTProbeDepthMap* dDepth, const PTReceiver* dQueries,
                                 uint64_t count, PTIrradiance* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiance: ctx == NULL");
    std::string err;
    if (!ptvol::check_grid(grid, err)) return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiance: " + err);
    if (!dSH || !dQueries || !dOut) return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiance: sh/queries/out == NULL");
    if ((grid->flags & PT_GRID_VISIBILITY) && !dDepth) return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiance: PT_GRID_VISIBILITY with depth == NULL");
    if (misaligned(dSH) || misaligned(dDepth) || misaligned(dQueries) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, "PTProbeGridIrradiance: sh/depth/queries/out is not 16-byte aligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_probe_grid_irradiance(*grid, dSH, dDepth, dQueries + first, n, dOut + first, c->stream));
        return PT_OK;
    });
}

} // extern "C"
