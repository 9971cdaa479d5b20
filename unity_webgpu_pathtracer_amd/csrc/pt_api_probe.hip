// pt_api_probe.hip — SH light probes: nine spherical-harmonic coefficients per channel at a caller's list of positions, and their
// evaluation (include/ptmi_plugin.h Part 15).
#include "pt_context.h"

namespace {

int check_flags(uint32_t flags, const char* who)
{
    if (flags & ~PT_PROBE_DELTA_LIGHTS) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": unknown flag bits " + std::to_string(flags));
    return PT_OK;
}

// The delta lights of the whole call, on the context stream: one any-hit ray per (probe, light) pair into the context's scratch.
// Every chunk's chain starts behind an event recorded on that stream afterwards, so its resolve finds the records complete.
int trace_delta_lights(PTContext* c, const PTProbe* dProbes, uint64_t count, uint32_t lightCount)
{
    constexpr uint64_t kLaunchPairs = 1ull << 28;              // the query kernels' ray index stays 32-bit (pt_api_query.hip)
    int rc;
    if ((rc = query_prepare(c))) return rc;
    PTContext::Probe& W = c->probe;
    const uint64_t pairs = count * lightCount;
    // growing drains the context stream, which every earlier call's chunks have joined
    if ((rc = W.deltaRays.reserve(pairs * 2u * sizeof(float4), c->stream))) return rc;
    if ((rc = W.deltaLi.reserve(pairs * sizeof(float4), c->stream))) return rc;
    if ((rc = W.deltaHits.reserve(pairs * sizeof(float4), c->stream))) return rc;
    const bool stats = c->statsLevel > 0;
    const uint32_t cap = c->query.caps[pt_query_kernel_index(c->scene.hasTlas != 0u, PT_QUERY_ANY_HIT, stats)];
    const uint64_t perLaunch = kLaunchPairs / lightCount;       // whole probes
    if (perLaunch == 0u) return fail(PT_ERR_UNSUPPORTED, "PTProbeSH: more than 2^28 lights");
    return for_each_launch(count, perLaunch, [&](uint64_t first, uint32_t n) {
        float4* rays = (float4*)W.deltaRays.ptr + first * lightCount * 2u;
        float4* li = (float4*)W.deltaLi.ptr + first * lightCount;
        float4* hits = (float4*)W.deltaHits.ptr + first * lightCount;
        HIP_TRY(pt_launch_probe_delta_rays(c->scene, dProbes + first, n, rays, li, c->stream));
        HIP_TRY(pt_launch_query(c->scene, rays, n * lightCount, PT_QUERY_ANY_HIT, stats, hits, nullptr, (uint2*)c->query.slab.ptr, cap,
                                (unsigned long long*)c->dStats.ptr, c->stream));
        return PT_OK;
    });
}

// One launch sequence per chunk of floor(PT_RADIANCE_CHUNK / samples) whole probes (enqueue_list_chunks), behind the delta lights.
// p1 is inside wavefront_limits already (import_sampled_params), so no check is left that the delta lights would run ahead of.
int probe_sh(PTContext* c, const PTFrameParams& p1, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples, uint32_t flags,
             PTProbeCoeffs* dOut, const char* who)
{
    int rc;
    if ((rc = check_list_schedule(c, who, "probe"))) return rc;
    const uint32_t lightCount = (flags & PT_PROBE_DELTA_LIGHTS) && c->scene.hasLights && c->scene.lightCount > 0 ? (uint32_t)c->scene.lightCount : 0u;
    if (count && lightCount) {
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = trace_delta_lights(c, dProbes, count, lightCount))) return rc;
    }
    const PTContext::Probe& W = c->probe;
    return enqueue_list_chunks(c, p1, count, PT_RADIANCE_CHUNK / samples, samples, "PT SH probes (enqueue)", [&](uint64_t first, uint32_t n, PTWfLaunch& L) {
        L.mapKind = PT_WF_MAP_PROBE;
        L.probe.probes = dProbes + first;
        L.probe.entries = n;
        L.probe.samples = samples;
        L.probe.firstSample = firstSample;
        L.probe.lightCount = lightCount;
        if (lightCount) {
            L.probe.deltaRays = (const float4*)W.deltaRays.ptr + first * lightCount * 2u;
            L.probe.deltaLi = (const float4*)W.deltaLi.ptr + first * lightCount;
            L.probe.deltaHits = (const float4*)W.deltaHits.ptr + first * lightCount;
        }
        L.output = dOut + first;
    });
}

} // namespace

extern "C" {

PT_API int PTProbeSH(PTContext* c, const PTFrameParams* hostParams, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples,
                     uint32_t flags, PTProbeCoeffs* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeSH: ctx == NULL");
    PTFrameParams p1;
    if (int rc = import_sampled_params(hostParams, samples, "PTProbeSH", p1)) return rc;
    if (int rc = check_flags(flags, "PTProbeSH")) return rc;
    if (!dProbes || !dOut) return fail(PT_ERR_INVALID_ARG, "PTProbeSH: probes/out == NULL");
    if (misaligned(dProbes) || misaligned(dOut)) return fail(PT_ERR_INVALID_ARG, "PTProbeSH: probes/out is not 16-byte aligned");
    return probe_sh(c, p1, dProbes, count, firstSample, samples, flags, dOut, "PTProbeSH");
}

PT_API int PTProbeSHHost(PTContext* c, const PTFrameParams* hostParams, const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples,
                         uint32_t flags, PTProbeCoeffs* out)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeSHHost: ctx == NULL");
    PTFrameParams p1;
    int rc = import_sampled_params(hostParams, samples, "PTProbeSHHost", p1);
    if (rc) return rc;
    if ((rc = check_flags(flags, "PTProbeSHHost"))) return rc;
    if (!probes || !out) return fail(PT_ERR_INVALID_ARG, "PTProbeSHHost: probes/out == NULL");
    return host_round_trip(c, c->probe.host, probes, count, out, [&](const PTProbe* dProbes, PTProbeCoeffs* dOut) {
        return probe_sh(c, p1, dProbes, count, firstSample, samples, flags, dOut, "PTProbeSHHost");
    });
}

PT_API int PTProbeRays(PTContext* c, const PTFrameParams* hostParams, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples,
                       PTRadianceRay* dRays)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeRays: ctx == NULL");
    PTFrameParams p1;
    int rc = import_sampled_params(hostParams, samples, "PTProbeRays", p1);
    if (rc) return rc;
    if (!dProbes || !dRays) return fail(PT_ERR_INVALID_ARG, "PTProbeRays: probes/rays == NULL");
    if (misaligned(dProbes) || misaligned(dRays)) return fail(PT_ERR_INVALID_ARG, "PTProbeRays: probes/rays is not 16-byte aligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, (1ull << 30) / samples, [&](uint64_t first, uint32_t n) {       // whole probes, <= 2^30 slots per launch
        PTProbeMap pm = {};
        pm.probes = dProbes + first;
        pm.entries = n;
        pm.samples = samples;
        pm.firstSample = firstSample;
        HIP_TRY(pt_launch_probe_rays(pm, dRays + first * samples, c->stream));
        return PT_OK;
    });
}

PT_API int PTProbeIrradiance(PTContext* c, const PTProbeCoeffs* dSH, uint64_t probeCount, const PTProbeQuery* dQueries, uint64_t count, PTIrradiance* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeIrradiance: ctx == NULL");
    if (!dQueries || !dOut || (probeCount && !dSH)) return fail(PT_ERR_INVALID_ARG, "PTProbeIrradiance: sh/queries/out == NULL");
    if (misaligned(dSH) || misaligned(dQueries) || misaligned(dOut)) return fail(PT_ERR_INVALID_ARG, "PTProbeIrradiance: sh/queries/out is not 16-byte aligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_probe_irradiance(dSH, probeCount, dQueries + first, n, dOut + first, c->stream));
        return PT_OK;
    });
}

} // extern "C"
