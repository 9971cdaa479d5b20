// pt_api_probe.hip — SH light probes: nine spherical-harmonic coefficients per channel at a caller's list of positions, and their
// evaluation (include/ptmi_plugin.h Part 15).
#include "pt_context.h"

namespace {

bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0u; }

// what every entry point that makes samples checks after the context: params, the sample count, the bounce limit.  p1: params with
// one sample per slot
int import_probe_params(const PTFrameParams* hostParams, uint32_t samples, const char* who, PTFrameParams& p1)
{
    if (!hostParams) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": params == NULL");
    if (int rc = import_frame_params(hostParams, p1)) return rc;
    p1.SamplesPerPass = 1;
    if (samples == 0u || samples > PT_GATHER_MAX_SAMPLES)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": samples = " + std::to_string(samples) + " (1 ... " + std::to_string(PT_GATHER_MAX_SAMPLES) + ")");
    if (p1.MaxRayBounces > 8191u) return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": MaxRayBounces > 8191 does not fit the packed path state");
    return PT_OK;
}

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
    for (uint64_t first = 0; first < count; first += perLaunch) {
        const uint32_t n = (uint32_t)(count - first < perLaunch ? count - first : perLaunch);
        float4* rays = (float4*)W.deltaRays.ptr + first * lightCount * 2u;
        float4* li = (float4*)W.deltaLi.ptr + first * lightCount;
        float4* hits = (float4*)W.deltaHits.ptr + first * lightCount;
        HIP_TRY(pt_launch_probe_delta_rays(c->scene, dProbes + first, n, rays, li, c->stream));
        HIP_TRY(pt_launch_query(c->scene, rays, n * lightCount, PT_QUERY_ANY_HIT, stats, hits, nullptr, (uint2*)c->query.slab.ptr, cap,
                                (unsigned long long*)c->dStats.ptr, c->stream));
    }
    return PT_OK;
}

// One launch sequence per chunk of floor(PT_RADIANCE_CHUNK / samples) whole probes, each on the next state set and its stream,
// exactly as a gather enqueues its chunks (pt_api_gather.hip)
int probe_sh(PTContext* c, const PTFrameParams& p1, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples, uint32_t flags,
             PTProbeCoeffs* dOut, const char* who)
{
    RoctxRange range("PT SH probes (enqueue)");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    const int schedule = effective_schedule(c);
    if (schedule < 1 || schedule > 3)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": schedule " + std::to_string(schedule) + " has no pass over a probe list (schedules 1, 2 and 3 do: PTSetSchedule)");
    int rc;
    uint32_t maxIterations;
    if ((rc = wavefront_limits(p1, maxIterations))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t lightCount = (flags & PT_PROBE_DELTA_LIGHTS) && c->scene.hasLights && c->scene.lightCount > 0 ? (uint32_t)c->scene.lightCount : 0u;
    if (lightCount && (rc = trace_delta_lights(c, dProbes, count, lightCount))) return rc;
    const uint64_t perChunk = PT_RADIANCE_CHUNK / samples;           // >= 32 probes (samples <= 65536)
    uint32_t used = 0u;                 // bit k: set k carries a chunk of this call
    static_assert(PT_WF_SETS <= 32, "one bit per state set");
    for (uint64_t first = 0; first < count; first += perChunk) {
        const uint32_t n = (uint32_t)(count - first < perChunk ? count - first : perChunk);
        EventPair ep;
        if (c->profiling && (rc = take_event_pair(c, ep))) return rc;
        uint32_t k;
        PTContext::WfSet& set = next_wavefront_set(c, &k);
        used |= 1u << k;
        const uint32_t numSlots = (n * samples + 255u) & ~255u;
        if ((rc = ensure_wavefront(c, set, numSlots, maxIterations))) return rc;
        set.wf.slotsPerPass = numSlots;
        PTWfLaunch L = {};
        L.params = &p1;
        L.mapKind = PT_WF_MAP_PROBE;
        L.probe.probes = dProbes + first;
        L.probe.entries = n;
        L.probe.samples = samples;
        L.probe.firstSample = firstSample;
        L.probe.lightCount = lightCount;
        if (lightCount) {
            L.probe.deltaRays = (const float4*)c->probe.deltaRays.ptr + first * lightCount * 2u;
            L.probe.deltaLi = (const float4*)c->probe.deltaLi.ptr + first * lightCount;
            L.probe.deltaHits = (const float4*)c->probe.deltaHits.ptr + first * lightCount;
        }
        L.output = dOut + first;
        // the whole chain waits for what the context stream holds so far: the caller's probes and the delta lights' records
        HIP_TRY(hipEventRecord(set.callEv, c->stream));
        HIP_TRY(hipStreamWaitEvent(set.stream, set.callEv, 0));
        uint32_t launches = 0;
        if ((rc = enqueue_wavefront(c, set, L, c->profiling ? ep.start.h : nullptr, c->profiling ? ep.stop.h : nullptr, launches))) return rc;
        if (c->profiling) {
            ep.launches = launches;
            c->pending.push_back(std::move(ep));
        }
    }
    for (uint32_t k = 0; k < c->numSets; ++k)
        if (used & (1u << k)) HIP_TRY(hipStreamWaitEvent(c->stream, c->sets[k].done, 0));
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTProbeSH(PTContext* c, const PTFrameParams* hostParams, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples,
                     uint32_t flags, PTProbeCoeffs* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeSH: ctx == NULL");
    PTFrameParams p1;
    if (int rc = import_probe_params(hostParams, samples, "PTProbeSH", p1)) return rc;
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
    int rc = import_probe_params(hostParams, samples, "PTProbeSHHost", p1);
    if (rc) return rc;
    if ((rc = check_flags(flags, "PTProbeSHHost"))) return rc;
    if (!probes || !out) return fail(PT_ERR_INVALID_ARG, "PTProbeSHHost: probes/out == NULL");
    PTContext::Probe& W = c->probe;
    if (count) {
        HIP_TRY(hipSetDevice(c->device));
        // the staging buffers regrow without a drain: every use of them ends in this call's final synchronise
        if ((rc = W.probes.reserve(count * sizeof(PTProbe)))) return rc;
        if ((rc = W.out.reserve(count * sizeof(PTProbeCoeffs)))) return rc;
        HIP_TRY(hipMemcpyAsync(W.probes.ptr, probes, count * sizeof(PTProbe), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = probe_sh(c, p1, (const PTProbe*)W.probes.ptr, count, firstSample, samples, flags, (PTProbeCoeffs*)W.out.ptr, "PTProbeSHHost"))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipMemcpyAsync(out, W.out.ptr, count * sizeof(PTProbeCoeffs), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

PT_API int PTProbeRays(PTContext* c, const PTFrameParams* hostParams, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples,
                       PTRadianceRay* dRays)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeRays: ctx == NULL");
    PTFrameParams p1;
    int rc = import_probe_params(hostParams, samples, "PTProbeRays", p1);
    if (rc) return rc;
    if (!dProbes || !dRays) return fail(PT_ERR_INVALID_ARG, "PTProbeRays: probes/rays == NULL");
    if (misaligned(dProbes) || misaligned(dRays)) return fail(PT_ERR_INVALID_ARG, "PTProbeRays: probes/rays is not 16-byte aligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t perLaunch = (1ull << 30) / samples;               // whole probes, <= 2^30 slots per launch
    for (uint64_t first = 0; first < count; first += perLaunch) {
        PTProbeMap pm = {};
        pm.probes = dProbes + first;
        pm.entries = (uint32_t)(count - first < perLaunch ? count - first : perLaunch);
        pm.samples = samples;
        pm.firstSample = firstSample;
        HIP_TRY(pt_launch_probe_rays(pm, dRays + first * samples, c->stream));
    }
    return PT_OK;
}

PT_API int PTProbeIrradiance(PTContext* c, const PTProbeCoeffs* dSH, uint64_t probeCount, const PTProbeQuery* dQueries, uint64_t count, PTIrradiance* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTProbeIrradiance: ctx == NULL");
    if (!dQueries || !dOut || (probeCount && !dSH)) return fail(PT_ERR_INVALID_ARG, "PTProbeIrradiance: sh/queries/out == NULL");
    if (misaligned(dSH) || misaligned(dQueries) || misaligned(dOut)) return fail(PT_ERR_INVALID_ARG, "PTProbeIrradiance: sh/queries/out is not 16-byte aligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    constexpr uint64_t kPerLaunch = 1ull << 30;
    for (uint64_t first = 0; first < count; first += kPerLaunch) {
        const uint32_t n = (uint32_t)(count - first < kPerLaunch ? count - first : kPerLaunch);
        HIP_TRY(pt_launch_probe_irradiance(dSH, probeCount, dQueries + first, n, dOut + first, c->stream));
    }
    return PT_OK;
}

} // extern "C"
