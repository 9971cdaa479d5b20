// pt_api_gather.hip — irradiance gathers: the irradiance at a caller's list of receivers (include/ptmi_plugin.h Part 13;
// DESIGN.md 5.18).
#include "pt_context.h"

namespace {

bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0u; }

// what every entry point checks after the context: params, the sample count, the bounce limit.  p1: params with one sample per slot
int import_gather_params(const PTFrameParams* hostParams, uint32_t samples, const char* who, PTFrameParams& p1)
{
    if (!hostParams) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": params == NULL");
    if (int rc = import_frame_params(hostParams, p1)) return rc;
    p1.SamplesPerPass = 1;
    if (samples == 0u || samples > PT_GATHER_MAX_SAMPLES)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": samples = " + std::to_string(samples) + " (1 ... " + std::to_string(PT_GATHER_MAX_SAMPLES) + ")");
    if (p1.MaxRayBounces > 8191u) return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": MaxRayBounces > 8191 does not fit the packed path state");
    return PT_OK;
}

int check_schedule(PTContext* c, const char* who)
{
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    const int schedule = effective_schedule(c);
    if (schedule < 1 || schedule > 3)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": schedule " + std::to_string(schedule) + " has no pass over a receiver list (schedules 1, 2 and 3 do: PTSetSchedule)");
    return PT_OK;
}

// One launch sequence per chunk of floor(PT_RADIANCE_CHUNK / samples) whole entries, each on the next state set and its stream,
// exactly as trace_radiance enqueues the chunks of a ray list (pt_api_radiance.hip): ordered after what the context stream holds
// so far -- the receivers --, joined by the context stream after the last chunk.
int gather_irradiance(PTContext* c, const PTFrameParams& p1, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                      PTIrradiance* dOut, const char* who)
{
    RoctxRange range("PT irradiance gather (enqueue)");
    int rc;
    if ((rc = check_schedule(c, who))) return rc;
    uint32_t maxIterations;
    if ((rc = wavefront_limits(p1, maxIterations))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t perChunk = PT_RADIANCE_CHUNK / samples;           // >= 32 entries (samples <= 65536)
    uint32_t used = 0u;                 // bit k: set k carries a chunk of this call
    static_assert(PT_WF_SETS <= 32, "one bit per state set");
    static_assert(PT_GATHER_MAX_SAMPLES <= PT_RADIANCE_CHUNK, "a chunk holds at least one whole entry");
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
        L.mapKind = PT_WF_MAP_GATHER;
        L.gather.recv = dRecv + first;
        L.gather.entries = n;
        L.gather.samples = samples;
        L.gather.firstSample = firstSample;
        L.output = dOut + first;
        // the whole chain waits for what the context stream holds so far: its init kernel reads the caller's receivers
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

PT_API int PTGatherIrradiance(PTContext* c, const PTFrameParams* hostParams, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                              PTIrradiance* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradiance: ctx == NULL");
    PTFrameParams p1;
    if (int rc = import_gather_params(hostParams, samples, "PTGatherIrradiance", p1)) return rc;
    if (!dRecv || !dOut) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradiance: receivers/out == NULL");
    if (misaligned(dRecv) || misaligned(dOut)) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradiance: receivers/out is not 16-byte aligned");
    return gather_irradiance(c, p1, dRecv, count, firstSample, samples, dOut, "PTGatherIrradiance");
}

PT_API int PTGatherIrradianceHost(PTContext* c, const PTFrameParams* hostParams, const PTReceiver* recv, uint64_t count, uint32_t firstSample, uint32_t samples,
                                  PTIrradiance* out)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceHost: ctx == NULL");
    PTFrameParams p1;
    int rc = import_gather_params(hostParams, samples, "PTGatherIrradianceHost", p1);
    if (rc) return rc;
    if (!recv || !out) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceHost: receivers/out == NULL");
    for (uint64_t i = 0; i < count; ++i)
        if (recv[i].reserved != 0u) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceHost: receivers[" + std::to_string(i) + "].reserved != 0");
    PTContext::Gather& G = c->gather;
    if (count) {
        HIP_TRY(hipSetDevice(c->device));
        // the staging buffers regrow without a drain: every use of them ends in this call's final synchronise
        if ((rc = G.recv.reserve(count * sizeof(PTReceiver)))) return rc;
        if ((rc = G.out.reserve(count * sizeof(PTIrradiance)))) return rc;
        HIP_TRY(hipMemcpyAsync(G.recv.ptr, recv, count * sizeof(PTReceiver), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = gather_irradiance(c, p1, (const PTReceiver*)G.recv.ptr, count, firstSample, samples, (PTIrradiance*)G.out.ptr, "PTGatherIrradianceHost"))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipMemcpyAsync(out, G.out.ptr, count * sizeof(PTIrradiance), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

PT_API int PTGatherRays(PTContext* c, const PTFrameParams* hostParams, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                        PTRadianceRay* dRays)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGatherRays: ctx == NULL");
    PTFrameParams p1;
    int rc = import_gather_params(hostParams, samples, "PTGatherRays", p1);
    if (rc) return rc;
    if (!dRecv || !dRays) return fail(PT_ERR_INVALID_ARG, "PTGatherRays: receivers/rays == NULL");
    if (misaligned(dRecv) || misaligned(dRays)) return fail(PT_ERR_INVALID_ARG, "PTGatherRays: receivers/rays is not 16-byte aligned");
    if ((rc = check_schedule(c, "PTGatherRays"))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    // on the context stream, which every scene update joins (end_update): the step reads the lights and the environment
    const uint64_t perLaunch = (1ull << 30) / samples;               // whole entries, <= 2^30 slots per launch
    for (uint64_t first = 0; first < count; first += perLaunch) {
        PTGatherMap gm;
        gm.recv = dRecv + first;
        gm.entries = (uint32_t)(count - first < perLaunch ? count - first : perLaunch);
        gm.samples = samples;
        gm.firstSample = firstSample;
        HIP_TRY(pt_launch_gather_rays(c->scene, p1, gm, dRays + first * samples, c->stream));
    }
    return PT_OK;
}

} // extern "C"
