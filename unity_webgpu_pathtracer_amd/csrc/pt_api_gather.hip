// pt_api_gather.hip — irradiance gathers: the irradiance at a caller's list of receivers (include/ptmi_plugin.h Part 13;
// DESIGN.md 5.18).
#include "pt_context.h"

// One launch sequence per chunk of floor(PT_RADIANCE_CHUNK / samples) whole entries (enqueue_list_chunks); also a round of
// PTGatherIrradianceAdaptive (pt_api_adaptive_gather.hip)
int gather_irradiance(PTContext* c, const PTFrameParams& p1, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                      PTIrradiance* dOut, const char* who)
{
    if (int rc = check_list_schedule(c, who, "receiver")) return rc;
    static_assert(PT_GATHER_MAX_SAMPLES <= PT_RADIANCE_CHUNK, "a chunk holds at least one whole entry");
    return enqueue_list_chunks(c, p1, count, PT_RADIANCE_CHUNK / samples, samples, "PT irradiance gather (enqueue)", [&](uint64_t first, uint32_t n, PTWfLaunch& L) {
        L.mapKind = PT_WF_MAP_GATHER;
        L.gather.recv = dRecv + first;
        L.gather.entries = n;
        L.gather.samples = samples;
        L.gather.firstSample = firstSample;
        L.output = dOut + first;
    });
}

extern "C" {

PT_API int PTGatherIrradiance(PTContext* c, const PTFrameParams* hostParams, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                              PTIrradiance* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradiance: ctx == NULL");
    PTFrameParams p1;
    if (int rc = import_sampled_params(hostParams, samples, "PTGatherIrradiance", p1)) return rc;
    if (!dRecv || !dOut) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradiance: receivers/out == NULL");
    if (misaligned(dRecv) || misaligned(dOut)) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradiance: receivers/out is not 16-byte aligned");
    return gather_irradiance(c, p1, dRecv, count, firstSample, samples, dOut, "PTGatherIrradiance");
}

PT_API int PTGatherIrradianceHost(PTContext* c, const PTFrameParams* hostParams, const PTReceiver* recv, uint64_t count, uint32_t firstSample, uint32_t samples,
                                  PTIrradiance* out)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceHost: ctx == NULL");
    PTFrameParams p1;
    if (int rc = import_sampled_params(hostParams, samples, "PTGatherIrradianceHost", p1)) return rc;
    if (!recv || !out) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceHost: receivers/out == NULL");
    for (uint64_t i = 0; i < count; ++i)
        if (recv[i].reserved != 0u) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceHost: receivers[" + std::to_string(i) + "].reserved != 0");
    return host_round_trip(c, c->gather, recv, count, out, [&](const PTReceiver* dRecv, PTIrradiance* dOut) {
        return gather_irradiance(c, p1, dRecv, count, firstSample, samples, dOut, "PTGatherIrradianceHost");
    });
}

PT_API int PTGatherRays(PTContext* c, const PTFrameParams* hostParams, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                        PTRadianceRay* dRays)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGatherRays: ctx == NULL");
    PTFrameParams p1;
    int rc = import_sampled_params(hostParams, samples, "PTGatherRays", p1);
    if (rc) return rc;
    if (!dRecv || !dRays) return fail(PT_ERR_INVALID_ARG, "PTGatherRays: receivers/rays == NULL");
    if (misaligned(dRecv) || misaligned(dRays)) return fail(PT_ERR_INVALID_ARG, "PTGatherRays: receivers/rays is not 16-byte aligned");
    if ((rc = check_list_schedule(c, "PTGatherRays", "receiver"))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    // on the context stream, which every scene update joins (end_update): the step reads the lights and the environment
    return for_each_launch(count, (1ull << 30) / samples, [&](uint64_t first, uint32_t n) {       // whole entries, <= 2^30 slots per launch
        const PTGatherMap gm = {dRecv + first, n, samples, firstSample};
        HIP_TRY(pt_launch_gather_rays(c->scene, p1, gm, dRays + first * samples, c->stream));
        return PT_OK;
    });
}

} // extern "C"
