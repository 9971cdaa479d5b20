// pt_api_reflection.hip — reflection probes: octahedral radiance maps captured through the radiance query, prefiltered per
// roughness level and looked up with box projection (include/ptmi_plugin.h Part 20).
#include "pt_context.h"
#include "reflection_rule.h"

namespace {

int check_layout(uint32_t res, uint32_t levels, bool needLevels, const char* who)
{
    std::string err;
    if (!ptrefl::check_layout(res, levels, needLevels, err)) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": " + err);
    return PT_OK;
}

// what the three calls that make samples check before the context is used; p1: params with one sample per slot
int check_sampled(const PTFrameParams* hostParams, uint32_t res, uint32_t samples, const void* probes, const void* out, const char* who, PTFrameParams& p1)
{
    if (int rc = import_sampled_params(hostParams, samples, who, p1)) return rc;
    if (int rc = check_layout(res, 0u, false, who)) return rc;
    if (!probes || !out) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": probes/out == NULL");
    return PT_OK;
}

// One slab of floor(2^22 / samples) whole texels after another, all through the same scratch: the rays kernel on the context
// stream, the radiance query's launch sequences over the slab -- each behind what the context stream holds, and joined by it after
// the last one (enqueue_list_chunks) --, the fold on the context stream.  The next slab's rays kernel therefore runs behind this
// slab's fold.  No map kind of its own: the slab IS a ray list.
int reflection_capture(PTContext* c, const PTFrameParams& p1, const PTProbe* dProbes, uint64_t count, uint32_t res, uint32_t firstSample, uint32_t samples,
                       PTReflectionTexel* dOut, const char* who)
{
    RoctxRange range("PT reflection capture (enqueue)");
    int rc;
    if ((rc = check_list_schedule(c, who, "reflection probe"))) return rc;
    uint32_t maxIterations;
    if ((rc = wavefront_limits(p1, maxIterations))) return rc;        // before anything is launched, as trace_radiance would refuse it
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t texels = count * res * res;
    const uint64_t perSlab = ptrefl::kSlabSlots / samples;             // >= 64 texels (samples <= 65536)
    const uint64_t slots = (texels < perSlab ? texels : perSlab) * samples;
    PTContext::Reflection& W = c->reflection;
    // growing drains the context stream, which every earlier call's chunks have joined
    if ((rc = W.rays.reserve(slots * sizeof(PTRadianceRay), c->stream))) return rc;
    if ((rc = W.radiance.reserve(slots * sizeof(PTRadiance), c->stream))) return rc;
    return for_each_launch(texels, perSlab, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_refl_rays(dProbes, first, n, res, firstSample, samples, (PTRadianceRay*)W.rays.ptr, c->stream));
        if (int r = trace_radiance(c, p1, (const PTRadianceRay*)W.rays.ptr, (uint64_t)n * samples, (PTRadiance*)W.radiance.ptr, who)) return r;
        HIP_TRY(pt_launch_refl_fold((const PTRadiance*)W.radiance.ptr, n, samples, dOut + first, c->stream));
        return PT_OK;
    });
}

// false: the byte ranges [a, a + na) and [b, b + nb) are disjoint
bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

} // namespace

extern "C" {

PT_API int PTReflectionRays(PTContext* c, const PTFrameParams* hostParams, const PTProbe* dProbes, uint64_t count, uint32_t res, uint32_t firstSample,
                            uint32_t samples, PTRadianceRay* dRays)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTReflectionRays: ctx == NULL");
    PTFrameParams p1;
    if (int rc = check_sampled(hostParams, res, samples, dProbes, dRays, "PTReflectionRays", p1)) return rc;
    if (misaligned(dProbes) || misaligned(dRays)) return fail(PT_ERR_INVALID_ARG, "PTReflectionRays: probes/rays is not 16-byte aligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count * res * res, (1ull << 30) / samples, [&](uint64_t first, uint32_t n) {      // whole texels, <= 2^30 slots per launch
        HIP_TRY(pt_launch_refl_rays(dProbes, first, n, res, firstSample, samples, dRays + first * samples, c->stream));
        return PT_OK;
    });
}

PT_API int PTReflectionCapture(PTContext* c, const PTFrameParams* hostParams, const PTProbe* dProbes, uint64_t count, uint32_t res, uint32_t firstSample,
                               uint32_t samples, PTReflectionTexel* dOutBase)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTReflectionCapture: ctx == NULL");
    PTFrameParams p1;
    if (int rc = check_sampled(hostParams, res, samples, dProbes, dOutBase, "PTReflectionCapture", p1)) return rc;
    if (misaligned(dProbes) || misaligned(dOutBase)) return fail(PT_ERR_INVALID_ARG, "PTReflectionCapture: probes/out is not 16-byte aligned");
    return reflection_capture(c, p1, dProbes, count, res, firstSample, samples, dOutBase, "PTReflectionCapture");
}

// host_round_trip moves as many results as entries; here a probe gives res * res texels, so the same three steps are written out
PT_API int PTReflectionCaptureHost(PTContext* c, const PTFrameParams* hostParams, const PTProbe* probes, uint64_t count, uint32_t res, uint32_t firstSample,
                                   uint32_t samples, PTReflectionTexel* outBase)
{
    const char* who = "PTReflectionCaptureHost";
    if (!c) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": ctx == NULL");
    PTFrameParams p1;
    int rc;
    if ((rc = check_sampled(hostParams, res, samples, probes, outBase, who, p1))) return rc;
    HostStaging& s = c->reflection.host;
    const uint64_t texels = count * res * res;
    if (count) {
        HIP_TRY(hipSetDevice(c->device));
        // the staging regrows without a drain: every use of it ends in this call's final synchronise
        if ((rc = s.in.reserve(count * sizeof(PTProbe))) || (rc = s.out.reserve(texels * sizeof(PTReflectionTexel)))) return rc;
        HIP_TRY(hipMemcpyAsync(s.in.ptr, probes, count * sizeof(PTProbe), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = reflection_capture(c, p1, (const PTProbe*)s.in.ptr, count, res, firstSample, samples, (PTReflectionTexel*)s.out.ptr, who)) || count == 0) return rc;
    HIP_TRY(hipMemcpyAsync(outBase, s.out.ptr, texels * sizeof(PTReflectionTexel), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

PT_API int PTReflectionPrefilter(PTContext* c, const PTReflectionTexel* dBase, uint64_t count, uint32_t res, uint32_t levels, PTReflectionTexel* dOutMaps)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTReflectionPrefilter: ctx == NULL");
    if (int rc = check_layout(res, levels, true, "PTReflectionPrefilter")) return rc;
    if (!dBase || !dOutMaps) return fail(PT_ERR_INVALID_ARG, "PTReflectionPrefilter: base/out == NULL");
    if (misaligned(dBase) || misaligned(dOutMaps)) return fail(PT_ERR_INVALID_ARG, "PTReflectionPrefilter: base/out is not 16-byte aligned");
    const uint64_t baseTexels = (uint64_t)res * res, mapTexels = ptrefl::level_offset(res, levels);
    if (dBase == dOutMaps || overlap(dBase, count * baseTexels * sizeof(PTReflectionTexel), dOutMaps, count * mapTexels * sizeof(PTReflectionTexel)))
        return fail(PT_ERR_INVALID_ARG, "PTReflectionPrefilter: out aliases base");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, 32768u, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_refl_prefilter(dBase + first * baseTexels, n, res, levels, dOutMaps + first * mapTexels, c->stream));
        return PT_OK;
    });
}

PT_API int PTReflectionLookup(PTContext* c, const PTReflectionTexel* dMaps, uint64_t probeCount, uint32_t res, uint32_t levels, const PTProbe* dProbes,
                              const PTReflectionBox* dBoxes, const PTReflectionQuery* dQueries, uint64_t count, PTReflectionTexel* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTReflectionLookup: ctx == NULL");
    if (int rc = check_layout(res, levels, true, "PTReflectionLookup")) return rc;
    if (!dQueries || !dOut || (probeCount && !dMaps)) return fail(PT_ERR_INVALID_ARG, "PTReflectionLookup: maps/queries/out == NULL");
    if (dBoxes && !dProbes) return fail(PT_ERR_INVALID_ARG, "PTReflectionLookup: boxes without probes (the projection needs the probes' positions)");
    if (misaligned(dMaps) || misaligned(dProbes) || misaligned(dBoxes) || misaligned(dQueries) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, "PTReflectionLookup: maps/probes/boxes/queries/out is not 16-byte aligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_refl_lookup(dMaps, probeCount, res, levels, dProbes, dBoxes, dQueries + first, n, dOut + first, c->stream));
        return PT_OK;
    });
}

} // extern "C"
