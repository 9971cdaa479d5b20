// pt_api_radiance.hip — radiance queries: the path-traced radiance along a caller's list of rays (include/ptmi_plugin.h Part 8;
// DESIGN.md 5.13).
#include "pt_context.h"

namespace {

bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0u; }

// One launch sequence per chunk of PT_RADIANCE_CHUNK entries, each on the next state set and its stream (as a pass: render_to),
// ordered after what the caller has enqueued on the context stream so far -- the rays -- and before what it enqueues next.
// The context stream joins the sets only after the last chunk is enqueued, so the chunks of one call overlap as passes in flight
// do.  Two CALLS do not: the second one's rays are ordered after the stream's tail, and that is the first one's join.
int trace_radiance(PTContext* c, const PTFrameParams& p, const PTRadianceRay* dRays, uint64_t count, PTRadiance* dOut, const char* who)
{
    RoctxRange range("PT radiance query (enqueue)");
    int rc;
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    const int schedule = effective_schedule(c);
    if (schedule < 1 || schedule > 3)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": schedule " + std::to_string(schedule) + " has no pass over a ray list (schedules 1, 2 and 3 do: PTSetSchedule)");
    uint32_t maxIterations;
    if ((rc = wavefront_limits(p, maxIterations))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t used = 0u;                 // bit k: set k carries a chunk of this call
    static_assert(PT_WF_SETS <= 32, "one bit per state set");
    for (uint64_t first = 0; first < count; first += PT_RADIANCE_CHUNK) {
        const uint32_t n = (uint32_t)(count - first < PT_RADIANCE_CHUNK ? count - first : PT_RADIANCE_CHUNK);
        EventPair ep;
        if (c->profiling && (rc = take_event_pair(c, ep))) return rc;
        uint32_t k;
        PTContext::WfSet& set = next_wavefront_set(c, &k);
        used |= 1u << k;
        const uint32_t numSlots = (n + 255u) & ~255u;
        // the arena only ever grows; a list of another length is a new carving of the same memory (ensure_wavefront)
        if ((rc = ensure_wavefront(c, set, numSlots, maxIterations))) return rc;
        set.wf.slotsPerPass = numSlots;
        PTWfLaunch L = {};
        L.params = &p;
        L.mapKind = PT_WF_MAP_RAYS;
        L.rays.rays = dRays + first;
        L.rays.count = n;
        L.output = dOut + first;
        // unlike a pass, the WHOLE chain waits for what the context stream holds so far: its init kernel reads the caller's rays
        HIP_TRY(hipEventRecord(set.callEv, c->stream));
        HIP_TRY(hipStreamWaitEvent(set.stream, set.callEv, 0));
        uint32_t launches = 0;
        if ((rc = enqueue_wavefront(c, set, L, c->profiling ? ep.start.h : nullptr, c->profiling ? ep.stop.h : nullptr, launches))) return rc;
        if (c->profiling) {
            ep.launches = launches;
            c->pending.push_back(std::move(ep));
        }
    }
    // joined after the last chunk, not per sequence: the chunks of a call overlap.  Consumers of the context stream then see every
    // entry's result (a set that carried several chunks: its last record covers them)
    for (uint32_t k = 0; k < c->numSets; ++k)
        if (used & (1u << k)) HIP_TRY(hipStreamWaitEvent(c->stream, c->sets[k].done, 0));
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTCameraRays(PTContext* c, const PTFrameParams* hostParams, const uint32_t* dPixelIndices, uint64_t count, PTRadianceRay* dRays)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTCameraRays: ctx == NULL");
    if (!hostParams) return fail(PT_ERR_INVALID_ARG, "PTCameraRays: params == NULL");
    PTFrameParams p;
    if (int rc = import_frame_params(hostParams, p)) return rc;
    if (!dRays) return fail(PT_ERR_INVALID_ARG, "PTCameraRays: rays == NULL");
    if (misaligned(dRays)) return fail(PT_ERR_INVALID_ARG, "PTCameraRays: rays is not 16-byte aligned");
    const uint64_t pixels = (uint64_t)p.OutputWidth * p.OutputHeight;
    if (!dPixelIndices && count > pixels)
        return fail(PT_ERR_INVALID_ARG, "PTCameraRays: count " + std::to_string(count) + " exceeds the " + std::to_string(pixels) + " pixels of the frame (pixel indices == NULL)");
    HIP_TRY(hipSetDevice(c->device));
    constexpr uint64_t kLaunch = 1ull << 30;
    for (uint64_t first = 0; first < count; first += kLaunch) {
        const uint32_t n = (uint32_t)(count - first < kLaunch ? count - first : kLaunch);
        // without a list entry i is pixel i: a launch past the first is never reached (count <= pixels < 2^29)
        HIP_TRY(pt_launch_camera_rays(p, dPixelIndices ? dPixelIndices + first : nullptr, n, dRays + first, c->stream));
    }
    return PT_OK;
}

PT_API int PTTraceRadiance(PTContext* c, const PTFrameParams* hostParams, const PTRadianceRay* dRays, uint64_t count, PTRadiance* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTTraceRadiance: ctx == NULL");
    if (!hostParams) return fail(PT_ERR_INVALID_ARG, "PTTraceRadiance: params == NULL");
    PTFrameParams p;
    if (int rc = import_frame_params(hostParams, p)) return rc;
    if (!dRays || !dOut) return fail(PT_ERR_INVALID_ARG, "PTTraceRadiance: rays/out == NULL");
    if (misaligned(dRays) || misaligned(dOut)) return fail(PT_ERR_INVALID_ARG, "PTTraceRadiance: rays/out is not 16-byte aligned");
    return trace_radiance(c, p, dRays, count, dOut, "PTTraceRadiance");
}

PT_API int PTTraceRadianceHost(PTContext* c, const PTFrameParams* hostParams, const PTRadianceRay* rays, uint64_t count, PTRadiance* out)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTTraceRadianceHost: ctx == NULL");
    if (!hostParams) return fail(PT_ERR_INVALID_ARG, "PTTraceRadianceHost: params == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    if (!rays || !out) return fail(PT_ERR_INVALID_ARG, "PTTraceRadianceHost: rays/out == NULL");
    for (uint64_t i = 0; i < count; ++i)
        if (rays[i].reserved != 0u) return fail(PT_ERR_INVALID_ARG, "PTTraceRadianceHost: rays[" + std::to_string(i) + "].reserved != 0");
    PTContext::Radiance& R = c->radiance;
    if (count) {
        HIP_TRY(hipSetDevice(c->device));
        // the staging buffers regrow without a drain: every use of them ends in this call's final synchronise
        if ((rc = R.rays.reserve(count * sizeof(PTRadianceRay)))) return rc;
        if ((rc = R.out.reserve(count * sizeof(PTRadiance)))) return rc;
        HIP_TRY(hipMemcpyAsync(R.rays.ptr, rays, count * sizeof(PTRadianceRay), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = trace_radiance(c, p, (const PTRadianceRay*)R.rays.ptr, count, (PTRadiance*)R.out.ptr, "PTTraceRadianceHost"))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipMemcpyAsync(out, R.out.ptr, count * sizeof(PTRadiance), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

} // extern "C"
