// pt_api_radiance.hip — radiance queries: the path-traced radiance along a caller's list of rays (include/ptmi_plugin.h Part 8;
// DESIGN.md 5.13).
#include "pt_context.h"

// One launch sequence per chunk of PT_RADIANCE_CHUNK rays (enqueue_list_chunks); PTReflectionCapture traces its slabs through it too
int trace_radiance(PTContext* c, const PTFrameParams& p, const PTRadianceRay* dRays, uint64_t count, PTRadiance* dOut, const char* who)
{
    if (int rc = check_list_schedule(c, who, "ray")) return rc;
    return enqueue_list_chunks(c, p, count, PT_RADIANCE_CHUNK, 1u, "PT radiance query (enqueue)", [&](uint64_t first, uint32_t n, PTWfLaunch& L) {
        L.mapKind = PT_WF_MAP_RAYS;
        L.rays.rays = dRays + first;
        L.rays.count = n;
        L.output = dOut + first;
    });
}

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
    // without a list entry i is pixel i: a launch past the first is never reached (count <= pixels < 2^29)
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_camera_rays(p, dPixelIndices ? dPixelIndices + first : nullptr, n, dRays + first, c->stream));
        return PT_OK;
    });
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
    if (int rc = import_frame_params(hostParams, p)) return rc;
    if (!rays || !out) return fail(PT_ERR_INVALID_ARG, "PTTraceRadianceHost: rays/out == NULL");
    for (uint64_t i = 0; i < count; ++i)
        if (rays[i].reserved != 0u) return fail(PT_ERR_INVALID_ARG, "PTTraceRadianceHost: rays[" + std::to_string(i) + "].reserved != 0");
    return host_round_trip(c, c->radiance, rays, count, out,
                           [&](const PTRadianceRay* dRays, PTRadiance* dOut) { return trace_radiance(c, p, dRays, count, dOut, "PTTraceRadianceHost"); });
}

} // extern "C"
