// pt_api_query.hip — batched ray queries (include/ptmi_plugin.h Part 3).
#include "pt_context.h"

namespace {
// Ray queries.  Every query of a context runs on c->stream, so they share one stack slab; PTSetScene synchronises that stream
// before it replaces the scene.  Launches carry at most 2^28 rays: the ray index and the per-lane counters stay 32-bit.
constexpr uint64_t kQueryLaunchRays = 1ull << 28;

int check_query_flags(uint32_t flags)
{
    if (flags & ~(PT_QUERY_ANY_HIT | PT_QUERY_SURFACE)) return fail(PT_ERR_INVALID_ARG, "PTTraceRays: unknown flag bits " + std::to_string(flags));
    if ((flags & PT_QUERY_ANY_HIT) && (flags & PT_QUERY_SURFACE)) return fail(PT_ERR_INVALID_ARG, "PTTraceRays: PT_QUERY_SURFACE needs closest-hit queries (not PT_QUERY_ANY_HIT)");
    return PT_OK;
}

int trace_rays(PTContext* c, const PTRay* dRays, uint64_t count, uint32_t flags, PTRayHit* dHits, PTRaySurface* dSurface)
{
    int rc = query_prepare(c);
    if (rc) return rc;
    const uint32_t mode = (flags & PT_QUERY_SURFACE) ? 2u : (flags & PT_QUERY_ANY_HIT) ? 1u : 0u;
    const bool stats = c->statsLevel > 0;
    const uint32_t cap = c->query.caps[pt_query_kernel_index(c->scene.hasTlas != 0u, mode, stats)];
    return for_each_launch(count, kQueryLaunchRays, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_query(c->scene, (const float4*)(dRays + first), n, mode, stats, (float4*)(dHits + first),
                                mode == 2u ? (float4*)(dSurface + first) : nullptr, (uint2*)c->query.slab.ptr, cap, (unsigned long long*)c->dStats.ptr, c->stream));
        return PT_OK;
    });
}
} // namespace

int query_prepare(PTContext* c)
{
    PTContext::Query& q = c->query;
    if (q.slab.ptr) return PT_OK;
    HIP_TRY(pt_query_grid_caps(c->device, q.caps));
    HIP_TRY(pt_direct_grid_caps(c->device, q.directCaps));
    for (uint32_t cap : q.caps) q.capMax = cap > q.capMax ? cap : q.capMax;
    for (uint32_t cap : q.directCaps) q.capMax = cap > q.capMax ? cap : q.capMax;
    return q.slab.reserve((size_t)q.capMax * pt_resident_wave_slab_bytes());
}

extern "C" {

PT_API int PTTraceRays(PTContext* c, const PTRay* dRays, uint64_t count, uint32_t flags, PTRayHit* dHits, PTRaySurface* dSurface)
{
    int rc = check_query_flags(flags);
    if (rc) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTTraceRays: ctx == NULL");
    if (!dRays || !dHits) return fail(PT_ERR_INVALID_ARG, "PTTraceRays: rays/hits == NULL");
    if ((flags & PT_QUERY_SURFACE) && !dSurface) return fail(PT_ERR_INVALID_ARG, "PTTraceRays: PT_QUERY_SURFACE with surface == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("PT ray query (enqueue)");
    return trace_rays(c, dRays, count, flags, dHits, dSurface);
}

PT_API int PTTraceRaysHost(PTContext* c, const PTRay* rays, uint64_t count, uint32_t flags, PTRayHit* hits, PTRaySurface* surface)
{
    int rc = check_query_flags(flags);
    if (rc) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTTraceRaysHost: ctx == NULL");
    if (!rays || !hits) return fail(PT_ERR_INVALID_ARG, "PTTraceRaysHost: rays/hits == NULL");
    if ((flags & PT_QUERY_SURFACE) && !surface) return fail(PT_ERR_INVALID_ARG, "PTTraceRaysHost: PT_QUERY_SURFACE with surface == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    for (uint64_t i = 0; i < count; ++i)
        if (rays[i].reserved != 0u) return fail(PT_ERR_INVALID_ARG, "PTTraceRaysHost: rays[" + std::to_string(i) + "].reserved != 0");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("PT ray query (host)");
    const bool surf = (flags & PT_QUERY_SURFACE) != 0u;
    // not host_round_trip: a third buffer, and the surface records come back through a temporary.  The staging buffers regrow
    // without a drain for its reason
    PTContext::Query& q = c->query;
    if ((rc = q.rays.reserve(count * sizeof(PTRay)))) return rc;
    if ((rc = q.hits.reserve(count * sizeof(PTRayHit)))) return rc;
    if (surf && (rc = q.surface.reserve(count * sizeof(PTRaySurface)))) return rc;
    HIP_TRY(hipMemcpyAsync(q.rays.ptr, rays, count * sizeof(PTRay), hipMemcpyHostToDevice, c->stream));
    if ((rc = trace_rays(c, (const PTRay*)q.rays.ptr, count, flags, (PTRayHit*)q.hits.ptr, surf ? (PTRaySurface*)q.surface.ptr : nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(hits, q.hits.ptr, count * sizeof(PTRayHit), hipMemcpyDeviceToHost, c->stream));
    // surface records exist only where a closest hit was found: the rest of the caller's array is left as it was
    std::vector<PTRaySurface> tmp(surf ? count : 0);
    if (surf) HIP_TRY(hipMemcpyAsync(tmp.data(), q.surface.ptr, count * sizeof(PTRaySurface), hipMemcpyDeviceToHost, c->stream));     // not the null stream
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; surf && i < count; ++i) if (hits[i].prim != 0xFFFFFFFFu) surface[i] = tmp[i];
    return PT_OK;
}

} // extern "C"
