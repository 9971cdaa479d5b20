// pt_api_lightmap_shade.hip — first hits shaded from baked lightmaps: the binding table, the lookup alone, the fused call and a
// whole frame (include/ptmi_plugin.h Part 22).
#include "pt_context.h"
#include "lightmap_lookup_rule.h"

namespace {

int shade_lightmapped(PTContext* c, const PTShadeInputs& in, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count,
                      float4* dOut, const void* = nullptr)
{
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_shade_lightmapped(c->scene, in, c->lightmaps.device(), c->lightmaps.count, dRays + first, dHits + first, dSurface + first, n,
                                            dOut + first, c->stream));
        return PT_OK;
    });
}

} // namespace

extern "C" {

PT_API int PTBindLightmaps(PTContext* c, const PTLightmapBinding* bindings, uint32_t count)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTBindLightmaps: ctx == NULL");
    if (count && !bindings) return fail(PT_ERR_INVALID_ARG, "PTBindLightmaps: bindings == NULL");
    if (count > PT_LIGHTMAP_MAX_BINDINGS)
        return fail(PT_ERR_INVALID_ARG, "PTBindLightmaps: count = " + std::to_string(count) + " (at most " + std::to_string(PT_LIGHTMAP_MAX_BINDINGS) + ")");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    std::string err;
    // a flat scene has no instances: only 0xFFFFFFFF passes
    if (!ptlm::check_bindings(bindings, count, c->attrs.used / sizeof(PTTriangleAttributes), c->update.instanceCount, err))
        return fail(PT_ERR_INVALID_ARG, "PTBindLightmaps: " + err);
    if (count) {
        HIP_TRY(hipSetDevice(c->device));
        PTLightmapBinding table[PT_LIGHTMAP_MAX_BINDINGS];
        memset(table, 0, sizeof(table));
        memcpy(table, bindings, (size_t)count * sizeof(PTLightmapBinding));
        if (int rc = c->lightmaps.table.send(table, sizeof(table), c->stream)) return rc;      // the old table stays bound if this fails
    }
    c->lightmaps.count = count;
    return PT_OK;
}

PT_API int PTLightmapLookup(PTContext* c, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count, PTIrradiance* dOut,
                            uint32_t* dOutBinding)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTLightmapLookup: ctx == NULL");
    if (!dRays || !dHits || !dSurface || !dOut) return fail(PT_ERR_INVALID_ARG, "PTLightmapLookup: rays/hits/surface/out == NULL");
    if (misaligned(dRays) || misaligned(dHits) || misaligned(dSurface) || misaligned(dOut) || misaligned(dOutBinding, 4))
        return fail(PT_ERR_INVALID_ARG, "PTLightmapLookup: rays/hits/surface/out is not 16-byte aligned, or the binding words not 4-byte");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_lightmap_lookup(c->scene, c->lightmaps.device(), c->lightmaps.count, dRays + first, dHits + first, dSurface + first, n, dOut + first,
                                          dOutBinding ? dOutBinding + first : nullptr, c->stream));
        return PT_OK;
    });
}

PT_API int PTShadeLightmapped(PTContext* c, const PTShadeInputs* inputs, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface,
                              uint64_t count, float* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTShadeLightmapped: ctx == NULL");
    if (int rc = check_shade_inputs(inputs, "PTShadeLightmapped")) return rc;
    if (!dRays || !dHits || !dSurface || !dOut) return fail(PT_ERR_INVALID_ARG, "PTShadeLightmapped: rays/hits/surface/out == NULL");
    if (misaligned(dRays) || misaligned(dHits) || misaligned(dSurface) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, "PTShadeLightmapped: rays/hits/surface/out is not 16-byte aligned");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return shade_lightmapped(c, *inputs, dRays, dHits, dSurface, count, (float4*)dOut);
}

PT_API int PTShadeLightmappedFrame(PTContext* c, const PTFrameParams* hostParams, const PTShadeInputs* inputs, float* dOut, PTRay* dOutRays)
{
    return shade_frame(c, hostParams, inputs, dOut, dOutRays, "PTShadeLightmappedFrame", shade_lightmapped);
}

} // extern "C"
