// pt_api_direct.hip — direct light at first hits: the pair count, the pairs' rays, the sum, the fused call, the mixed list call
// and a whole mixed frame (include/ptmi_plugin.h Part 24), and the same three through the context's light grid
// (Part 25).
#include "pt_context.h"
#include "direct_rule.h"

namespace {

int import_direct_params(const PTDirectParams* in, PTDirectParams& p, const char* who)
{
    std::string err;
    if (!ptdirect::check_params(in, err)) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": " + err);
    memset(&p, 0, sizeof(p));
    memcpy(&p, in, in->structSize < sizeof(p) ? in->structSize : sizeof(p));
    p.structSize = (uint32_t)sizeof(p);
    return PT_OK;
}

uint64_t pairs_per_entry(const PTContext* c, uint32_t strata)
{
    uint64_t pairs = 0;
    if (c->scene.hasLights)
        for (uint32_t type : c->update.lightTypes) pairs += ptdirect::pairs_of(type, strata);
    return pairs;
}

// grid: the context's light grid, which the entry point has found current (current_light_grid): the culled kernels (Part 25);
// null: the kernels that walk every light
int direct_light(PTContext* c, const PTDirectParams& p, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count, float4* dOut,
                 bool add, const PTLightGridDevice* grid = nullptr)
{
    if (int rc = query_prepare(c)) return rc;
    const int k = c->scene.hasTlas ? 1 : 0;
    uint32_t cap = c->query.directCaps[k];
    if (grid) {
        if (!c->query.culledCaps[0]) HIP_TRY(pt_direct_culled_grid_caps(c->device, c->query.culledCaps));
        cap = c->query.culledCaps[k] < c->query.capMax ? c->query.culledCaps[k] : c->query.capMax;      // the slab holds capMax waves
    }
    return for_each_launch(count, 1ull << 28, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_direct_light(c->scene, p, dRays + first, dHits + first, dSurface + first, n, (uint32_t)first, dOut + first, add,
                                       (uint2*)c->query.slab.ptr, cap, c->stream, grid));
        return PT_OK;
    });
}

// what the mixed calls hand their list call: the checked PTDirectParams and, for a culled call, the grid its entry point checked
struct MixedUser {
    PTDirectParams direct;
    bool culled;
    PTLightGridDevice grid;
};

// PTShadeLightmapped's launches, then pt_direct_light adding into dOut (a ShadeList; user: a MixedUser)
int shade_mixed(PTContext* c, const PTShadeInputs& in, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count, float4* dOut,
                const void* user)
{
    const PTDirectParams& direct = ((const MixedUser*)user)->direct;
    const PTLightGridDevice* grid = ((const MixedUser*)user)->culled ? &((const MixedUser*)user)->grid : nullptr;
    int rc = for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_shade_lightmapped(c->scene, in, c->lightmaps.device(), c->lightmaps.count, dRays + first, dHits + first, dSurface + first, n,
                                            dOut + first, c->stream));
        return PT_OK;
    });
    if (rc) return rc;
    if (pairs_per_entry(c, direct.strata) == 0u) return PT_OK;               // nothing to add: PTShadeLightmapped's bits
    return direct_light(c, direct, dRays, dHits, dSurface, count, dOut, true, grid);
}

// the bodies of the fused call, the mixed list call and the mixed frame; culled: through the context's light grid, checked here, once
int direct_light_call(PTContext* c, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count,
                      float* dOut, const char* who, bool culled)
{
    const std::string w(who);
    if (!c) return fail(PT_ERR_INVALID_ARG, w + ": ctx == NULL");
    PTDirectParams p;
    if (int rc = import_direct_params(params, p, who)) return rc;
    if (!dRays || !dHits || !dSurface || !dOut) return fail(PT_ERR_INVALID_ARG, w + ": rays/hits/surface/out == NULL");
    if (misaligned(dRays) || misaligned(dHits) || misaligned(dSurface) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, w + ": rays/hits/surface/out is not 16-byte aligned");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    PTLightGridDevice grid;
    if (culled)                                                         // also with count == 0: a stale grid is the caller's mistake
        if (int rc = current_light_grid(c, who, grid)) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("PT direct light (enqueue)");
    return direct_light(c, p, dRays, dHits, dSurface, count, (float4*)dOut, false, culled ? &grid : nullptr);
}

int shade_mixed_call(PTContext* c, const PTShadeInputs* inputs, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits,
                     const PTRaySurface* dSurface, uint64_t count, float* dOut, const char* who, bool culled)
{
    const std::string w(who);
    if (!c) return fail(PT_ERR_INVALID_ARG, w + ": ctx == NULL");
    if (int rc = check_shade_inputs(inputs, who)) return rc;
    MixedUser u = {{}, culled, {}};
    if (int rc = import_direct_params(params, u.direct, who)) return rc;
    if (!dRays || !dHits || !dSurface || !dOut) return fail(PT_ERR_INVALID_ARG, w + ": rays/hits/surface/out == NULL");
    if (misaligned(dRays) || misaligned(dHits) || misaligned(dSurface) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, w + ": rays/hits/surface/out is not 16-byte aligned");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (culled)
        if (int rc = current_light_grid(c, who, u.grid)) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return shade_mixed(c, *inputs, dRays, dHits, dSurface, count, (float4*)dOut, &u);
}

int shade_mixed_frame_call(PTContext* c, const PTFrameParams* hostParams, const PTShadeInputs* inputs, const PTDirectParams* direct, float* dOut,
                           PTRay* dOutRays, const char* who, bool culled)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": ctx == NULL");
    MixedUser u = {{}, culled, {}};
    if (int rc = import_direct_params(direct, u.direct, who)) return rc;
    if (culled && c->hasScene)                                          // before the frame's rays are made; without a scene shade_frame refuses
        if (int rc = current_light_grid(c, who, u.grid)) return rc;
    return shade_frame(c, hostParams, inputs, dOut, dOutRays, who, shade_mixed, &u);
}

} // namespace

extern "C" {

PT_API int PTDirectPairCount(PTContext* c, uint32_t strata, uint32_t* outPairsPerEntry)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTDirectPairCount: ctx == NULL");
    if (!outPairsPerEntry) return fail(PT_ERR_INVALID_ARG, "PTDirectPairCount: outPairsPerEntry == NULL");
    if (!ptdirect::strata_ok(strata))
        return fail(PT_ERR_INVALID_ARG, "PTDirectPairCount: strata = " + std::to_string(strata) + " (1 ... " + std::to_string(PT_DIRECT_MAX_STRATA) + ")");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    *outPairsPerEntry = (uint32_t)pairs_per_entry(c, strata);
    return PT_OK;
}

PT_API int PTDirectRays(PTContext* c, const PTDirectParams* params, const PTRay* dRays, const PTShadeTerms* dTerms, const PTReceiver* dRecv, uint64_t count,
                        PTRay* dOutRays, float* dOutContrib)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTDirectRays: ctx == NULL");
    PTDirectParams p;
    if (int rc = import_direct_params(params, p, "PTDirectRays")) return rc;
    if (!dRays || !dTerms || !dRecv) return fail(PT_ERR_INVALID_ARG, "PTDirectRays: rays/terms/receivers == NULL");
    if (misaligned(dRays) || misaligned(dTerms) || misaligned(dRecv) || misaligned(dOutRays) || misaligned(dOutContrib))
        return fail(PT_ERR_INVALID_ARG, "PTDirectRays: rays/terms/receivers/outputs is not 16-byte aligned");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    const uint64_t pairs = pairs_per_entry(c, p.strata);
    if (count == 0 || pairs == 0) return PT_OK;
    if (!dOutRays || !dOutContrib) return fail(PT_ERR_INVALID_ARG, "PTDirectRays: outRays/outContrib == NULL");
    if (count * pairs > (1ull << 31)) return fail(PT_ERR_INVALID_ARG, "PTDirectRays: count * pairsPerEntry > 2^31");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(pt_launch_direct_rays(c->scene, p, (uint32_t)pairs, dRays, dTerms, dRecv, (uint32_t)count, 0u, dOutRays, (float4*)dOutContrib, c->stream));
    return PT_OK;
}

PT_API int PTDirectAccumulate(PTContext* c, const PTShadeTerms* dTerms, const float* dContrib, const PTRayHit* dPairHits, uint64_t count,
                              uint32_t pairsPerEntry, float* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTDirectAccumulate: ctx == NULL");
    if (!dTerms || !dOut || (pairsPerEntry && (!dContrib || !dPairHits))) return fail(PT_ERR_INVALID_ARG, "PTDirectAccumulate: terms/contrib/hits/out == NULL");
    if (misaligned(dTerms) || misaligned(dContrib) || misaligned(dPairHits) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, "PTDirectAccumulate: terms/contrib/hits/out is not 16-byte aligned");
    if (count == 0) return PT_OK;
    if (count > (1ull << 31) || count * pairsPerEntry > (1ull << 31)) return fail(PT_ERR_INVALID_ARG, "PTDirectAccumulate: count * pairsPerEntry > 2^31");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(pt_launch_direct_accumulate(dTerms, (const float4*)dContrib, dPairHits, (uint32_t)count, pairsPerEntry, (float4*)dOut, c->stream));
    return PT_OK;
}

PT_API int PTDirectLight(PTContext* c, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count,
                         float* dOut)
{
    return direct_light_call(c, params, dRays, dHits, dSurface, count, dOut, "PTDirectLight", false);
}

PT_API int PTShadeMixed(PTContext* c, const PTShadeInputs* inputs, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits,
                        const PTRaySurface* dSurface, uint64_t count, float* dOut)
{
    return shade_mixed_call(c, inputs, params, dRays, dHits, dSurface, count, dOut, "PTShadeMixed", false);
}

PT_API int PTShadeMixedFrame(PTContext* c, const PTFrameParams* hostParams, const PTShadeInputs* inputs, const PTDirectParams* direct, float* dOut,
                             PTRay* dOutRays)
{
    return shade_mixed_frame_call(c, hostParams, inputs, direct, dOut, dOutRays, "PTShadeMixedFrame", false);
}

// ---- Part 25: the same calls through the context's light grid ----
PT_API int PTDirectLightCulled(PTContext* c, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface,
                               uint64_t count, float* dOut)
{
    return direct_light_call(c, params, dRays, dHits, dSurface, count, dOut, "PTDirectLightCulled", true);
}

PT_API int PTShadeMixedCulled(PTContext* c, const PTShadeInputs* inputs, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits,
                              const PTRaySurface* dSurface, uint64_t count, float* dOut)
{
    return shade_mixed_call(c, inputs, params, dRays, dHits, dSurface, count, dOut, "PTShadeMixedCulled", true);
}

PT_API int PTShadeMixedFrameCulled(PTContext* c, const PTFrameParams* hostParams, const PTShadeInputs* inputs, const PTDirectParams* direct, float* dOut,
                                   PTRay* dOutRays)
{
    return shade_mixed_frame_call(c, hostParams, inputs, direct, dOut, dOutRays, "PTShadeMixedFrameCulled", true);
}

} // extern "C"
