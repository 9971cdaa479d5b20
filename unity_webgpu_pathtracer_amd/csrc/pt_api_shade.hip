// pt_api_shade.hip — shading from the bakes: the split-sum DFG table, a hit's terms and lookup queries, the compose step, the
// fused call and a whole frame (include/ptmi_plugin.h Part 21).
#include "pt_context.h"
#include "shade_rule.h"

namespace {

int check_dfg(uint32_t res, const char* who)
{
    std::string err;
    if (!ptshade::check_dfg_res(res, err)) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": " + err);
    return PT_OK;
}

} // namespace

int check_shade_inputs(const PTShadeInputs* in, const char* who)
{
    const std::string w(who);
    if (!in) return fail(PT_ERR_INVALID_ARG, w + ": inputs == NULL");
    std::string err;
    if (!ptvol::check_grid(&in->grid, err) || !ptrefl::check_layout(in->res, in->levels, true, err)) return fail(PT_ERR_INVALID_ARG, w + ": " + err);
    if (int rc = check_dfg(in->dfgRes, who)) return rc;
    if (!in->dSH || !in->dDFG || (in->probeCount && (!in->dMaps || !in->dProbes))) return fail(PT_ERR_INVALID_ARG, w + ": sh/dfg/maps/probes == NULL");
    if ((in->grid.flags & PT_GRID_VISIBILITY) && !in->dDepth) return fail(PT_ERR_INVALID_ARG, w + ": PT_GRID_VISIBILITY with depth == NULL");
    if (in->dBoxes && !in->dProbes) return fail(PT_ERR_INVALID_ARG, w + ": boxes without probes (the choice and the projection need the probes' positions)");
    if (misaligned(in->dSH) || misaligned(in->dDepth) || misaligned(in->dPlacement) || misaligned(in->dMaps) || misaligned(in->dProbes) ||
        misaligned(in->dBoxes) || misaligned(in->dDFG, 8))
        return fail(PT_ERR_INVALID_ARG, w + ": sh/depth/placement/maps/probes/boxes is not 16-byte aligned, or the DFG table not 8-byte");
    return PT_OK;
}

namespace {

int shade_baked(PTContext* c, const PTShadeInputs& in, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count, float4* dOut,
                const void* = nullptr)
{
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_shade_baked(c->scene, in, dRays + first, dHits + first, dSurface + first, n, dOut + first, c->stream));
        return PT_OK;
    });
}

} // namespace

int shade_frame(PTContext* c, const PTFrameParams* hostParams, const PTShadeInputs* inputs, float* dOut, PTRay* dOutRays, const char* who, ShadeList shade,
                const void* user)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": ctx == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    if ((rc = check_shade_inputs(inputs, who))) return rc;
    if (!dOut || misaligned(dOut) || misaligned(dOutRays)) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": out == NULL, or out/rays is not 16-byte aligned");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("PT shade baked frame (enqueue)");
    if ((rc = query_prepare(c))) return rc;
    const uint64_t pixels = (uint64_t)p.OutputWidth * p.OutputHeight;
    PTContext::Shade& W = c->shade;
    // growing drains the context stream, which every earlier frame ran on
    if (!dOutRays && (rc = W.rays.reserve(pixels * sizeof(PTRay), c->stream))) return rc;
    if ((rc = W.hits.reserve(pixels * sizeof(PTRayHit), c->stream))) return rc;
    if ((rc = W.surfaces.reserve(pixels * sizeof(PTRaySurface), c->stream))) return rc;
    PTRay* rays = dOutRays ? dOutRays : (PTRay*)W.rays.ptr;
    const bool stats = c->statsLevel > 0;
    const uint32_t cap = c->query.caps[pt_query_kernel_index(c->scene.hasTlas != 0u, 2u, stats)];
    rc = for_each_launch(pixels, 1ull << 28, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_shade_frame_rays(p, (uint32_t)first, n, rays + first, c->stream));
        HIP_TRY(pt_launch_query(c->scene, (const float4*)(rays + first), n, 2u, stats, (float4*)((PTRayHit*)W.hits.ptr + first),
                                (float4*)((PTRaySurface*)W.surfaces.ptr + first), (uint2*)c->query.slab.ptr, cap, (unsigned long long*)c->dStats.ptr, c->stream));
        return PT_OK;
    });
    if (rc) return rc;
    return shade(c, *inputs, rays, (const PTRayHit*)W.hits.ptr, (const PTRaySurface*)W.surfaces.ptr, pixels, (float4*)dOut, user);
}

extern "C" {

PT_API int PTBakeDFG(PTContext* c, uint32_t res, PTShadeDFG* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTBakeDFG: ctx == NULL");
    if (int rc = check_dfg(res, "PTBakeDFG")) return rc;
    if (!dOut || misaligned(dOut, 8)) return fail(PT_ERR_INVALID_ARG, "PTBakeDFG: out == NULL or not 8-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(pt_launch_shade_dfg(res, dOut, c->stream));
    return PT_OK;
}

PT_API int PTShadeSurfaces(PTContext* c, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count, const PTProbe* dProbes,
                           const PTReflectionBox* dBoxes, uint32_t probeCount, PTShadeMaterial* dOutMaterial, PTShadeTerms* dOutTerms,
                           PTReceiver* dOutReceivers, PTReflectionQuery* dOutQueries)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTShadeSurfaces: ctx == NULL");
    if (!dRays || !dHits || !dSurface || (probeCount && !dProbes)) return fail(PT_ERR_INVALID_ARG, "PTShadeSurfaces: rays/hits/surface/probes == NULL");
    if (dBoxes && !dProbes) return fail(PT_ERR_INVALID_ARG, "PTShadeSurfaces: boxes without probes (the choice needs the probes' positions)");
    if (misaligned(dRays) || misaligned(dHits) || misaligned(dSurface) || misaligned(dProbes) || misaligned(dBoxes) || misaligned(dOutMaterial) ||
        misaligned(dOutTerms) || misaligned(dOutReceivers) || misaligned(dOutQueries))
        return fail(PT_ERR_INVALID_ARG, "PTShadeSurfaces: rays/hits/surface/probes/boxes/outputs is not 16-byte aligned");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_shade_surfaces(c->scene, dRays + first, dHits + first, dSurface + first, n, dProbes, dBoxes, probeCount,
                                         dOutMaterial ? dOutMaterial + first : nullptr, dOutTerms ? dOutTerms + first : nullptr,
                                         dOutReceivers ? dOutReceivers + first : nullptr, dOutQueries ? dOutQueries + first : nullptr, c->stream));
        return PT_OK;
    });
}

PT_API int PTShadeCompose(PTContext* c, const PTShadeTerms* dTerms, const PTIrradiance* dIrradiance, const PTReflectionTexel* dReflection, uint64_t count,
                          const PTShadeDFG* dDFG, uint32_t dfgRes, float* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTShadeCompose: ctx == NULL");
    if (int rc = check_dfg(dfgRes, "PTShadeCompose")) return rc;
    if (!dTerms || !dIrradiance || !dReflection || !dDFG || !dOut) return fail(PT_ERR_INVALID_ARG, "PTShadeCompose: terms/irradiance/reflection/dfg/out == NULL");
    if (misaligned(dTerms) || misaligned(dIrradiance) || misaligned(dReflection) || misaligned(dDFG, 8) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, "PTShadeCompose: terms/irradiance/reflection/out is not 16-byte aligned, or the DFG table not 8-byte");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return for_each_launch(count, 1ull << 30, [&](uint64_t first, uint32_t n) {
        HIP_TRY(pt_launch_shade_compose(dTerms + first, dIrradiance + first, dReflection + first, n, dDFG, dfgRes, (float4*)dOut + first, c->stream));
        return PT_OK;
    });
}

PT_API int PTShadeBaked(PTContext* c, const PTShadeInputs* inputs, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count,
                        float* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTShadeBaked: ctx == NULL");
    if (int rc = check_shade_inputs(inputs, "PTShadeBaked")) return rc;
    if (!dRays || !dHits || !dSurface || !dOut) return fail(PT_ERR_INVALID_ARG, "PTShadeBaked: rays/hits/surface/out == NULL");
    if (misaligned(dRays) || misaligned(dHits) || misaligned(dSurface) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, "PTShadeBaked: rays/hits/surface/out is not 16-byte aligned");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    return shade_baked(c, *inputs, dRays, dHits, dSurface, count, (float4*)dOut);
}

PT_API int PTShadeBakedFrame(PTContext* c, const PTFrameParams* hostParams, const PTShadeInputs* inputs, float* dOut, PTRay* dOutRays)
{
    return shade_frame(c, hostParams, inputs, dOut, dOutRays, "PTShadeBakedFrame", shade_baked);
}

} // extern "C"
