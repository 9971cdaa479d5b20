// plugin_exports.cpp — Part 1 of include/ptmi_plugin.h: the acceleration-structure exports the Unity C#
// host binds (Assets/Scripts/util/TinyBVH.cs:15-50), replacing Assets/Plugins/Web/plugin.cpp.
//
// Same handle semantics as the reference: a handle is the index of the first free slot of a global
// table (plugin.cpp:8-21, 90-103), Destroy* frees and nulls the slot, invalid handles read as 0 / NULL.
// Differences, all on the safe side: degenerate input returns -1 instead of exit(1)
// (tiny_bvh.h:1615-1618), and "bool" results are full-width ints.
#include <chrono>
#include <cstddef>
#include <deque>
#include <string>
#include <algorithm>
#include "bvh_builder.h"
#include "bvh_refit.h"
#include "bvh_quality.h"
#include "skin_rule.h"
#include "morph_rule.h"
#include "chart_rule.h"
#include "sh_rule.h"
#include "volume_rule.h"
#include "placement_rule.h"
#include "lmfilter_rule.h"
#include "adaptive_gather_rule.h"
#include "reflection_rule.h"
#include "shade_rule.h"
#include "lightmap_lookup_rule.h"
#include "repack_rule.h"
#include "unwrap_rule.h"
#include "direct_rule.h"
#include "light_grid_rule.h"
#include "ptmi_plugin.h"

namespace {
std::deque<ptbvh::Cwbvh*> g_bvhs;
std::deque<ptbvh::Tlas*> g_tlases;

template <class T> int add_slot(std::deque<T*>& table, T* obj)
{
    for (size_t i = 0; i < table.size(); ++i)
        if (table[i] == nullptr) { table[i] = obj; return (int)i; }
    table.push_back(obj);
    return (int)table.size() - 1;
}
template <class T> T* get_slot(std::deque<T*>& table, int index)
{
    return (index >= 0 && index < (int)table.size()) ? table[index] : nullptr;
}
template <class T> void free_slot(std::deque<T*>& table, int index)
{
    if (index >= 0 && index < (int)table.size() && table[index]) { delete table[index]; table[index] = nullptr; }
}
} // namespace

extern "C" {

PT_API int BuildBVH(const PTFloat4* vertices, int triangleCount)
{
    if (!vertices || triangleCount <= 0) return -1;
    ptbvh::Cwbvh* bvh = new ptbvh::Cwbvh();
    const auto t0 = std::chrono::steady_clock::now();
    if (!bvh->build(vertices, (uint32_t)triangleCount)) { delete bvh; return -1; }
    bvh->buildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return add_slot(g_bvhs, bvh);
}

// The builder that runs on the MI355X (bvh_builder_gpu.hip).  Same handle table as BuildBVH: every Get* / DestroyBVH export
// works on the handle.  -1 on degenerate input or when there is no such HIP device (no CPU fallback: BuildBVH is the CPU path).
namespace { std::string g_buildError; }
PT_API int PTBuildBVHDevice(int deviceIndex, const PTFloat4* vertices, int triangleCount)
{
    if (!vertices || triangleCount <= 0) { g_buildError = "vertices == NULL or triangleCount <= 0"; return -1; }
    ptbvh::Cwbvh* bvh = new ptbvh::Cwbvh();
    if (!ptbvh::build_cwbvh_device(deviceIndex, vertices, (uint32_t)triangleCount, *bvh, &bvh->buildMs, g_buildError)) { delete bvh; return -1; }
    g_buildError.clear();
    return add_slot(g_bvhs, bvh);
}
PT_API const char* PTGetBVHBuildError(void) { return g_buildError.c_str(); }
PT_API double PTGetBVHBuildMs(int index)
{
    ptbvh::Cwbvh* b = get_slot(g_bvhs, index);
    return b ? b->buildMs : -1.0;
}
// Refit in place (bvh_refit.cpp): the handle keeps its topology, GetCWBVHData returns the refitted arrays.  No GPU involved.
PT_API int PTRefitBVH(int index, const PTFloat4* vertices, int triangleCount)
{
    ptbvh::Cwbvh* b = get_slot(g_bvhs, index);
    if (!b) { g_buildError = "no such BVH handle"; return 0; }
    if (!vertices || triangleCount <= 0 || (uint32_t)triangleCount != b->triCount) { g_buildError = "vertices == NULL or triangleCount is not the handle's"; return 0; }
    if (!ptbvh::refit_cwbvh(b->nodeData.data(), b->usedBlocks / 5u, b->triData.data(), (uint64_t)b->triCount * 3u, 0, 0, vertices, b->triCount, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// The same on arrays the host copied out of a handle (the reference's host destroys the handle right after the copy)
PT_API int PTRefitBVHArrays(PTFloat4* bvhNodes, uint64_t nodeBytes, PTFloat4* bvhTris, uint64_t triBytes, const PTFloat4* vertices, int triangleCount)
{
    if (!bvhNodes || !bvhTris || !vertices || triangleCount <= 0 || nodeBytes < 80 || nodeBytes % 80 || triBytes != (uint64_t)triangleCount * 48u) {
        g_buildError = "NULL array, nodeBytes not a multiple of 80 or triBytes != triangleCount * 48";
        return 0;
    }
    if (!ptbvh::refit_cwbvh(bvhNodes, nodeBytes / 80u, bvhTris, triBytes / 16u, 0, 0, vertices, (uint32_t)triangleCount, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// Tree quality of such arrays (bvh_quality.cpp; Part 10 has the rule).  No GPU involved.
PT_API int PTMeasureBVHArrays(const PTFloat4* bvhNodes, uint64_t nodeBytes, const PTFloat4* bvhTris, uint64_t triBytes, int triangleCount, PTGeometryQuality* out)
{
    if (!bvhNodes || !bvhTris || !out || triangleCount <= 0 || nodeBytes < 80 || nodeBytes % 80 || triBytes != (uint64_t)triangleCount * 48u) {
        g_buildError = "NULL array or result, nodeBytes not a multiple of 80 or triBytes != triangleCount * 48";
        return 0;
    }
    if (out->structSize < sizeof(PTGeometryQuality) || out->structSize > 4096u) {
        g_buildError = "PTGeometryQuality.structSize is not set (must be sizeof(PTGeometryQuality) of the host's header)";
        return 0;
    }
    ptbvh::Quality q;
    if (!ptbvh::measure_cwbvh(bvhNodes, nodeBytes / 80u, bvhTris, triBytes / 16u, (uint32_t)triangleCount, q, g_buildError)) return 0;
    out->nodeCapacity = q.nodeCapacity; out->nodeCount = q.nodeCount; out->triangleCount = q.triangleCount; out->levels = q.levels;
    out->reserved = 0;
    out->rootHalfArea = q.rootHalfArea; out->sahCost = q.sahCost;
    g_buildError.clear();
    return 1;
}
// Linear-blend skinning on the host (skin_host.cpp; Part 11 has the rule).  No GPU involved.
PT_API int PTSkinVerticesHost(const PTSkinDesc* desc, int triangleCount, const float* jointMatrices, PTFloat4* outVertices,
                              PTTriangleAttributes* outAttrsOrNull, float* outBoundsOrNull)
{
    if (!desc || !jointMatrices || !outVertices || triangleCount <= 0) { g_buildError = "NULL desc, matrices or result, or triangleCount <= 0"; return 0; }
    if (desc->structSize < sizeof(PTSkinDesc) || desc->structSize > 4096u) {
        g_buildError = "PTSkinDesc.structSize is not set (must be sizeof(PTSkinDesc) of the host's header)";
        return 0;
    }
    if (outAttrsOrNull && !desc->restAttrs) { g_buildError = "outAttrs needs PTSkinDesc.restAttrs"; return 0; }
    if (!ptskin::skin_check(*desc, (uint32_t)triangleCount, 0xFFFFFFFFu, g_buildError)) return 0;
    if (!ptskin::skin_check_palette(jointMatrices, desc->jointCount, g_buildError)) return 0;
    ptskin::skin_host(*desc, (uint32_t)triangleCount, jointMatrices, outVertices, outAttrsOrNull, outBoundsOrNull);
    g_buildError.clear();
    return 1;
}
// Morph targets, then the skin, on the host (morph_host.cpp; Part 12 has the rule).  No GPU involved.
PT_API int PTMorphVerticesHost(const PTMorphDesc* desc, const PTSkinDesc* skinOrNull, int triangleCount, const float* weights, const float* jointMatricesOrNull,
                               PTFloat4* outVertices, PTTriangleAttributes* outAttrsOrNull, float* outBoundsOrNull)
{
    if (!desc || !weights || !outVertices || triangleCount <= 0) { g_buildError = "NULL desc, weights or result, or triangleCount <= 0"; return 0; }
    if (desc->structSize < sizeof(PTMorphDesc) || desc->structSize > 4096u) {
        g_buildError = "PTMorphDesc.structSize is not set (must be sizeof(PTMorphDesc) of the host's header)";
        return 0;
    }
    if (skinOrNull && (skinOrNull->structSize < sizeof(PTSkinDesc) || skinOrNull->structSize > 4096u)) {
        g_buildError = "PTSkinDesc.structSize is not set (must be sizeof(PTSkinDesc) of the host's header)";
        return 0;
    }
    if (jointMatricesOrNull && !skinOrNull) { g_buildError = "a palette needs a skin"; return 0; }
    if (outAttrsOrNull && !desc->restAttrs) { g_buildError = "outAttrs needs PTMorphDesc.restAttrs"; return 0; }
    if (!ptmorph::morph_check(*desc, (uint32_t)triangleCount, 0xFFFFFFFFu, g_buildError)) return 0;
    if (!ptmorph::morph_check_weights(weights, desc->targetCount, g_buildError)) return 0;
    if (jointMatricesOrNull) {
        if (!ptskin::skin_check(*skinOrNull, (uint32_t)triangleCount, 0xFFFFFFFFu, g_buildError)) return 0;
        if (!ptskin::skin_check_palette(jointMatricesOrNull, skinOrNull->jointCount, g_buildError)) return 0;
    }
    ptmorph::morph_host(*desc, skinOrNull, (uint32_t)triangleCount, weights, jointMatricesOrNull, outVertices, outAttrsOrNull, outBoundsOrNull);
    g_buildError.clear();
    return 1;
}
// PTSetMorph's conversion of one CSR stream into the layout the kernels read (morph_host.cpp), for tests.  The stream is not checked here.
PT_API uint64_t PTMorphLayoutHost(const uint32_t* offsets, const PTMorphEntry* entries, uint32_t cornerCount, uint32_t* outCount, uint32_t* outSliceBase,
                                  PTMorphEntry* outEntries)
{
    if (!offsets) return 0;
    const uint64_t stored = ptmorph::morph_layout_size(offsets, cornerCount);
    if (stored > 0xFFFFFFFFull) return UINT64_MAX;
    if (!outCount && !outSliceBase && !outEntries) return stored;
    ptmorph::MorphLayout L;
    ptmorph::morph_layout(offsets, entries, cornerCount, L);
    if (outCount) std::copy(L.count.begin(), L.count.end(), outCount);
    if (outSliceBase) std::copy(L.sliceBase.begin(), L.sliceBase.end(), outSliceBase);
    if (outEntries) std::copy(L.entries.begin(), L.entries.end(), outEntries);
    return stored;
}
// Lightmap charts on the host (chart_host.cpp; Part 14 has the rule).  No GPU involved.
PT_API int PTRasterizeChartHost(const PTChartDesc* desc, const PTFloat4* tris, const PTTriangleAttributes* attrs, const float* uvsOrNull,
                                const float* localToWorldOrNull, const float* worldToLocalOrNull, uint32_t* texels, PTReceiver* recv, uint64_t capacity,
                                uint64_t* count)
{
    if (!desc || !count) { g_buildError = "NULL desc or count"; return 0; }
    *count = 0;
    if (desc->structSize < sizeof(PTChartDesc) || desc->structSize > 4096u) {
        g_buildError = "PTChartDesc.structSize is not set (must be sizeof(PTChartDesc) of the host's header)";
        return 0;
    }
    if (desc->triangleCount <= 0) { g_buildError = "triangleCount <= 0"; return 0; }
    if (desc->reserved[0] || desc->reserved[1] || desc->reserved[2]) { g_buildError = "PTChartDesc.reserved != 0"; return 0; }
    const ptchart::ChartInput in = {tris, attrs, uvsOrNull, localToWorldOrNull, worldToLocalOrNull, (uint32_t)desc->triangleCount, desc->width, desc->height,
                                    desc->seedBase};
    if (!ptchart::chart_rasterize_host(in, texels, recv, capacity, *count, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTResolveLightmapHost(const uint32_t* texels, const PTIrradiance* irr, uint64_t count, uint32_t width, uint32_t height, uint32_t dilate, void* image)
{
    if (!ptchart::chart_resolve_host(texels, irr, count, width, height, dilate, (float*)image, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// SH light probes on the host (probe_host.cpp; Part 15 has the rule).  No GPU involved.
PT_API int PTProbeDirectionsHost(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, PTRadianceRay* rays)
{
    if (!ptsh::probe_directions_host(probes, count, firstSample, samples, rays, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTProbeProjectHost(const float* directions, const float* colours, uint64_t count, uint32_t samples, PTProbeCoeffs* out)
{
    if (!ptsh::probe_project_host(directions, colours, count, samples, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTProbeIrradianceHost(const PTProbeCoeffs* sh, uint64_t probeCount, const PTProbeQuery* queries, uint64_t count, PTIrradiance* out)
{
    if (!ptsh::probe_irradiance_host(sh, probeCount, queries, count, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// Probe volumes on the host (volume_host.cpp; Part 16 has the rule).  No GPU involved.
PT_API int PTProbeDepthProjectHost(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const float* distances,
                                   float maxDistance, PTProbeDepthMap* out)
{
    if (!ptvol::depth_project_host(probes, count, firstSample, samples, distances, maxDistance, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTProbeGridIrradianceHost(const PTProbeGrid* grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTReceiver* queries,
                                     uint64_t count, PTIrradiance* out)
{
    if (!ptvol::grid_irradiance_host(grid, sh, depth, queries, count, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// Probe placement on the host (placement_host.cpp; Part 18 has the rule).  No GPU involved.
PT_API int PTProbePlaceStepHost(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const PTProbePlaceParams* params,
                                const PTRayHit* hits, const PTRaySurface* surfaces, int move, PTProbePlacement* inout, PTProbePlaceStats* stats)
{
    if (!ptplace::place_step_host(probes, count, firstSample, samples, params, hits, surfaces, move, inout, stats, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTProbeGridIrradiancePlacedHost(const PTProbeGrid* grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTProbePlacement* placement,
                                           const PTReceiver* queries, uint64_t count, PTIrradiance* out)
{
    if (!ptplace::grid_irradiance_placed_host(grid, sh, depth, placement, queries, count, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// The lightmap denoiser on the host (lmfilter_host.cpp; Part 17 has the rule).  No GPU involved.
PT_API int PTDenoiseLightmapHost(const PTLightmapDenoiseParams* params, const uint32_t* texels, const PTReceiver* recv, const PTIrradiance* irr, uint64_t count,
                                 uint32_t width, uint32_t height, PTIrradiance* out)
{
    if (!ptlmf::denoise_host(params, texels, recv, irr, count, width, height, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// The steps of an adaptive gather on the host (adaptive_gather_host.cpp; Part 19 has the rule).  No GPU involved.
PT_API int PTSelectReceiversHost(const PTAdaptiveGather* adaptive, uint32_t n, const uint32_t* active, uint64_t activeCount, const PTIrradiance* acc,
                                 const PTReceiver* recv, uint64_t entryCount, uint32_t* outActive, PTReceiver* outRecv, uint64_t* survivors, uint64_t* stopped)
{
    if (!ptag::select_host(adaptive, n, active, activeCount, acc, recv, entryCount, outActive, outRecv, survivors, stopped, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTFoldIrradianceHost(const uint32_t* active, uint64_t activeCount, const PTIrradiance* fresh, uint32_t m, uint32_t n, uint64_t entryCount,
                                PTIrradiance* acc, uint32_t* counts)
{
    if (!ptag::fold_host(active, activeCount, fresh, m, n, entryCount, acc, counts, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTEqualiseIrradianceHost(const PTIrradiance* irr, const uint32_t* counts, uint64_t count, uint32_t samplesEq, PTIrradiance* out)
{
    if (!ptag::equalise_host(irr, counts, count, samplesEq, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// Reflection probes on the host (reflection_host.cpp; Part 20 has the rule).  No GPU involved.
PT_API int PTReflectionDirectionsHost(const PTProbe* probes, uint64_t count, uint32_t res, uint32_t firstSample, uint32_t samples, PTRadianceRay* rays)
{
    if (!ptrefl::directions_host(probes, count, res, firstSample, samples, rays, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTReflectionFoldHost(const PTRadiance* radiance, uint64_t count, uint32_t res, uint32_t samples, PTReflectionTexel* out)
{
    if (!ptrefl::fold_host(radiance, count, res, samples, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTReflectionPrefilterHost(const PTReflectionTexel* base, uint64_t count, uint32_t res, uint32_t levels, PTReflectionTexel* outMaps)
{
    if (!ptrefl::prefilter_host(base, count, res, levels, outMaps, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTReflectionLookupHost(const PTReflectionTexel* maps, uint64_t probeCount, uint32_t res, uint32_t levels, const PTProbe* probes,
                                  const PTReflectionBox* boxes, const PTReflectionQuery* queries, uint64_t count, PTReflectionTexel* out)
{
    if (!ptrefl::lookup_host(maps, probeCount, res, levels, probes, boxes, queries, count, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// The slot-repack rule on the host (repack_host.cpp; repack_rule.h has the rule).  No GPU involved.
PT_API int PTRepackPlanHost(const uint32_t* flags, uint32_t numSlots, uint32_t capacity, uint32_t fillNum, uint32_t fillDen, uint32_t* outPlan, uint32_t* outDest)
{
    ptrepack::Plan plan;
    if (!flags || !outPlan || !ptrepack::plan_host(flags, numSlots, capacity, fillNum, fillDen, plan, outDest, nullptr)) {
        g_buildError = "NULL flags or plan, numSlots not a multiple of 256, or fillDen == 0";
        return 0;
    }
    outPlan[0] = plan.go; outPlan[1] = plan.live; outPlan[2] = plan.extent;
    g_buildError.clear();
    return 1;
}
// Shading from the bakes on the host (shade_host.cpp; Part 21 has the rule).  No GPU involved.
PT_API int PTBakeDFGHost(uint32_t res, PTShadeDFG* out)
{
    if (!ptshade::bake_dfg_host(res, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTShadeTermsHost(const PTShadeMaterial* materials, const PTRay* rays, const PTRaySurface* surface, uint64_t count, const PTProbe* probes,
                            const PTReflectionBox* boxes, uint32_t probeCount, PTShadeTerms* outTerms, PTReceiver* outReceivers,
                            PTReflectionQuery* outQueries)
{
    if (!ptshade::terms_host(materials, rays, surface, count, probes, boxes, probeCount, outTerms, outReceivers, outQueries, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTShadeComposeHost(const PTShadeTerms* terms, const PTIrradiance* irradiance, const PTReflectionTexel* reflection, uint64_t count,
                              const PTShadeDFG* dfg, uint32_t dfgRes, float* out)
{
    if (!ptshade::compose_host(terms, irradiance, reflection, count, dfg, dfgRes, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// The lightmap lookup on the host (lightmap_lookup_host.cpp; Part 22 has the rule).  No GPU involved.
PT_API int PTLightmapLookupHost(const PTLightmapBinding* bindings, uint32_t bindingCount, const PTTriangleAttributes* attrs, uint64_t attrCount,
                                uint32_t materialCount, const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces, uint64_t count,
                                PTIrradiance* out, uint32_t* outBinding)
{
    if (!ptlm::lookup_host(bindings, bindingCount, attrs, attrCount, materialCount, rays, hits, surfaces, count, out, outBinding, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// Lightmap UVs on the host (unwrap_host.cpp; Part 23 has the rule).  No GPU involved.
namespace {
bool unwrap_desc_ok(const PTUnwrapDesc* desc, const char* who)
{
    if (!desc) { g_buildError = std::string(who) + ": desc == NULL"; return false; }
    if (desc->structSize < sizeof(PTUnwrapDesc) || desc->structSize > 4096u) {
        g_buildError = "PTUnwrapDesc.structSize is not set (must be sizeof(PTUnwrapDesc) of the host's header)";
        return false;
    }
    for (uint32_t r : desc->reserved) if (r) { g_buildError = "PTUnwrapDesc.reserved != 0"; return false; }
    return ptunwrap::unwrap_check_count(desc->triangleCount, who, g_buildError);
}
} // namespace
PT_API int PTUnwrapChartsHost(const PTUnwrapDesc* desc, const PTFloat4* tris, const PTFloat4* verticesOrNull, uint32_t* chartOfPrim, PTUnwrapChart* charts,
                              uint32_t capacity, uint32_t* chartCount, PTUnwrapStats* statsOrNull)
{
    if (!chartCount) { g_buildError = "PTUnwrapChartsHost: chartCount == NULL"; return 0; }
    *chartCount = 0;
    if (!unwrap_desc_ok(desc, "PTUnwrapChartsHost")) return 0;
    if (!ptunwrap::unwrap_charts_host(tris, verticesOrNull, (uint32_t)desc->triangleCount, chartOfPrim, charts, capacity, *chartCount, statsOrNull, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTPackChartsHost(const PTUnwrapChart* charts, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float texelsPerUnit,
                            int32_t* origins, uint32_t* rowsUsed)
{
    if (!rowsUsed) { g_buildError = "PTPackChartsHost: rowsUsed == NULL"; return 0; }
    if (!ptunwrap::pack_charts_host(charts, chartCount, width, height, padding, texelsPerUnit, origins, *rowsUsed, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTEmitChartUVsHost(const PTUnwrapDesc* desc, const PTFloat4* tris, const PTFloat4* verticesOrNull, const uint32_t* chartOfPrim,
                              const PTUnwrapChart* charts, const int32_t* origins, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding,
                              float texelsPerUnit, float* uvs)
{
    if (!unwrap_desc_ok(desc, "PTEmitChartUVsHost")) return 0;
    if (!ptunwrap::emit_uvs_host(tris, verticesOrNull, (uint32_t)desc->triangleCount, chartOfPrim, charts, origins, chartCount, width, height, padding,
                                 texelsPerUnit, uvs, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// Direct light at first hits on the host (direct_host.cpp; Part 24 has the rule).  No GPU involved.
PT_API int PTDirectPairCountHost(const void* lights, uint32_t lightCount, uint32_t strata, uint32_t* outPairsPerEntry)
{
    if (!ptdirect::pair_count_host(lights, lightCount, strata, outPairsPerEntry, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTDirectRaysHost(const PTDirectParams* params, const void* lights, uint32_t lightCount, const PTRay* rays, const PTShadeTerms* terms,
                            const PTReceiver* receivers, uint64_t count, PTRay* outRays, float* outContrib)
{
    if (!ptdirect::rays_host(params, lights, lightCount, rays, terms, receivers, count, outRays, outContrib, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API int PTDirectAccumulateHost(const PTShadeTerms* terms, const float* contrib, const PTRayHit* pairHits, uint64_t count, uint32_t pairsPerEntry,
                                  float* out)
{
    if (!ptdirect::accumulate_host(terms, contrib, pairHits, count, pairsPerEntry, out, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
// The light grid of the culled direct-light calls on the host (light_grid_host.cpp; Part 25 has the rule).  No GPU involved.
PT_API int PTBuildLightGridHost(const PTLightGridParams* params, const void* lights, uint32_t lightCount, uint32_t* offsets, uint32_t* indices,
                                uint64_t indexCapacity, uint32_t* rectBefore, uint64_t* outTotal)
{
    if (!ptlgrid::build_host(params, lights, lightCount, offsets, indices, indexCapacity, rectBefore, outTotal, g_buildError)) return 0;
    g_buildError.clear();
    return 1;
}
PT_API void DestroyBVH(int index) { free_slot(g_bvhs, index); }
PT_API int IsBVHReady(int index) { return get_slot(g_bvhs, index) != nullptr; }
PT_API void* GetBVH(int index) { return get_slot(g_bvhs, index); }
PT_API void* GetBVHPtr(int index) { return get_slot(g_bvhs, index); }
PT_API int GetCWBVHNodesSize(int index)
{
    ptbvh::Cwbvh* b = get_slot(g_bvhs, index);
    return b ? (int)(b->usedBlocks * 16u) : 0;
}
PT_API int GetCWBVHTrisSize(int index)
{
    ptbvh::Cwbvh* b = get_slot(g_bvhs, index);
    return b ? (int)(b->triCount * 3u * 16u) : 0;
}
PT_API int GetCWBVHData(int index, PTFloat4** bvhNodes, PTFloat4** bvhTris)
{
    ptbvh::Cwbvh* b = get_slot(g_bvhs, index);
    if (!b || !bvhNodes || !bvhTris || b->nodeData.empty() || b->triData.empty()) return 0;
    *bvhNodes = b->nodeData.data();
    *bvhTris = b->triData.data();
    return 1;
}

PT_API int BuildTLAS(const PTBlasInstance* instances, int instanceCount)
{
    if (!instances || instanceCount <= 0) return -1;
    ptbvh::Tlas* t = new ptbvh::Tlas();
    if (!t->build(instances, (uint32_t)instanceCount)) { delete t; return -1; }
    return add_slot(g_tlases, t);
}
PT_API void DestroyTLAS(int index) { free_slot(g_tlases, index); }
PT_API int IsTLASReady(int index) { return get_slot(g_tlases, index) != nullptr; }
PT_API int GetTLASNodesSize(int index)
{
    ptbvh::Tlas* t = get_slot(g_tlases, index);
    return t ? (int)(t->usedNodes * 64u) : 0;
}
PT_API int GetTLASData(int index, PTFloat4** tlasNodes, uint32_t** tlasIndices)
{
    ptbvh::Tlas* t = get_slot(g_tlases, index);
    if (!t || !tlasNodes || !tlasIndices || t->nodes.empty()) return 0;
    *tlasNodes = (PTFloat4*)t->nodes.data();
    *tlasIndices = t->indices.data();
    return 1;
}

} // extern "C"
