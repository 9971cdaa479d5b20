// pt_api_unwrap.hip — lightmap UVs: one BLAS of the current scene into charts, and the packed charts into UVs (include/ptmi_plugin.h
// Part 23).  The host twins and the packer are in plugin_exports.cpp over unwrap_host.cpp.
#include "pt_context.h"
#include "unwrap_rule.h"

namespace {

// what both calls check of the desc and the scene; plan: the BLAS it names
int import_unwrap_desc(PTContext* c, const PTUnwrapDesc* hostDesc, const char* who, PTUnwrapDesc& d, PTContext::GeomPlan*& plan)
{
    if (int rc = import_struct(hostDesc, d, sizeof(PTUnwrapDesc), "PTUnwrapDesc", (std::string(who) + ": desc == NULL").c_str())) return rc;
    for (uint32_t r : d.reserved)
        if (r) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": PTUnwrapDesc.reserved != 0");
    std::string err;
    if (!ptunwrap::unwrap_check_count(d.triangleCount, who, err)) return fail(PT_ERR_INVALID_ARG, err);
    if (d.bvhOffset < 0 || d.triOffset < 0 || d.triAttributeOffset < 0) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": a negative offset");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_host_copy(c)) return rc;
    return find_plan(c, d.bvhOffset, d.triOffset, d.triAttributeOffset, (uint32_t)d.triangleCount, plan);
}

} // namespace

extern "C" {

PT_API int PTUnwrapCharts(PTContext* c, const PTUnwrapDesc* hostDesc, const PTFloat4* dVerticesOrNull, uint32_t* dChartOfPrim, PTUnwrapChart* dCharts,
                          uint32_t capacity, uint32_t* chartCount, PTUnwrapStats* statsOrNull)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTUnwrapCharts: ctx == NULL");
    if (!chartCount) return fail(PT_ERR_INVALID_ARG, "PTUnwrapCharts: chartCount == NULL");
    *chartCount = 0;
    if ((dChartOfPrim == nullptr) != (dCharts == nullptr))
        return fail(PT_ERR_INVALID_ARG, "PTUnwrapCharts: chartOfPrim and charts come together (both NULL: only the count)");
    if (misaligned(dVerticesOrNull, 16) || misaligned(dChartOfPrim, 4) || misaligned(dCharts, 16))
        return fail(PT_ERR_INVALID_ARG, "PTUnwrapCharts: vertices or charts (16 bytes) or chartOfPrim (4 bytes) misaligned");
    PTUnwrapDesc d;
    PTContext::GeomPlan* plan = nullptr;
    int rc;
    if ((rc = import_unwrap_desc(c, hostDesc, "PTUnwrapCharts", d, plan))) return rc;
    const uint32_t T = plan->triCount;
    const size_t workBytes = pt_unwrap_work_bytes(T);
    if (!workBytes) return fail(PT_ERR_HIP, "PTUnwrapCharts: rocprim::radix_sort_pairs: size query failed");
    PTContext::Unwrap& U = c->unwrap;
    // grown only for a larger BLAS; the kernels that used the old array ran on the context stream
    if ((rc = U.work.reserve(workBytes, c->stream)) || (rc = U.small.reserve(kUnwrapSmallWords * 4u))) return rc;
    PTUnwrapArgs A = {};
    A.tris = c->scene.tris + (size_t)d.triOffset;
    A.vertices = (const float4*)dVerticesOrNull;
    pt_unwrap_carve(U.work.ptr, T, A);
    uint32_t* small = (uint32_t*)U.small.ptr;
    // on the context stream, which every scene update joins (end_update): the current generation of the records
    RoctxRange range("PT unwrap charts");
    HIP_TRY(pt_launch_unwrap_edges(A, c->stream));
    uint32_t sweeps = 0;
    for (;;) {
        if (sweeps == PT_UNWRAP_MAX_SWEEPS) return fail(PT_ERR_HIP, "PTUnwrapCharts: the component search did not settle in 64 sweeps");
        HIP_TRY(pt_launch_unwrap_sweep(A, sweeps, c->stream));
        HIP_TRY(hipMemcpyAsync(small, A.small + 8u + sweeps, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ++sweeps;
        if (!small[0]) break;
    }
    HIP_TRY(pt_launch_unwrap_count(A, c->stream));
    HIP_TRY(hipMemcpyAsync(small, A.small, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *chartCount = small[4];
    if (statsOrNull) { statsOrNull->excluded = small[0]; statsOrNull->linkedEdges = small[1]; statsOrNull->singleCharts = small[2]; statsOrNull->sweeps = sweeps; }
    if (!dCharts) return PT_OK;
    if (*chartCount > capacity)
        return fail(PT_ERR_INVALID_ARG, "PTUnwrapCharts: the mesh has " + std::to_string(*chartCount) + " charts, the array holds " + std::to_string(capacity));
    HIP_TRY(pt_launch_unwrap_charts(A, dChartOfPrim, dCharts, *chartCount, c->stream));
    return PT_OK;
}

PT_API int PTEmitChartUVs(PTContext* c, const PTUnwrapDesc* hostDesc, const PTFloat4* dVerticesOrNull, const uint32_t* dChartOfPrim, const PTUnwrapChart* dCharts,
                          const int32_t* dOrigins, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float texelsPerUnit, float* dUvs)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTEmitChartUVs: ctx == NULL");
    if (!dChartOfPrim || !dUvs || (chartCount && (!dCharts || !dOrigins))) return fail(PT_ERR_INVALID_ARG, "PTEmitChartUVs: chartOfPrim / charts / origins / uvs == NULL");
    if (misaligned(dVerticesOrNull, 16) || misaligned(dChartOfPrim, 4) || misaligned(dCharts, 16) || misaligned(dOrigins, 8) || misaligned(dUvs, 8))
        return fail(PT_ERR_INVALID_ARG, "PTEmitChartUVs: vertices or charts (16 bytes), origins or uvs (8 bytes) or chartOfPrim (4 bytes) misaligned");
    std::string err;
    if (!ptunwrap::unwrap_check_atlas(width, height, padding, texelsPerUnit, "PTEmitChartUVs", err)) return fail(PT_ERR_INVALID_ARG, err);
    PTUnwrapDesc d;
    PTContext::GeomPlan* plan = nullptr;
    if (int rc = import_unwrap_desc(c, hostDesc, "PTEmitChartUVs", d, plan)) return rc;
    RoctxRange range("PT unwrap emit");
    HIP_TRY(pt_launch_unwrap_emit(c->scene.tris + (size_t)d.triOffset, (const float4*)dVerticesOrNull, plan->triCount, dChartOfPrim, dCharts, dOrigins, chartCount,
                                  width, height, padding, texelsPerUnit, dUvs, c->stream));
    return PT_OK;
}

} // extern "C"
