// pt_api_lightmap.hip — lightmap charts: a BLAS's UV chart into receivers, gathered irradiance back into an image (include/ptmi_plugin.h
// Part 14).  The host twins are in plugin_exports.cpp over chart_host.cpp.
#include "pt_context.h"
#include "chart_rule.h"

namespace {

int check_size(uint32_t width, uint32_t height, const char* who)
{
    if (width < 1u || width > ptchart::kMaxSize || height < 1u || height > ptchart::kMaxSize)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": width x height = " + std::to_string(width) + " x " + std::to_string(height) + " (each 1 ... 8192)");
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTRasterizeChart(PTContext* c, const PTChartDesc* hostDesc, const float* dUvsOrNull, uint32_t* dTexels, PTReceiver* dRecv, uint64_t capacity,
                            uint64_t* count)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: ctx == NULL");
    PTChartDesc d;
    if (int rc = import_struct(hostDesc, d, sizeof(PTChartDesc), "PTChartDesc", "PTRasterizeChart: desc == NULL")) return rc;
    if (!count) return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: count == NULL");
    *count = 0;
    if ((dTexels == nullptr) != (dRecv == nullptr)) return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: texels and receivers come together (both NULL: only the count)");
    if (misaligned(dTexels, 4) || misaligned(dRecv, 16) || misaligned(dUvsOrNull, 16))
        return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: texels (4 bytes), receivers or uvs (16 bytes) misaligned");
    if (d.reserved[0] || d.reserved[1] || d.reserved[2]) return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: PTChartDesc.reserved != 0");
    int rc;
    if ((rc = check_size(d.width, d.height, "PTRasterizeChart"))) return rc;
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (d.triangleCount <= 0 || d.bvhOffset < 0 || d.triOffset < 0 || d.triAttributeOffset < 0)
        return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: triangleCount <= 0 or a negative offset");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_host_copy(c))) return rc;
    PTContext::GeomPlan* plan = nullptr;
    if ((rc = find_plan(c, d.bvhOffset, d.triOffset, d.triAttributeOffset, (uint32_t)d.triangleCount, plan))) return rc;
    if (d.instance != -1) {
        // the offsets rows of the instance records are PTSetScene's: instance updates keep them
        const std::vector<int32_t>& keys = c->update.geometry.blasKeys;
        if (!c->scene.hasTlas || d.instance < 0 || (uint32_t)d.instance >= c->update.instanceCount)
            return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: instance " + std::to_string(d.instance) + " is not an instance of the scene (-1: identity)");
        const int32_t* k = &keys[(size_t)d.instance * 3u];
        if (k[0] != d.bvhOffset || k[1] != d.triOffset || k[2] != d.triAttributeOffset)
            return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: instance " + std::to_string(d.instance) + " belongs to another BLAS");
    }
    PTContext::Lightmap& L = c->lightmap;
    const size_t n = (size_t)d.width * d.height, blocks = pt_lm_blocks(d.width, d.height), T = plan->triCount;
    // grown only for a larger atlas or BLAS; the kernels that used the old arrays ran on the context stream
    if ((rc = L.owner.reserve(n * 4u, c->stream)) || (rc = L.blockBase.reserve((blocks + 2u) / 2u * 8u + 8u, c->stream)) ||
        (rc = L.prims.reserve((2u * T + 1u) * 4u, c->stream)) || (rc = L.count.reserve(8)))
        return rc;
    PTChartArgs A = {};
    A.tris = c->scene.tris + (size_t)d.triOffset;
    A.attrs = c->scene.attrs + (size_t)d.triAttributeOffset * 8u;
    A.uvs = dUvsOrNull;
    A.instance = d.instance >= 0 ? c->scene.instances + (size_t)d.instance * 9u : nullptr;
    A.triCount = (uint32_t)T; A.width = d.width; A.height = d.height; A.seedBase = d.seedBase;
    A.owner = (uint32_t*)L.owner.ptr;
    A.blockBase = (uint32_t*)L.blockBase.ptr;
    A.total = (uint64_t*)((char*)L.blockBase.ptr + (blocks + 2u) / 2u * 8u);
    A.recOfPrim = (uint32_t*)L.prims.ptr;
    A.large = A.recOfPrim + T;
    // on the context stream, which every scene update joins (end_update): the current generation of the records
    RoctxRange range("PT lightmap chart (rasterise)");
    HIP_TRY(pt_launch_lm_coverage(A, c->stream));
    HIP_TRY(hipMemcpyAsync(L.count.ptr, A.total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(count, L.count.ptr, 8);
    if (!dTexels) return PT_OK;
    if (*count > capacity)
        return fail(PT_ERR_INVALID_ARG, "PTRasterizeChart: the chart covers " + std::to_string(*count) + " texels, the arrays hold " + std::to_string(capacity));
    if (*count) HIP_TRY(pt_launch_lm_emit(A, dTexels, dRecv, c->stream));
    return PT_OK;
}

PT_API int PTResolveLightmap(PTContext* c, const uint32_t* dTexels, const PTIrradiance* dIrr, uint64_t count, uint32_t width, uint32_t height, uint32_t dilate,
                             void* dImage)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTResolveLightmap: ctx == NULL");
    if (!dImage || (count && (!dTexels || !dIrr))) return fail(PT_ERR_INVALID_ARG, "PTResolveLightmap: texels / irradiance / image == NULL");
    if (misaligned(dTexels, 4) || misaligned(dIrr, 16) || misaligned(dImage, 16))
        return fail(PT_ERR_INVALID_ARG, "PTResolveLightmap: texels (4 bytes), irradiance or image (16 bytes) misaligned");
    int rc;
    if ((rc = check_size(width, height, "PTResolveLightmap"))) return rc;
    if (dilate > ptchart::kMaxDilate) return fail(PT_ERR_INVALID_ARG, "PTResolveLightmap: dilate = " + std::to_string(dilate) + " (0 ... 16)");
    if (count > (uint64_t)width * height) return fail(PT_ERR_INVALID_ARG, "PTResolveLightmap: more entries than texels (indices are unique)");
    HIP_TRY(hipSetDevice(c->device));
    PTContext::Lightmap& L = c->lightmap;
    if (dilate && (rc = L.image.reserve((size_t)width * height * 16u, c->stream))) return rc;
    RoctxRange range("PT lightmap resolve");
    HIP_TRY(pt_launch_lm_resolve(dTexels, dIrr, count, width, height, dilate, (float4*)dImage, (float4*)L.image.ptr, c->stream));
    return PT_OK;
}

} // extern "C"
