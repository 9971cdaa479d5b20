// pt_api_lmfilter.hip — the lightmap denoiser: a gathered list filtered in texel space, list in, list out (include/ptmi_plugin.h
// Part 17).  The host twin is in plugin_exports.cpp over lmfilter_host.cpp, which also holds the checks shared here.
#include "pt_context.h"
#include "lmfilter_rule.h"

extern "C" {

PT_API int PTDenoiseLightmap(PTContext* c, const PTLightmapDenoiseParams* hostParams, const uint32_t* dTexels, const PTReceiver* dRecv, const PTIrradiance* dIrr,
                             uint64_t count, uint32_t width, uint32_t height, PTIrradiance* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTDenoiseLightmap: ctx == NULL");
    std::string err;
    if (!ptlmf::check_params(hostParams, err) || !ptlmf::check_size(width, height, count, err)) return fail(PT_ERR_INVALID_ARG, "PTDenoiseLightmap: " + err);
    if (count && (!dTexels || !dRecv || !dIrr || !dOut)) return fail(PT_ERR_INVALID_ARG, "PTDenoiseLightmap: texels / receivers / irradiance / out == NULL");
    if (misaligned(dTexels, 4) || misaligned(dRecv, 16) || misaligned(dIrr, 16) || misaligned(dOut, 16))
        return fail(PT_ERR_INVALID_ARG, "PTDenoiseLightmap: texels (4 bytes), receivers, irradiance or out (16 bytes) misaligned");
    if (count == 0) return PT_OK;
    PTLightmapDenoiseParams p;
    if (int rc = import_struct(hostParams, p, sizeof(PTLightmapDenoiseParams), "PTLightmapDenoiseParams", "PTDenoiseLightmap: params == NULL")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    PTContext::LightmapFilter& F = c->lmfilter;
    const size_t bytes = (size_t)width * height * 16u;
    // grown only for a larger atlas; the kernels that used the old images ran on the context stream
    int rc;
    if ((rc = F.state[0].reserve(bytes, c->stream)) || (rc = F.state[1].reserve(bytes, c->stream)) || (rc = F.guideP.reserve(bytes, c->stream)) ||
        (rc = F.guideN.reserve(bytes, c->stream)))
        return rc;
    const PTLmfImages im = {{(float4*)F.state[0].ptr, (float4*)F.state[1].ptr}, (float4*)F.guideP.ptr, (float4*)F.guideN.ptr};
    RoctxRange range("PT lightmap denoise");
    HIP_TRY(pt_launch_lmfilter(p, im, dTexels, dRecv, dIrr, count, width, height, dOut, c->stream));
    return PT_OK;
}

} // extern "C"
