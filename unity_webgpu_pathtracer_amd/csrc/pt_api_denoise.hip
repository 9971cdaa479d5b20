// pt_api_denoise.hip — first-hit guide buffers and the a-trous filter (include/ptmi_plugin.h Part 4).
#include "pt_context.h"

namespace {
// Everything runs on c->stream; buffers are regrown only after that stream has drained, so no launch still reads a buffer
// that is freed.
int ensure_guides(PTContext* c, uint32_t w, uint32_t h)
{
    PTContext::Guide& g = c->guide;
    if (!g.slab.ptr) {
        HIP_TRY(pt_guide_grid_caps(c->device, g.caps));
        const uint32_t cap = g.caps[0] > g.caps[1] ? g.caps[0] : g.caps[1];
        if (int rc = g.slab.reserve((size_t)cap * pt_resident_wave_slab_bytes())) return rc;
    }
    return g.frames.resize(w, h, {sizeof(float4), sizeof(float4)}, c->stream);
}

int import_denoise_params(const PTDenoiseParams* in, PTDenoiseParams& p)
{
    if (int rc = import_struct(in, p, sizeof(PTDenoiseParams), "PTDenoiseParams", "PTDenoise: params == NULL")) return rc;
    if (p.iterations < 0 || p.iterations > 8) return fail(PT_ERR_INVALID_ARG, "PTDenoise: iterations " + std::to_string(p.iterations) + " outside 0..8");
    // !(x > 0): NaN and <= 0
    if (!(p.sigmaLuminance > 0.0f) || !(p.sigmaNormal > 0.0f) || !(p.sigmaDepth > 0.0f))
        return fail(PT_ERR_INVALID_ARG, "PTDenoise: sigmaLuminance / sigmaNormal / sigmaDepth must be > 0 (and not NaN)");
    if (p.flags & ~PT_DENOISE_DEMODULATE_ALBEDO) return fail(PT_ERR_INVALID_ARG, "PTDenoise: unknown flag bits " + std::to_string(p.flags));
    return PT_OK;
}
} // namespace

extern "C" {

PT_API int PTRenderGuides(PTContext* c, const PTFrameParams* hostParams, int samplesPerPixel)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTRenderGuides: ctx == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    if (samplesPerPixel != 1 && samplesPerPixel != 4 && samplesPerPixel != 16)
        return fail(PT_ERR_INVALID_ARG, "PTRenderGuides: samplesPerPixel " + std::to_string(samplesPerPixel) + " is not 1, 4 or 16");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("PT guides (enqueue)");
    if ((rc = ensure_guides(c, p.OutputWidth, p.OutputHeight))) return rc;
    const uint32_t n = samplesPerPixel == 1 ? 1u : samplesPerPixel == 4 ? 2u : 4u;
    const PTContext::Guide& g = c->guide;
    HIP_TRY(pt_launch_guides(c->scene, p, n, g.frames.f4(0), g.frames.f4(1), (uint2*)g.slab.ptr, g.caps[c->scene.hasTlas ? 1 : 0], c->stream));
    return PT_OK;
}

PT_API int PTDenoise(PTContext* c, const PTDenoiseParams* params, const void* dSrc, void* dDst)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTDenoise: ctx == NULL");
    return denoise_frame(c, params, dSrc, dDst, nullptr);
}

} // extern "C"

int denoise_frame(PTContext* c, const PTDenoiseParams* params, const void* dSrc, void* dDst, const PTDenoiseVariance* variance)
{
    PTDenoiseParams p;
    int rc = import_denoise_params(params, p);
    if (rc) return rc;
    if (!dDst) return fail(PT_ERR_INVALID_ARG, "PTDenoise: dst == NULL");
    const FrameSet<2>& guides = c->guide.frames;
    if (!guides.w) return fail(PT_ERR_INVALID_ARG, "PTDenoise: no guides (call PTRenderGuides first)");
    if (!dSrc) {
        if (!c->frames.w) return fail(PT_ERR_INVALID_ARG, "PTDenoise: no frame rendered yet");
        if (c->frames.w != guides.w || c->frames.h != guides.h)
            return fail(PT_ERR_INVALID_ARG, "PTDenoise: the guides are " + std::to_string(guides.w) + "x" + std::to_string(guides.h) +
                                                ", the Output frame " + std::to_string(c->frames.w) + "x" + std::to_string(c->frames.h));
        dSrc = c->frames.f4(c->cur);
    }
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("PT denoise (enqueue)");
    const size_t bytes = (size_t)guides.w * guides.h * sizeof(float4);
    if (p.iterations == 0) {
        if (dSrc != dDst) HIP_TRY(hipMemcpyAsync(dDst, dSrc, bytes, hipMemcpyDeviceToDevice, c->stream));
        return PT_OK;
    }
    FrameSet<3>& state = c->denoise.state;
    if ((rc = state.resize(guides.w, guides.h, {sizeof(float4), sizeof(float4), sizeof(float2)}, c->stream))) return rc;
    PTDenoiseArgs A = {guides.w, guides.h, p.sigmaLuminance, p.sigmaNormal, p.sigmaDepth, p.flags};
    HIP_TRY(pt_launch_denoise(A, p.iterations, (const float4*)dSrc, (float4*)dDst, guides.f4(0), guides.f4(1), state.f4(0), state.f4(1),
                              (float2*)state.buf[2].ptr, variance, c->stream));
    return PT_OK;
}

extern "C" {

PT_API int PTDenoiseToHost(PTContext* c, const PTDenoiseParams* params, float* dst, uint64_t dstFloats)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTDenoiseToHost: ctx == NULL");
    if (!params || !dst) return fail(PT_ERR_INVALID_ARG, "PTDenoiseToHost: params/dst == NULL");
    if (!c->guide.frames.w) return fail(PT_ERR_INVALID_ARG, "PTDenoise: no guides (call PTRenderGuides first)");
    const uint64_t need = (uint64_t)c->guide.frames.w * c->guide.frames.h * 4;
    if (dstFloats < need) return fail(PT_ERR_INVALID_ARG, "destination too small");
    HIP_TRY(hipSetDevice(c->device));
    int rc = c->denoise.host.reserve(need * sizeof(float), c->stream);
    if (rc) return rc;
    if ((rc = PTDenoise(c, params, nullptr, c->denoise.host.ptr))) return rc;
    HIP_TRY(hipMemcpyAsync(dst, c->denoise.host.ptr, need * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

PT_API void* PTGetGuidePointer(PTContext* c, int which)
{
    if (!c || which < 0 || which > 1) return nullptr;
    return c->guide.frames.f4(which);
}

} // extern "C"
