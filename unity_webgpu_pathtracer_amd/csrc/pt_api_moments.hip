// pt_api_moments.hip — per-pixel variance across passes: moments, the noise metric and the denoiser led by them
// (include/ptmi_plugin.h Part 6).
#include "pt_context.h"

#include <cmath>

namespace {

std::string dims(uint32_t w, uint32_t h) { return std::to_string(w) + "x" + std::to_string(h); }

// Everything runs on c->stream.  A pass's resolve is ordered on that stream on both sides (render_to records its call event there
// and makes the stream wait for the set's `done`), so a kernel enqueued here runs after the resolve of the passes enqueued so
// far and before the resolve of any later pass; the trace chains run on their sets' streams and never wait for it.
int accumulate(PTContext* c, const PTFrameParams& p, int count, const void* dOut, const void* dAcc, int ownIndex, const char* who)
{
    PTContext::Moments& M = c->moments;
    if (c->adaptive.live)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": adaptive state is live, its blocks hold different sample counts (use PTAccumulateMomentsActive, or PTAdaptiveEnd first)");
    if (count < 1 || count > PT_MAX_BATCH)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": count " + std::to_string(count) + " outside 1.." + std::to_string(PT_MAX_BATCH));
    if (!dOut) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": output frame == NULL");
    const uint64_t n = p.CurrentSample;
    const uint64_t m = (uint64_t)count * (uint64_t)(p.SamplesPerPass > 1 ? p.SamplesPerPass : 1);
    const uint32_t W = p.OutputWidth, H = p.OutputHeight;
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0u) {
        if (int rc = M.planes.resize(W, H, {sizeof(float4), sizeof(float4)}, c->stream)) return rc;
        for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(M.planes.f4(k), 0, M.planes.buf[k].used, c->stream));
        M.observations = 1u;
        M.samples = m;
    } else {
        if (!M.planes.w) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": CurrentSample " + std::to_string(n) + " but nothing accumulated yet (start at CurrentSample 0)");
        if (M.planes.w != W || M.planes.h != H)
            return fail(PT_ERR_INVALID_ARG, std::string(who) + ": the moments are " + dims(M.planes.w, M.planes.h) + ", the frame is " + dims(W, H));
        if (n != M.samples)
            return fail(PT_ERR_INVALID_ARG, std::string(who) + ": CurrentSample " + std::to_string(n) + " does not continue the " +
                                                std::to_string(M.samples) + " samples accumulated so far");
        if (!dAcc) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": CurrentSample > 0 needs an accumulated frame");
        const float f = (float)((double)n * (double)(n + m) / (double)m);
        HIP_TRY(pt_launch_moments_accumulate(W * H, f, (const float4*)dOut, (const float4*)dAcc, M.planes.f4(0), M.planes.f4(1), c->stream));
        M.observations += 1u;
        M.samples = n + m;
    }
    M.lastOwn = ownIndex;
    M.lastPtr = ownIndex < 0 ? dOut : nullptr;
    return PT_OK;
}

// the frame last accumulated, or nullptr with the error set
const void* last_frame(PTContext* c, const char* who)
{
    const PTContext::Moments& M = c->moments;
    if (M.lastOwn < 0) return M.lastPtr;
    if (c->frames.w != M.planes.w || c->frames.h != M.planes.h) {
        fail(PT_ERR_INVALID_ARG, std::string(who) + ": the frame last accumulated no longer exists (the context's frames are now " +
                                     dims(c->frames.w, c->frames.h) + ")");
        return nullptr;
    }
    return c->frames.f4(M.lastOwn);
}

int need_observations(const PTContext* c, const char* who)
{
    if (c->moments.observations < 2u)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": needs at least 2 observations, has " + std::to_string(c->moments.observations));
    return PT_OK;
}

float inv_dof(const PTContext* c) { return (float)(1.0 / ((double)(c->moments.observations - 1u) * (double)c->moments.samples)); }

} // namespace

extern "C" {

PT_API int PTAccumulateMoments(PTContext* c, const PTFrameParams* hostParams, int count)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTAccumulateMoments: ctx == NULL");
    PTFrameParams p;
    if (int rc = import_frame_params(hostParams, p)) return rc;
    if (c->frames.w != p.OutputWidth || c->frames.h != p.OutputHeight)
        return fail(PT_ERR_INVALID_ARG, "PTAccumulateMoments: the context's frames are " + dims(c->frames.w, c->frames.h) + ", the params say " +
                                            dims(p.OutputWidth, p.OutputHeight) + " (call it after the pass)");
    return accumulate(c, p, count, c->frames.f4(c->cur), c->frames.f4(1 - c->cur), c->cur, "PTAccumulateMoments");
}

PT_API int PTAccumulateMomentsTo(PTContext* c, const PTFrameParams* hostParams, int count, const void* dOutput, const void* dAccumulated)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTAccumulateMomentsTo: ctx == NULL");
    PTFrameParams p;
    if (int rc = import_frame_params(hostParams, p)) return rc;
    return accumulate(c, p, count, dOutput, dAccumulated, -1, "PTAccumulateMomentsTo");
}

PT_API int PTGetMomentsInfo(PTContext* c, uint32_t* observations, uint64_t* samples, uint32_t* width, uint32_t* height)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGetMomentsInfo: ctx == NULL");
    if (observations) *observations = c->moments.observations;
    if (samples) *samples = c->moments.samples;
    if (width) *width = c->moments.planes.w;
    if (height) *height = c->moments.planes.h;
    return PT_OK;
}

PT_API void* PTGetMomentsPointer(PTContext* c, int which)
{
    if (!c || which < 0 || which > 1) return nullptr;
    return c->moments.planes.f4(which);
}

PT_API int PTMeasureNoise(PTContext* c, const PTNoiseParams* params, const void* dFrame, PTNoiseStats* out)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTMeasureNoise: ctx == NULL");
    if (!params || !out) return fail(PT_ERR_INVALID_ARG, "PTMeasureNoise: params/out == NULL");
    if (params->structSize < sizeof(PTNoiseParams) || params->structSize > 4096u)
        return fail(PT_ERR_INVALID_ARG, "PTNoiseParams.structSize is not set (must be sizeof(PTNoiseParams) of the host's header)");
    if (out->structSize < sizeof(PTNoiseStats) || out->structSize > 65536u)
        return fail(PT_ERR_INVALID_ARG, "PTNoiseStats.structSize is not set (must be sizeof(PTNoiseStats) of the host's header)");
    // !(x > 0): NaN and <= 0
    if (!(params->relFloor > 0.0f) || !(params->threshold > 0.0f))
        return fail(PT_ERR_INVALID_ARG, "PTMeasureNoise: relFloor / threshold must be > 0 (and not NaN)");
    if (!(params->percentile > 0.0f) || !(params->percentile <= 1.0f))
        return fail(PT_ERR_INVALID_ARG, "PTMeasureNoise: percentile outside (0, 1]");
    if (int rc = need_observations(c, "PTMeasureNoise")) return rc;
    if (!dFrame && !(dFrame = last_frame(c, "PTMeasureNoise"))) return PT_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(c->device));
    PTContext::Moments& M = c->moments;
    const uint32_t W = M.planes.w, H = M.planes.h;
    const size_t blocks = (size_t)((W + 15u) / 16u) * ((H + 15u) / 16u);
    int rc;
    if ((rc = M.stats.reserve(PT_NOISE_WORDS * sizeof(uint32_t), c->stream)) || (rc = M.blockSums.reserve(blocks * sizeof(float), c->stream)) ||
        (rc = M.tiles.reserve(blocks * sizeof(float), c->stream)))
        return rc;
    HIP_TRY(hipMemsetAsync(M.stats.ptr, 0, PT_NOISE_WORDS * sizeof(uint32_t), c->stream));
    // adaptive state of this size: one 1 / ((k_b - 1) W_b) per block, and the statistics name the least converged owned block
    const float* blockInvDof;
    uint32_t observations;
    uint64_t samples;
    if ((rc = adaptive_inv_dof(c, &blockInvDof, &observations, &samples))) return rc;
    const PTNoiseArgs A = {W, H, (uint32_t)c->rank, (uint32_t)(c->world > 1 ? c->world : 1), inv_dof(c), params->relFloor, params->threshold};
    HIP_TRY(pt_launch_noise(A, (const float4*)dFrame, M.planes.f4(0), (uint32_t*)M.stats.ptr, (float*)M.blockSums.ptr, (float*)M.tiles.ptr, c->stream, blockInvDof));
    uint32_t words[PT_NOISE_WORDS];
    HIP_TRY(hipMemcpyAsync(words, M.stats.ptr, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));

    PTNoiseStats s;
    memset(&s, 0, sizeof(s));
    s.structSize = (uint32_t)sizeof(s);
    s.observations = observations;
    s.samples = samples;
    for (int b = 0; b < 256; ++b) { s.histogram[b] = words[b]; s.pixels += words[b]; }
    s.pixelsBelow = words[PT_NOISE_BELOW];
    float sum;
    memcpy(&s.maxError, &words[PT_NOISE_MAX], sizeof(float));
    memcpy(&sum, &words[PT_NOISE_SUM], sizeof(float));
    if (s.pixels) {
        s.meanError = sum / (float)s.pixels;
        const uint64_t target = (uint64_t)std::ceil((double)params->percentile * (double)s.pixels);
        uint64_t cum = 0;
        int bin = 0;
        for (; bin < 255; ++bin) { cum += s.histogram[bin]; if (cum >= target) break; }
        // the upper edge of bin b is the value whose bits are (b + 1 + ((127 - 24) << 3)) << 20
        const uint32_t edge = (uint32_t)(bin + 1 + ((127 - 24) << 3)) << 20;
        if (bin == 255) s.percentileError = INFINITY;
        else memcpy(&s.percentileError, &edge, sizeof(float));
    }
    memcpy(out, &s, sizeof(s));
    return PT_OK;
}

PT_API void* PTGetNoiseTilePointer(PTContext* c)
{
    return c ? c->moments.tiles.ptr : nullptr;
}

PT_API int PTDenoiseMoments(PTContext* c, const PTDenoiseParams* params, const void* dSrc, void* dDst)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTDenoiseMoments: ctx == NULL");
    if (!params || !dDst) return fail(PT_ERR_INVALID_ARG, "PTDenoiseMoments: params/dst == NULL");
    if (int rc = need_observations(c, "PTDenoiseMoments")) return rc;
    const PTContext::Moments& M = c->moments;
    const FrameSet<2>& guides = c->guide.frames;
    if (!guides.w) return fail(PT_ERR_INVALID_ARG, "PTDenoiseMoments: no guides (call PTRenderGuides first)");
    if (guides.w != M.planes.w || guides.h != M.planes.h)
        return fail(PT_ERR_INVALID_ARG, "PTDenoiseMoments: the guides are " + dims(guides.w, guides.h) + ", the moments " + dims(M.planes.w, M.planes.h));
    if (!dSrc && !(dSrc = last_frame(c, "PTDenoiseMoments"))) return PT_ERR_INVALID_ARG;
    PTDenoiseVariance V = {M.planes.f4(0), M.planes.f4(1), inv_dof(c)};
    uint32_t observations;
    uint64_t samples;
    if (int rc = adaptive_inv_dof(c, &V.blockInvDof, &observations, &samples)) return rc;
    return denoise_frame(c, params, dSrc, dDst, &V);
}

PT_API int PTDenoiseMomentsToHost(PTContext* c, const PTDenoiseParams* params, float* dst, uint64_t dstFloats)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTDenoiseMomentsToHost: ctx == NULL");
    if (!params || !dst) return fail(PT_ERR_INVALID_ARG, "PTDenoiseMomentsToHost: params/dst == NULL");
    if (int rc = need_observations(c, "PTDenoiseMomentsToHost")) return rc;
    const uint64_t need = (uint64_t)c->moments.planes.w * c->moments.planes.h * 4;
    if (dstFloats < need) return fail(PT_ERR_INVALID_ARG, "destination too small");
    HIP_TRY(hipSetDevice(c->device));
    int rc = c->denoise.host.reserve(need * sizeof(float), c->stream);
    if (rc) return rc;
    if ((rc = PTDenoiseMoments(c, params, nullptr, c->denoise.host.ptr))) return rc;
    HIP_TRY(hipMemcpyAsync(dst, c->denoise.host.ptr, need * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

} // extern "C"
