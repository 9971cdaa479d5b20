// lmfilter_host.cpp — the host twin of the lightmap denoiser (include/ptmi_plugin.h Part 17): the rule of
// lmfilter_rule.h in plain loops, texel by texel, and the argument checks the context's entry point shares with it.  No GPU involved.
#include "lmfilter_rule.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ptlmf {

bool check_params(const PTLightmapDenoiseParams* p, std::string& err)
{
    if (!p) { err = "params == NULL"; return false; }
    if (p->structSize < sizeof(PTLightmapDenoiseParams) || p->structSize > 4096u) {
        err = "PTLightmapDenoiseParams.structSize is not set (must be sizeof(PTLightmapDenoiseParams) of the host's header)";
        return false;
    }
    if (p->samples < kMinSamples || p->samples > kMaxSamples) { err = "samples = " + std::to_string(p->samples) + " (2 ... 16777216)"; return false; }
    if (p->iterations > kMaxIterations) { err = "iterations = " + std::to_string(p->iterations) + " (0 ... 8)"; return false; }
    if (p->normalPower > kMaxNormalPower) { err = "normalPower = " + std::to_string(p->normalPower) + " (0 ... 7)"; return false; }
    const float sigmas[3] = {p->sigmaLuminance, p->sigmaPosition, p->sigmaPlane};
    const char* names[3] = {"sigmaLuminance", "sigmaPosition", "sigmaPlane"};
    for (int k = 0; k < 3; ++k)
        if (!(std::isfinite(sigmas[k]) && sigmas[k] > 0.0f)) { err = std::string(names[k]) + " is not finite and positive"; return false; }
    for (uint32_t r : p->reserved)
        if (r) { err = "PTLightmapDenoiseParams.reserved != 0"; return false; }
    return true;
}

bool check_size(uint32_t width, uint32_t height, uint64_t count, std::string& err)
{
    if (width < 1u || width > kMaxSize || height < 1u || height > kMaxSize) {
        err = "width x height = " + std::to_string(width) + " x " + std::to_string(height) + " (each 1 ... 8192)";
        return false;
    }
    if (count > (uint64_t)width * height) { err = "more entries than texels (indices are unique)"; return false; }
    return true;
}

bool denoise_host(const PTLightmapDenoiseParams* params, const uint32_t* texels, const PTReceiver* recv, const PTIrradiance* irr, uint64_t count,
                  uint32_t width, uint32_t height, PTIrradiance* out, std::string& err)
{
    if (!check_params(params, err) || !check_size(width, height, count, err)) return false;
    if (count && (!texels || !recv || !irr || !out)) { err = "texels / receivers / irradiance / out == NULL"; return false; }
    const size_t n = (size_t)width * height;
    std::vector<uint8_t> flags(n, 0);
    for (uint64_t i = 0; i < count; ++i) {
        if (texels[i] >= n) { err = "texels[" + std::to_string(i) + "] = " + std::to_string(texels[i]) + " >= width * height"; return false; }
        if (flags[texels[i]]) { err = "texels[" + std::to_string(i) + "] = " + std::to_string(texels[i]) + " appears twice"; return false; }
        flags[texels[i]] = 1;
    }
    // step 1
    std::vector<Texel> a(n), b;
    for (uint64_t i = 0; i < count; ++i) {
        const float v = entry_variance(irr[i].rgb, irr[i].m2, params->samples);
        Texel& t = a[texels[i]];
        flags[texels[i]] = entry_bad(recv[i], irr[i], v) ? kBad : kGood;
        t = Texel{{irr[i].rgb[0], irr[i].rgb[1], irr[i].rgb[2]}, v, {recv[i].position[0], recv[i].position[1], recv[i].position[2]}, 0.0f,
                  {recv[i].normal[0], recv[i].normal[1], recv[i].normal[2]}};
    }
    // step 2
    static const int kDx[4] = {-1, 1, 0, 0}, kDy[4] = {0, 0, -1, 1};
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t t = (size_t)y * width + x;
            if (flags[t] != kGood) continue;
            float h2 = 0.0f;
            for (int k = 0; k < 4; ++k) {
                const int64_t xx = (int64_t)x + kDx[k], yy = (int64_t)y + kDy[k];
                if (xx < 0 || yy < 0 || xx >= (int64_t)width || yy >= (int64_t)height) continue;
                const size_t q = (size_t)yy * width + (size_t)xx;
                if (flags[q] == kGood) h2 = footprint_step(h2, a[t].P, a[q].P);
            }
            a[t].h2 = h2;
        }
    // step 4
    const Sigmas sg = {params->sigmaLuminance, params->sigmaPosition * params->sigmaPosition, params->sigmaPlane, params->normalPower};
    if (params->iterations) b = a;
    for (uint32_t k = 0; k < params->iterations; ++k) {
        const int32_t s = 1 << k;
        auto fetch = [&](int32_t xx, int32_t yy, Texel& q) {
            const size_t t = (size_t)yy * width + (size_t)xx;
            if (flags[t] != kGood) return false;
            q = a[t];
            return true;
        };
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                const size_t t = (size_t)y * width + x;
                if (flags[t] != kGood || a[t].h2 == 0.0f) continue;                 // b[t] is a[t] already
                float o[4];
                filter_texel(sg, a[t], (int32_t)x, (int32_t)y, (int32_t)width, (int32_t)height, s, fetch, o);
                b[t].e[0] = o[0]; b[t].e[1] = o[1]; b[t].e[2] = o[2]; b[t].v = o[3];
            }
        a.swap(b);
    }
    // step 5
    for (uint64_t i = 0; i < count; ++i) {
        const Texel& t = a[texels[i]];
        if (flags[texels[i]] == kBad) memmove(&out[i], &irr[i], sizeof(PTIrradiance));
        else out[i] = PTIrradiance{{t.e[0], t.e[1], t.e[2]}, t.v};
    }
    return true;
}

} // namespace ptlmf
