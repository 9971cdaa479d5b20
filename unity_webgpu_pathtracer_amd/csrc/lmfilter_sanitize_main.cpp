// lmfilter_sanitize_main.cpp — the host twin of the lightmap denoiser (lmfilter_host.cpp) in a stand-alone program for
// `make lmfilter-sanitize` (AddressSanitizer + UBSan, host code only, no GPU): filters generated lists in exactly sized heap
// arrays (a one-texel atlas; a sparse two-plane atlas with bad entries and isolated texels at sizes the steps outgrow, in place
// and out of place, at every number of levels), and makes the refusals.  Prints "lmfilter ok" and returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "lmfilter_rule.h"

namespace {

uint32_t g_state = 1717u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("lmfilter-sanitize: %s\n", what); return 1; }

PTLightmapDenoiseParams params(uint32_t samples, uint32_t iterations)
{
    PTLightmapDenoiseParams p = {};
    p.structSize = sizeof(p);
    p.samples = samples; p.iterations = iterations; p.normalPower = 5;
    p.sigmaLuminance = 4.0f; p.sigmaPosition = 4.0f; p.sigmaPlane = 1.0f;
    return p;
}

} // namespace

int main()
{
    using namespace ptlmf;
    std::string err;
    // ---- one texel: isolated, so its rgb stays and m2 becomes the variance of the mean
    {
        const uint32_t texel = 0;
        const PTReceiver r = {{1, 2, 3}, 0, {0, 1, 0}, 0};
        const PTIrradiance in = {{1.0f, 1.0f, 1.0f}, 40.0f};
        PTIrradiance out = {};
        const PTLightmapDenoiseParams p = params(16, 8);
        if (!denoise_host(&p, &texel, &r, &in, 1, 1, 1, &out, err)) return bad(err.c_str());
        if (std::memcmp(out.rgb, in.rgb, 12) != 0) return bad("the lone texel's rgb moved");
        if (!(std::fabs(out.m2 - (40.0f - 16.0f) / 15.0f / 16.0f) < 1e-6f)) return bad("the lone texel's variance is wrong");
    }
    // ---- a floor and a wall, sparse, with a bad entry of each kind
    static const uint32_t kSizes[3][2] = {{7, 5}, {17, 16}, {130, 67}};
    for (const auto& size : kSizes) {
        const uint32_t W = size[0], H = size[1];
        std::vector<uint32_t> texels;
        std::vector<PTReceiver> recv;
        std::vector<PTIrradiance> irr;
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                if (rnd() < 0.2f) continue;
                const bool wall = y >= H / 2;
                const float u = 0.1f * (float)x, t = 0.1f * (float)y;
                PTReceiver r = {{u, wall ? t : 0.0f, wall ? 0.0f : t}, 0, {0, wall ? 0.0f : 1.0f, wall ? 1.0f : 0.0f}, 0};
                const float e = 0.5f + rnd();
                PTIrradiance i = {{e, 0.5f * e, 0.25f * e}, 16.0f * e * e * (1.0f + 0.3f * rnd())};
                const uint32_t k = (uint32_t)texels.size();
                const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
                if (k % 41 == 7) i.rgb[1] = nan;
                if (k % 41 == 13) i.m2 = inf;
                if (k % 41 == 19) r.position[2] = -inf;
                if (k % 41 == 23) r.normal[0] = nan;
                texels.push_back(y * W + x);
                recv.push_back(r);
                irr.push_back(i);
            }
        const uint64_t n = texels.size();
        for (uint32_t it = 0; it <= 8; ++it) {
            const PTLightmapDenoiseParams p = params(16, it);
            std::vector<PTIrradiance> out(n), inplace(irr);
            if (!denoise_host(&p, texels.data(), recv.data(), irr.data(), n, W, H, out.data(), err)) return bad(err.c_str());
            if (!denoise_host(&p, texels.data(), recv.data(), inplace.data(), n, W, H, inplace.data(), err)) return bad(err.c_str());
            if (std::memcmp(out.data(), inplace.data(), n * sizeof(PTIrradiance)) != 0) return bad("in place differs from out of place");
            for (uint64_t k = 0; k < n; ++k) {
                const bool isBad = k % 41 == 7 || k % 41 == 13 || k % 41 == 19 || k % 41 == 23;
                if (isBad && std::memcmp(&out[k], &irr[k], 16) != 0) return bad("a bad entry's bytes moved");
                if (!isBad && !(std::isfinite(out[k].rgb[0]) && std::isfinite(out[k].rgb[1]) && std::isfinite(out[k].rgb[2]) && out[k].m2 >= 0.0f))
                    return bad("a good entry is not finite");
            }
        }
        // the refusals
        PTLightmapDenoiseParams p = params(16, 5);
        std::vector<PTIrradiance> out(n);
        if (!denoise_host(&p, nullptr, nullptr, nullptr, 0, W, H, nullptr, err)) return bad("an empty list was refused");
        std::vector<uint32_t> t2(texels);
        t2[n - 1] = W * H;
        if (denoise_host(&p, t2.data(), recv.data(), irr.data(), n, W, H, out.data(), err)) return bad("an index past the image was not refused");
        t2[n - 1] = t2[0];
        if (denoise_host(&p, t2.data(), recv.data(), irr.data(), n, W, H, out.data(), err)) return bad("a duplicate was not refused");
        if (denoise_host(&p, texels.data(), recv.data(), irr.data(), n, 0, H, out.data(), err)) return bad("width 0 was not refused");
        if (denoise_host(&p, texels.data(), recv.data(), irr.data(), (uint64_t)W * H + 1, W, H, out.data(), err)) return bad("count > width * height was not refused");
        p.samples = 1;
        if (denoise_host(&p, texels.data(), recv.data(), irr.data(), n, W, H, out.data(), err)) return bad("samples 1 was not refused");
        p = params(16, 9);
        if (denoise_host(&p, texels.data(), recv.data(), irr.data(), n, W, H, out.data(), err)) return bad("iterations 9 was not refused");
        p = params(16, 5); p.sigmaPlane = 0.0f;
        if (denoise_host(&p, texels.data(), recv.data(), irr.data(), n, W, H, out.data(), err)) return bad("sigmaPlane 0 was not refused");
        p = params(16, 5); p.reserved[4] = 1;
        if (denoise_host(&p, texels.data(), recv.data(), irr.data(), n, W, H, out.data(), err)) return bad("a reserved word was not refused");
    }
    std::printf("lmfilter ok\n");
    return 0;
}
