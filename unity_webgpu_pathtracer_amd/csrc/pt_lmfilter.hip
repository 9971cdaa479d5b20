// pt_lmfilter.hip — the lightmap denoiser on the MI355X (include/ptmi_plugin.h Part 17): the rule of
// lmfilter_rule.h in kernels.  pt_lmf_scatter turns the list into a state image (e, v) and two guide images (P, h2) and
// (N, flags) -- the flags image is cleared first, so a texel no entry names reads as uncovered --, pt_lmf_footprint fills h2,
// one launch per level goes from one state image into the other (a 256-thread workgroup per 16x16 tile: pt_lmf_atrous_lds<S>
// stages the tile and its halo in LDS for the steps 1, 2 and 4, pt_lmf_atrous reads the taps of the larger steps through L2),
// pt_lmf_collect turns the last state back into the list.  No atomics: the same input gives the same bytes.
#include "pt_lmfilter.h"
#include "lmfilter_rule.h"

using namespace ptlmf;

namespace {

__global__ __launch_bounds__(256) void pt_lmf_scatter(const uint32_t* __restrict__ texels, const float4* __restrict__ recv, const float4* __restrict__ irr,
                                                      uint64_t count, uint32_t n, uint32_t samples, float4* __restrict__ state, float4* __restrict__ guideP,
                                                      float4* __restrict__ guideN)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t t = texels[i];
    if (t >= n) return;
    const float4 r0 = recv[i * 2u], r1 = recv[i * 2u + 1u], e = irr[i];
    const PTReceiver r = {{r0.x, r0.y, r0.z}, 0u, {r1.x, r1.y, r1.z}, 0u};
    const PTIrradiance in = {{e.x, e.y, e.z}, e.w};
    const float v = entry_variance(in.rgb, in.m2, samples);
    state[t] = make_float4(e.x, e.y, e.z, v);
    guideP[t] = make_float4(r0.x, r0.y, r0.z, 0.0f);
    guideN[t] = make_float4(r1.x, r1.y, r1.z, pt_asfloat(entry_bad(r, in, v) ? kBad : kGood));
}

__global__ __launch_bounds__(256) void pt_lmf_footprint(float4* __restrict__ guideP, const float4* __restrict__ guideN, uint32_t width, uint32_t height)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height || pt_asuint(guideN[i].w) != kGood) return;
    const int32_t x = (int32_t)(i % width), y = (int32_t)(i / width);
    const float4 p = guideP[i];
    const float Pp[3] = {p.x, p.y, p.z};
    float h2 = 0.0f;
    for (int k = 0; k < 4; ++k) {
        const int32_t xx = x + (k == 0 ? -1 : k == 1 ? 1 : 0), yy = y + (k == 2 ? -1 : k == 3 ? 1 : 0);
        if (xx < 0 || yy < 0 || xx >= (int32_t)width || yy >= (int32_t)height) continue;
        const size_t q = (size_t)yy * width + (size_t)xx;
        if (pt_asuint(guideN[q].w) != kGood) continue;
        const float4 pq = guideP[q];
        const float Pq[3] = {pq.x, pq.y, pq.z};
        h2 = footprint_step(h2, Pp, Pq);
    }
    // only the h2 word: the neighbours read this texel's position meanwhile
    reinterpret_cast<float*>(guideP + i)[3] = h2;
}

__device__ __forceinline__ void load_texel(const float4 st, const float4 gp, const float4 gn, Texel& t)
{
    t.e[0] = st.x; t.e[1] = st.y; t.e[2] = st.z; t.v = st.w;
    t.P[0] = gp.x; t.P[1] = gp.y; t.P[2] = gp.z; t.h2 = gp.w;
    t.N[0] = gn.x; t.N[1] = gn.y; t.N[2] = gn.z;
}

__global__ __launch_bounds__(256) void pt_lmf_atrous(const float4* __restrict__ src, float4* __restrict__ dst, const float4* __restrict__ guideP,
                                                     const float4* __restrict__ guideN, uint32_t width, uint32_t height, int32_t s, Sigmas sg)
{
    const int32_t x = (int32_t)(blockIdx.x * 16u + (threadIdx.x & 15u)), y = (int32_t)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (x >= (int32_t)width || y >= (int32_t)height) return;
    const size_t i = (size_t)y * width + (size_t)x;
    const float4 gn = guideN[i];
    if (pt_asuint(gn.w) != kGood) return;                           // uncovered or bad: never read as a tap, not collected from here
    const float4 st = src[i], gp = guideP[i];
    if (gp.w == 0.0f) { dst[i] = st; return; }                      // isolated: kept, and a tap of others at the next level
    Texel p;
    load_texel(st, gp, gn, p);
    auto fetch = [&](int32_t xx, int32_t yy, Texel& q) {
        const size_t t = (size_t)yy * width + (size_t)xx;
        const float4 qn = guideN[t];
        if (pt_asuint(qn.w) != kGood) return false;
        load_texel(src[t], guideP[t], qn, q);
        return true;
    };
    float o[4];
    filter_texel(sg, p, x, y, (int32_t)width, (int32_t)height, s, fetch, o);
    dst[i] = make_float4(o[0], o[1], o[2], o[3]);
}

// The same level with the tile and its halo of 2 * S texels staged in LDS: (16 + 4 S)^2 texels of 48 bytes (19, 27 and 48 KB for
// S = 1, 2, 4).  A texel outside the image or not good is staged as flags = 0.  Every thread reaches the barrier.
template <int S>
__global__ __launch_bounds__(256) void pt_lmf_atrous_lds(const float4* __restrict__ src, float4* __restrict__ dst, const float4* __restrict__ guideP,
                                                         const float4* __restrict__ guideN, uint32_t width, uint32_t height, Sigmas sg)
{
    constexpr int32_t T = 16 + 4 * S;
    __shared__ float4 lst[T * T], lp[T * T], ln[T * T];
    const int32_t ox0 = (int32_t)(blockIdx.x * 16u) - 2 * S, oy0 = (int32_t)(blockIdx.y * 16u) - 2 * S;
    for (int32_t k = (int32_t)threadIdx.x; k < T * T; k += 256) {
        const int32_t xx = ox0 + k % T, yy = oy0 + k / T;
        float4 qn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (xx >= 0 && yy >= 0 && xx < (int32_t)width && yy < (int32_t)height) {
            const size_t t = (size_t)yy * width + (size_t)xx;
            qn = guideN[t];
            if (pt_asuint(qn.w) == kGood) { lst[k] = src[t]; lp[k] = guideP[t]; }
        }
        ln[k] = qn;
    }
    __syncthreads();
    const int32_t x = (int32_t)(blockIdx.x * 16u + (threadIdx.x & 15u)), y = (int32_t)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (x >= (int32_t)width || y >= (int32_t)height) return;
    const int32_t self = (y - oy0) * T + (x - ox0);
    const float4 gn = ln[self];
    if (pt_asuint(gn.w) != kGood) return;
    const float4 st = lst[self], gp = lp[self];
    const size_t i = (size_t)y * width + (size_t)x;
    if (gp.w == 0.0f) { dst[i] = st; return; }
    Texel p;
    load_texel(st, gp, gn, p);
    auto fetch = [&](int32_t xx, int32_t yy, Texel& q) {
        const int32_t k = (yy - oy0) * T + (xx - ox0);          // within the tile and its halo: a tap is at most 2 * S away
        const float4 qn = ln[k];
        if (pt_asuint(qn.w) != kGood) return false;
        load_texel(lst[k], lp[k], qn, q);
        return true;
    };
    float o[4];
    filter_texel(sg, p, x, y, (int32_t)width, (int32_t)height, S, fetch, o);
    dst[i] = make_float4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void pt_lmf_collect(const uint32_t* __restrict__ texels, const float4* irr, uint64_t count, uint32_t n,
                                                      const float4* __restrict__ state, const float4* __restrict__ guideN, float4* out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t t = texels[i];
    // a bad entry (and an index the scatter skipped) gets its input bytes; out may be irr, entry by entry
    out[i] = (t < n && pt_asuint(guideN[t].w) == kGood) ? state[t] : irr[i];
}

} // namespace

hipError_t pt_launch_lmfilter(const PTLightmapDenoiseParams& p, const PTLmfImages& im, const uint32_t* texels, const PTReceiver* recv, const PTIrradiance* irr,
                              uint64_t count, uint32_t width, uint32_t height, PTIrradiance* out, hipStream_t stream)
{
    const size_t n = (size_t)width * height;
    const uint32_t texelBlocks = (uint32_t)((n + 255u) / 256u), entryBlocks = (uint32_t)((count + 255u) / 256u);
    hipError_t e;
    if ((e = hipMemsetAsync(im.guideN, 0, n * 16u, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt_lmf_scatter, dim3(entryBlocks), dim3(256), 0, stream, texels, (const float4*)recv, (const float4*)irr, count, (uint32_t)n, p.samples,
                       im.state[0], im.guideP, im.guideN);
    hipLaunchKernelGGL(pt_lmf_footprint, dim3(texelBlocks), dim3(256), 0, stream, im.guideP, im.guideN, width, height);
    const Sigmas sg = {p.sigmaLuminance, p.sigmaPosition * p.sigmaPosition, p.sigmaPlane, p.normalPower};
    uint32_t cur = 0;
    const dim3 tiles((width + 15u) / 16u, (height + 15u) / 16u);
    for (uint32_t k = 0; k < p.iterations; ++k) {
        const float4* src = im.state[cur];
        float4* dst = im.state[cur ^ 1u];
        // s = 1, 2, 4: the tile and its halo fit LDS (0.48 against 0.56 ms for five levels at 1024^2); from 8 on through L2
        if (k == 0) hipLaunchKernelGGL(pt_lmf_atrous_lds<1>, tiles, dim3(256), 0, stream, src, dst, im.guideP, im.guideN, width, height, sg);
        else if (k == 1) hipLaunchKernelGGL(pt_lmf_atrous_lds<2>, tiles, dim3(256), 0, stream, src, dst, im.guideP, im.guideN, width, height, sg);
        else if (k == 2) hipLaunchKernelGGL(pt_lmf_atrous_lds<4>, tiles, dim3(256), 0, stream, src, dst, im.guideP, im.guideN, width, height, sg);
        else hipLaunchKernelGGL(pt_lmf_atrous, tiles, dim3(256), 0, stream, src, dst, im.guideP, im.guideN, width, height, (int32_t)(1u << k), sg);
        cur ^= 1u;
    }
    hipLaunchKernelGGL(pt_lmf_collect, dim3(entryBlocks), dim3(256), 0, stream, texels, (const float4*)irr, count, (uint32_t)n, im.state[cur], im.guideN,
                       (float4*)out);
    return hipGetLastError();
}
