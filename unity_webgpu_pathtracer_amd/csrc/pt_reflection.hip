// pt_reflection.hip — reflection probes (include/ptmi_plugin.h Part 20): the kernels around the radiance query's
// launch sequences and the two that need no scene.
//
//     pt_refl_rays        one lane per slot = (texel, sample): the jittered direction inside the texel and the RNG state the path
//                         starts with, as a PTRadianceRay
//     [ PTTraceRadiance's launch sequences over the slab: pt_wavefront.hip, unchanged ]
//     pt_refl_fold        one lane per texel: its samples' radiance in ascending order into one base texel
//     pt_refl_prefilter   a 256-thread workgroup owns up to 256 output texels of one level of one probe and walks the probe's
//                         whole base map through LDS, 256 source texels a tile
//     pt_refl_lookup      one lane per query: box projection, two levels, four taps each
//
// The arithmetic is reflection_rule.h's, which the host twins evaluate too.
#include "pt_device.h"
#include "pt_launch.h"
#include "reflection_rule.h"

namespace {

constexpr uint32_t kTile = 256u;            // source texels staged per step: 32 bytes each, 8 KiB

// slot -> texel of the list (probe * R * R + t) and sample; firstTexel: the list texel of the launch's slot 0
struct Slot { uint32_t probe, t, sample; };
PT_DEV Slot slot_of(uint64_t firstTexel, uint32_t slot, uint32_t samples, uint32_t log2Texels)
{
    const uint32_t tl = slot / samples;
    const uint64_t g = firstTexel + tl;
    return {(uint32_t)(g >> log2Texels), (uint32_t)g & ((1u << log2Texels) - 1u), slot - tl * samples};
}

__global__ __launch_bounds__(256) void pt_refl_rays(const PTProbe* __restrict__ probes, uint64_t firstTexel, uint32_t slots, uint32_t res, uint32_t log2Texels,
                                                    uint32_t firstSample, uint32_t samples, PTRadianceRay* __restrict__ rays)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= slots) return;
    const Slot s = slot_of(firstTexel, slot, samples, log2Texels);
    const float4 pr = ((const float4*)probes)[s.probe];
    uint32_t rng = ptrefl::sample_rng(pt_asuint(pr.w), s.t, firstSample, s.sample);
    float d[3];
    ptrefl::sample_direction(res, s.t & (res - 1u), s.t >> (log2Texels >> 1), rng, d);
    float4* e = (float4*)(rays + slot);
    e[0] = make_float4(pr.x, pr.y, pr.z, d[0]);
    e[1] = make_float4(d[1], d[2], pt_asfloat(rng), pt_asfloat(0u));
}

__global__ __launch_bounds__(256) void pt_refl_fold(const PTRadiance* __restrict__ radiance, uint32_t texels, uint32_t samples,
                                                    PTReflectionTexel* __restrict__ out)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= texels) return;
    const float4* c = (const float4*)radiance + (size_t)t * samples;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t j = 0; j < samples; ++j) {
        const float4 cj = c[j];
        const float L[3] = {cj.x, cj.y, cj.z};
        ptrefl::fold_step(acc, L);
    }
    const float n = (float)samples;
    ((float4*)out)[t] = make_float4(acc[0] / n, acc[1] / n, acc[2] / n, acc[3]);
}

// blockIdx.y: the probe; blockIdx.x: the block of the probe's map -- the blocks of level 0 (a copy), then of level 1, ...  Every
// thread of a workgroup makes one source texel's {l, J} per tile and loads its rgb; then every lane walks the tile in LDS, all
// lanes at the same address (a broadcast).  The loops and both barriers are uniform over the workgroup: a lane without an output
// texel (a level of fewer than 256) stages and waits like the others.
__global__ __launch_bounds__(256) void pt_refl_prefilter(const PTReflectionTexel* __restrict__ base, uint32_t res, uint32_t levels, uint32_t mapTexels,
                                                         PTReflectionTexel* __restrict__ out)
{
    __shared__ float4 tile[2u * kTile];         // [2 i] = {l, J}, [2 i + 1] = {rgb, -}
    const uint32_t baseTexels = res * res;
    uint32_t b = blockIdx.x, k = 0u, Rk = res, offset = 0u;
    for (;;) {
        const uint32_t blocks = (Rk * Rk + 255u) >> 8;
        if (b < blocks) break;                   // the grid has exactly the blocks of `levels` levels: k < levels here
        b -= blocks;
        offset += Rk * Rk;
        Rk >>= 1;
        ++k;
    }
    const float4* src = (const float4*)base + (size_t)blockIdx.y * baseTexels;
    float4* dst = (float4*)out + (size_t)blockIdx.y * mapTexels + offset;
    const uint32_t o = b * 256u + threadIdx.x;
    const bool owns = o < Rk * Rk;
    if (k == 0u) {                               // the whole workgroup
        if (owns) dst[o] = src[o];
        return;
    }
    const float g = ptrefl::lobe_g(k, levels);
    float n[3] = {0.0f, 0.0f, 1.0f}, len;
    if (owns) ptrefl::direction(Rk, o % Rk, o / Rk, 0.5f, 0.5f, n, len);
    float acc[3] = {0.0f, 0.0f, 0.0f}, sw = 0.0f;
    for (uint32_t first = 0u; first < baseTexels; first += kTile) {
        const uint32_t s = first + threadIdx.x;
        if (s < baseTexels) {
            float l[3], J;
            ptrefl::source(res, s, l, J);
            tile[2u * threadIdx.x] = make_float4(l[0], l[1], l[2], J);
            tile[2u * threadIdx.x + 1u] = src[s];
        }
        __syncthreads();
        const uint32_t cnt = baseTexels - first < kTile ? baseTexels - first : kTile;
        if (owns)
            for (uint32_t i = 0u; i < cnt; ++i) {
                const float4 lj = tile[2u * i], c = tile[2u * i + 1u];
                const float l[3] = {lj.x, lj.y, lj.z};
                float w;
                if (!ptrefl::weight(n, l, lj.w, g, w)) continue;
                acc[0] = acc[0] + w * c.x;
                acc[1] = acc[1] + w * c.y;
                acc[2] = acc[2] + w * c.z;
                sw = sw + w;
            }
        __syncthreads();
    }
    if (owns) dst[o] = make_float4(acc[0] / sw, acc[1] / sw, acc[2] / sw, sw);
}

__global__ __launch_bounds__(256) void pt_refl_lookup(const PTReflectionTexel* __restrict__ maps, uint64_t probeCount, uint32_t res, uint32_t levels,
                                                      uint32_t mapTexels, const PTProbe* __restrict__ probes, const PTReflectionBox* __restrict__ boxes,
                                                      const PTReflectionQuery* __restrict__ queries, uint32_t count, PTReflectionTexel* __restrict__ out)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= count) return;
    const float4 q0 = ((const float4*)queries)[2u * q], q1 = ((const float4*)queries)[2u * q + 1u];
    const uint32_t probe = pt_asuint(q1.w);
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (probe < probeCount) {
        const float P[3] = {q0.x, q0.y, q0.z}, dir[3] = {q1.x, q1.y, q1.z};
        const float4* map = (const float4*)maps + (size_t)probe * mapTexels;
        const auto load = [&](uint32_t t, float rgb[3]) {
            const float4 v = map[t];
            rgb[0] = v.x; rgb[1] = v.y; rgb[2] = v.z;
        };
        if (boxes) {
            const float4 pr = ((const float4*)probes)[probe];
            const float4 b0 = ((const float4*)boxes)[2u * (size_t)probe], b1 = ((const float4*)boxes)[2u * (size_t)probe + 1u];
            const float Q[3] = {pr.x, pr.y, pr.z}, bmin[3] = {b0.x, b0.y, b0.z}, bmax[3] = {b1.x, b1.y, b1.z};
            ptrefl::lookup(res, levels, P, q0.w, dir, Q, bmin, bmax, load, o);
        } else {
            ptrefl::lookup(res, levels, P, q0.w, dir, nullptr, nullptr, nullptr, load, o);
        }
    }
    ((float4*)out)[q] = make_float4(o[0], o[1], o[2], o[3]);
}

} // namespace

hipError_t pt_launch_refl_rays(const PTProbe* probes, uint64_t firstTexel, uint32_t texels, uint32_t res, uint32_t firstSample, uint32_t samples,
                               PTRadianceRay* rays, hipStream_t stream)
{
    const uint64_t slots = (uint64_t)texels * samples;
    if (samples == 0u || slots > (1ull << 30)) return hipErrorInvalidValue;
    if (slots == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_refl_rays, dim3((uint32_t)((slots + 255u) / 256u)), dim3(256), 0, stream, probes, firstTexel, (uint32_t)slots, res,
                       2u * ptrefl::log2_res(res), firstSample, samples, rays);
    return hipGetLastError();
}

hipError_t pt_launch_refl_fold(const PTRadiance* radiance, uint32_t texels, uint32_t samples, PTReflectionTexel* out, hipStream_t stream)
{
    if (samples == 0u) return hipErrorInvalidValue;
    if (texels == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_refl_fold, dim3((texels + 255u) / 256u), dim3(256), 0, stream, radiance, texels, samples, out);
    return hipGetLastError();
}

hipError_t pt_launch_refl_prefilter(const PTReflectionTexel* base, uint32_t probes, uint32_t res, uint32_t levels, PTReflectionTexel* out, hipStream_t stream)
{
    if (probes > 65535u) return hipErrorInvalidValue;            // blockIdx.y
    if (probes == 0u) return hipSuccess;
    uint32_t blocks = 0u;
    for (uint32_t k = 0; k < levels; ++k) blocks += ((res >> k) * (res >> k) + 255u) >> 8;
    hipLaunchKernelGGL(pt_refl_prefilter, dim3(blocks, probes), dim3(256), 0, stream, base, res, levels, ptrefl::level_offset(res, levels), out);
    return hipGetLastError();
}

hipError_t pt_launch_refl_lookup(const PTReflectionTexel* maps, uint64_t probeCount, uint32_t res, uint32_t levels, const PTProbe* probes,
                                 const PTReflectionBox* boxes, const PTReflectionQuery* queries, uint32_t count, PTReflectionTexel* out, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    if (boxes && !probes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_refl_lookup, dim3((count + 255u) / 256u), dim3(256), 0, stream, maps, probeCount, res, levels, ptrefl::level_offset(res, levels),
                       probes, boxes, queries, count, out);
    return hipGetLastError();
}
