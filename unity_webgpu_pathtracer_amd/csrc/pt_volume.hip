// pt_volume.hip — probe volumes (include/ptmi_plugin.h Part 16): the kernels on either side of the closest-hit
// query of a depth bake, and the lookup.
//
//     pt_probe_depth_rays       one lane per (probe, sample): the PTRay {P, w_j, maxDistance, 0}
//     [ pt_launch_query ]       pt_query.hip's closest-hit kernel, unchanged
//     pt_probe_depth_resolve    one WAVE per probe, lane l = texel l: a tile of 64 samples is staged in LDS as {w, dist}, every lane
//                               walks it (a broadcast read) and keeps its three sums in registers; 512 contiguous bytes per wave
//     pt_probe_grid_irradiance  one lane per query: up to eight corners, each seven 16-byte loads of coefficients and one 8-byte
//                               load of moments
//
// The arithmetic is volume_rule.h's, which the host twins evaluate too; a direction is made from the seed wherever it is needed.
#include "pt_device.h"
#include "pt_launch.h"
#include "volume_rule.h"
#include "pt_volume_loads.h"

namespace {

constexpr uint32_t kWaves = 4u;             // probes per workgroup of the resolve

__global__ __launch_bounds__(256) void pt_probe_depth_rays(const PTProbe* __restrict__ probes, uint32_t entries, uint32_t samples, uint32_t firstSample,
                                                           float maxDistance, float4* __restrict__ rays)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const uint32_t entry = slot / samples, j = slot - entry * samples;
    if (entry >= entries) return;
    const float4 p = ((const float4*)probes)[entry];
    uint32_t rng = ptsh::sample_rng(pt_asuint(p.w), firstSample, j);
    float w[3];
    ptsh::direction(rng, w);
    rays[2u * (size_t)slot] = make_float4(p.x, p.y, p.z, w[0]);
    rays[2u * (size_t)slot + 1u] = make_float4(w[1], w[2], maxDistance, pt_asfloat(0u));
}

// Four probes per workgroup.  A wave whose probe is past the end still walks every tile and reaches every barrier: its loads and
// its store are guarded, not its loop (samples is uniform over the workgroup).
__global__ __launch_bounds__(256) void pt_probe_depth_resolve(const PTProbe* __restrict__ probes, uint32_t entries, uint32_t samples, uint32_t firstSample,
                                                              float maxDistance, const float4* __restrict__ hits, PTProbeDepthMap* __restrict__ out)
{
    __shared__ float4 stage[kWaves][ptvol::kTexels];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t entry = blockIdx.x * kWaves + wave;
    const bool live = entry < entries;
    uint32_t seed = 0u;
    if (live) seed = pt_asuint(((const float4*)probes)[entry].w);
    float d[3];
    ptvol::texel_direction(lane, d);
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (uint32_t base = 0; base < samples; base += ptvol::kTexels) {
        const uint32_t n = samples - base < ptvol::kTexels ? samples - base : ptvol::kTexels;
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live && lane < n) {
            uint32_t rng = ptsh::sample_rng(seed, firstSample, base + lane);
            float w[3];
            ptsh::direction(rng, w);
            e = make_float4(w[0], w[1], w[2], hits[(size_t)entry * samples + base + lane].x);
        }
        stage[wave][lane] = e;
        __syncthreads();
        for (uint32_t k = 0; k < n; ++k) {
            const float4 s = stage[wave][k];
            const float w[3] = {s.x, s.y, s.z};
            ptvol::accumulate(sw, s1, s2, d, w, s.w);
        }
        __syncthreads();
    }
    if (!live) return;
    float mean, mean2;
    ptvol::moments(sw, s1, s2, maxDistance, mean, mean2);
    ((float2*)(out + entry))[lane] = make_float2(mean, mean2);
}

__global__ __launch_bounds__(256) void pt_probe_grid_irradiance(PTProbeGrid G, const PTProbeCoeffs* __restrict__ sh, const PTProbeDepthMap* __restrict__ depth,
                                                                const PTReceiver* __restrict__ queries, uint32_t count, PTIrradiance* __restrict__ out)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= count) return;
    const float4 q0 = ((const float4*)queries)[2u * (size_t)q], q1 = ((const float4*)queries)[2u * (size_t)q + 1u];
    const float P[3] = {q0.x, q0.y, q0.z}, N[3] = {q1.x, q1.y, q1.z};
    float o[4];
    ptvol::lookup(G, P, N, [&](uint32_t probe, float co[27]) { pt_load_probe_sh(sh, probe, co); },
                  [&](uint32_t probe, uint32_t texel, float& mean, float& mean2) { pt_load_probe_depth(depth, probe, texel, mean, mean2); }, o);
    ((float4*)out)[q] = make_float4(o[0], o[1], o[2], o[3]);
}

} // namespace

hipError_t pt_launch_probe_depth_rays(const PTProbe* probes, uint32_t entries, uint32_t samples, uint32_t firstSample, float maxDistance, float4* rays,
                                      hipStream_t stream)
{
    const uint64_t slots = (uint64_t)entries * samples;
    if (samples == 0u || slots > ptvol::kChunkSamples) return hipErrorInvalidValue;
    if (slots == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_probe_depth_rays, dim3((uint32_t)((slots + 255u) / 256u)), dim3(256), 0, stream, probes, entries, samples, firstSample, maxDistance, rays);
    return hipGetLastError();
}

hipError_t pt_launch_probe_depth_resolve(const PTProbe* probes, uint32_t entries, uint32_t samples, uint32_t firstSample, float maxDistance,
                                         const float4* hits, PTProbeDepthMap* out, hipStream_t stream)
{
    if (samples == 0u || (uint64_t)entries * samples > ptvol::kChunkSamples) return hipErrorInvalidValue;
    if (entries == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_probe_depth_resolve, dim3((entries + kWaves - 1u) / kWaves), dim3(256), 0, stream, probes, entries, samples, firstSample, maxDistance,
                       hits, out);
    return hipGetLastError();
}

hipError_t pt_launch_probe_grid_irradiance(const PTProbeGrid& grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTReceiver* queries,
                                           uint32_t count, PTIrradiance* out, hipStream_t stream)
{
    if ((grid.flags & PT_GRID_VISIBILITY) && !depth) return hipErrorInvalidValue;
    if (count == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_probe_grid_irradiance, dim3((count + 255u) / 256u), dim3(256), 0, stream, grid, sh, depth, queries, count, out);
    return hipGetLastError();
}
