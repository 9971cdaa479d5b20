// pt_placement.hip — probe placement (include/ptmi_plugin.h Part 18): the kernels on either side of the
// closest-hit query with surface records of one placement step.
//
//     pt_probe_place_rays       one lane per (probe, sample): the PTRay {P + o, w_j, maxDistance, 0}, o the probe's stored offset
//                               as the rule reads it
//     [ pt_launch_query ]       pt_query.hip's closest-hit kernel with surface records, unchanged
//     pt_probe_place_step       one WAVE per probe, lane l owns the samples j = l (mod 64): one 16-byte load of the hit record and, on
//                               a hit, one of the surface record's normal row; two counters and three 64-bit keys per lane, merged
//                               by an xor butterfly of integer min / max / add; lane 0 stores 16 bytes (and 32 of statistics)
//     pt_probe_grid_irradiance_placed   the placed lookup: Part 16's with a corner standing at its placed position or left out
//
// The arithmetic is placement_rule.h's, which the host twin evaluates too.  A direction is made from the seed wherever it is
// needed, as the depth resolve makes it: the step kernel then does not depend on the ray scratch, and the twin has no rays.
#include "pt_device.h"
#include "pt_launch.h"
#include "placement_rule.h"
#include "pt_volume_loads.h"

namespace {

constexpr uint32_t kWaves = 4u;             // probes per workgroup of the step

__device__ __forceinline__ void stored_offset(const PTProbePlaceParams& Q, const PTProbePlacement* __restrict__ placement, uint32_t entry, float o[3])
{
    const float4 s = ((const float4*)placement)[entry];
    const float stored[3] = {s.x, s.y, s.z};
    ptplace::read_offset(Q, stored, o);
}

__global__ __launch_bounds__(256) void pt_probe_place_rays(const PTProbe* __restrict__ probes, uint32_t entries, uint32_t samples, uint32_t firstSample,
                                                           PTProbePlaceParams Q, const PTProbePlacement* __restrict__ placement, float4* __restrict__ rays)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const uint32_t entry = slot / samples, j = slot - entry * samples;
    if (entry >= entries) return;
    const float4 p = ((const float4*)probes)[entry];
    float o[3];
    stored_offset(Q, placement, entry, o);
    uint32_t rng = ptsh::sample_rng(pt_asuint(p.w), firstSample, j);
    float w[3];
    ptsh::direction(rng, w);
    rays[2u * (size_t)slot] = make_float4(p.x + o[0], p.y + o[1], p.z + o[2], w[0]);
    rays[2u * (size_t)slot + 1u] = make_float4(w[1], w[2], Q.maxDistance, pt_asfloat(0u));
}

// Four probes per workgroup.  A wave whose probe is past the end walks the loop with its loads guarded and stores nothing.
__global__ __launch_bounds__(256) void pt_probe_place_step(const PTProbe* __restrict__ probes, uint32_t entries, uint32_t samples, uint32_t firstSample,
                                                           PTProbePlaceParams Q, const float4* __restrict__ hits, const float4* __restrict__ surfaces, uint32_t move,
                                                           PTProbePlacement* __restrict__ placement, PTProbePlaceStats* __restrict__ stats)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t entry = blockIdx.x * kWaves + wave;
    const bool live = entry < entries;
    uint32_t seed = 0u;
    if (live) seed = pt_asuint(((const float4*)probes)[entry].w);
    ptplace::Tally T = ptplace::empty();
    for (uint32_t j = lane; j < samples; j += ptsh::kLanes) {
        if (!live) continue;
        const size_t slot = (size_t)entry * samples + j;
        const float4 h = hits[slot];
        if (pt_asuint(h.w) == ptplace::kNone) continue;         // a miss: its surface record is not read
        const float4 nr = surfaces[3u * slot + 1u];
        uint32_t rng = ptsh::sample_rng(seed, firstSample, j);
        float w[3];
        ptsh::direction(rng, w);
        const float n[3] = {nr.x, nr.y, nr.z};
        ptplace::add_hit(T, j, h.x, w, n);
    }
    // integer min / max / add: exact in any order, and after the butterfly every lane holds the probe's tally
    for (uint32_t m = 32u; m >= 1u; m >>= 1) {
        ptplace::Tally o;
        o.back = __shfl_xor(T.back, m, 64);
        o.front = __shfl_xor(T.front, m, 64);
        o.nearestBack = __shfl_xor((unsigned long long)T.nearestBack, m, 64);
        o.nearestFront = __shfl_xor((unsigned long long)T.nearestFront, m, 64);
        o.farthestFront = __shfl_xor((unsigned long long)T.farthestFront, m, 64);
        ptplace::merge(T, o);
    }
    if (!live || lane != 0u) return;
    const PTProbePlaceStats s = ptplace::stats_of(T);
    float o[3];
    stored_offset(Q, placement, entry, o);
    const uint32_t state = ptplace::finish(Q, seed, firstSample, samples, s, move != 0u, o);
    ((float4*)placement)[entry] = make_float4(o[0], o[1], o[2], pt_asfloat(state));
    if (stats) {
        float4* d = (float4*)(stats + entry);
        d[0] = make_float4(pt_asfloat(s.back), pt_asfloat(s.front), pt_asfloat(s.nearestBack), pt_asfloat(s.nearestFront));
        d[1] = make_float4(pt_asfloat(s.farthestFront), s.tNearestBack, s.tNearestFront, s.tFarthestFront);
    }
}

// One lane per query, as pt_probe_grid_irradiance (pt_volume.hip) with its loads: volume_rule.h's lookup with the placement loaded,
// one more 16-byte load per corner that has a trilinear weight.
__global__ __launch_bounds__(256) void pt_probe_grid_irradiance_placed(PTProbeGrid G, const PTProbeCoeffs* __restrict__ sh, const PTProbeDepthMap* __restrict__ depth,
                                                                       const PTProbePlacement* __restrict__ placement, const PTReceiver* __restrict__ queries,
                                                                       uint32_t count, PTIrradiance* __restrict__ out)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= count) return;
    const float4 q0 = ((const float4*)queries)[2u * (size_t)q], q1 = ((const float4*)queries)[2u * (size_t)q + 1u];
    const float P[3] = {q0.x, q0.y, q0.z}, N[3] = {q1.x, q1.y, q1.z};
    float o[4];
    ptvol::lookup(G, P, N, [&](uint32_t probe, float co[27]) { pt_load_probe_sh(sh, probe, co); },
                  [&](uint32_t probe, uint32_t texel, float& mean, float& mean2) { pt_load_probe_depth(depth, probe, texel, mean, mean2); },
                  [&](uint32_t probe, float off[3], uint32_t& state) {
                      const float4 v = ((const float4*)placement)[probe];
                      off[0] = v.x; off[1] = v.y; off[2] = v.z;
                      state = pt_asuint(v.w);
                  },
                  o);
    ((float4*)out)[q] = make_float4(o[0], o[1], o[2], o[3]);
}

} // namespace

hipError_t pt_launch_probe_grid_irradiance_placed(const PTProbeGrid& grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTProbePlacement* placement,
                                                  const PTReceiver* queries, uint32_t count, PTIrradiance* out, hipStream_t stream)
{
    if (((grid.flags & PT_GRID_VISIBILITY) && !depth) || !placement) return hipErrorInvalidValue;
    if (count == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_probe_grid_irradiance_placed, dim3((count + 255u) / 256u), dim3(256), 0, stream, grid, sh, depth, placement, queries, count, out);
    return hipGetLastError();
}

hipError_t pt_launch_probe_place_rays(const PTProbe* probes, uint32_t entries, uint32_t samples, uint32_t firstSample, const PTProbePlaceParams& params,
                                      const PTProbePlacement* placement, float4* rays, hipStream_t stream)
{
    const uint64_t slots = (uint64_t)entries * samples;
    if (samples == 0u || slots > ptplace::kChunkSamples) return hipErrorInvalidValue;
    if (slots == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_probe_place_rays, dim3((uint32_t)((slots + 255u) / 256u)), dim3(256), 0, stream, probes, entries, samples, firstSample, params,
                       placement, rays);
    return hipGetLastError();
}

hipError_t pt_launch_probe_place_step(const PTProbe* probes, uint32_t entries, uint32_t samples, uint32_t firstSample, const PTProbePlaceParams& params,
                                      const float4* hits, const float4* surfaces, bool move, PTProbePlacement* placement, PTProbePlaceStats* stats,
                                      hipStream_t stream)
{
    if (samples == 0u || (uint64_t)entries * samples > ptplace::kChunkSamples) return hipErrorInvalidValue;
    if (entries == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_probe_place_step, dim3((entries + kWaves - 1u) / kWaves), dim3(256), 0, stream, probes, entries, samples, firstSample, params, hits,
                       surfaces, move ? 1u : 0u, placement, stats);
    return hipGetLastError();
}
