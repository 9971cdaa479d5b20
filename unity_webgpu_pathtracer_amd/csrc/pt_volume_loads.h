// pt_volume_loads.h — how the lookup kernels (pt_probe_grid_irradiance in pt_volume.hip, pt_probe_grid_irradiance_placed in
// pt_placement.hip) read a probe's records: the load callables volume_rule.h's lookup takes, in the widths the records have.
#pragma once
#include "pt_device.h"
#include "volume_rule.h"

// seven 16-byte loads of coefficients
__device__ __forceinline__ void pt_load_probe_sh(const PTProbeCoeffs* __restrict__ sh, uint32_t probe, float co[27])
{
    const float4* s = (const float4*)(sh + probe);
#pragma unroll
    for (uint32_t t = 0; t < 7u; ++t) {
        const float4 v = s[t];
        co[4u * t] = v.x; co[4u * t + 1u] = v.y; co[4u * t + 2u] = v.z;
        if (t < 6u) co[4u * t + 3u] = v.w;
    }
}

// one 8-byte load of a texel's moments
__device__ __forceinline__ void pt_load_probe_depth(const PTProbeDepthMap* __restrict__ depth, uint32_t probe, uint32_t texel, float& mean, float& mean2)
{
    const float2 m = ((const float2*)(depth + probe))[texel];
    mean = m.x; mean2 = m.y;
}
