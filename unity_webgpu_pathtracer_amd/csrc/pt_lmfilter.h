// pt_lmfilter.h — launcher of the lightmap denoiser's kernels (pt_lmfilter.hip; include/ptmi_plugin.h Part 17).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ptmi_plugin.h"

// The context's images of one atlas, width * height float4 each.
struct PTLmfImages {
    float4* state[2];           // (e.rgb, v): the levels go from one to the other
    float4* guideP;             // (P.xyz, h2)
    float4* guideN;             // (N.xyz, flags): 0 uncovered, 1 good, 2 bad
};

// scatter, footprint, `iterations` levels, collect; count > 0, the parameters and sizes checked by the caller
hipError_t pt_launch_lmfilter(const PTLightmapDenoiseParams& p, const PTLmfImages& im, const uint32_t* texels, const PTReceiver* recv, const PTIrradiance* irr,
                              uint64_t count, uint32_t width, uint32_t height, PTIrradiance* out, hipStream_t stream);
