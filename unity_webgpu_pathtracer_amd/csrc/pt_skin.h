// pt_skin.h — linear-blend skinning on the device behind PTSkinGeometry (pt_skin.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One BLAS's skin as PTSetSkin uploaded it.  Every joint index was checked against jointCount on the host; the palette holds
// jointCount x 3 float4 (the rows of the 3x4 matrices) and is the only thing the kernels index with them.
struct PTSkinArgs {
    const float4* rest;         // 3 * triCount rest positions
    const uint2* joints;        // 4 x uint16 per vertex
    const float4* weights;      // 4 floats per vertex
    const float4* restAttrs;    // 8 rows per triangle, or null
    const float4* palette;
    uint32_t triCount;
};

// floats of work space: 6 results (min.xyz, max.xyz), then 6 per workgroup of pt_skin_vertices
size_t pt_skin_work_floats(uint32_t triCount);
// pt_skin_vertices (3 * triCount skinned vertices into outVerts, one box per workgroup), then pt_skin_bounds_fold (work[0 ... 5])
hipError_t pt_launch_skin_vertices(const PTSkinArgs& A, float4* outVerts, float* work, hipStream_t stream);
// pt_skin_bounds_fold alone: `count` boxes of 6 floats (min.xyz, max.xyz) at `partial`, folded in index order into out[0 ... 5]
hipError_t pt_launch_skin_bounds_fold(const float* partial, uint32_t count, float* out, hipStream_t stream);
// pt_skin_attrs: the triCount attribute records of the skinned pose, each written once, to dstAttrs (the BLAS's first record)
hipError_t pt_launch_skin_attrs(const PTSkinArgs& A, float4* dstAttrs, hipStream_t stream);
