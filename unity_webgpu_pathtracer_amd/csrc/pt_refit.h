// pt_refit.h — CWBVH refit on the device behind PTUpdateGeometry (pt_refit.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One BLAS inside the scene's node / triangle arrays.  Everything a kernel indexes with was checked on the host when the plan
// was made (ptbvh::plan_refit) and is never rewritten: row n1, imask, the records' primIdx.
struct PTRefitArgs {
    uint4* nodes;               // the generation being written: 5 x uint4 per node
    float4* tris;               // 3 x float4 per record
    const float4* verts;        // 3 * triCount vertices in primitive order
    float* nodeBox;             // 6 floats per node of the scene (mn.xyz, mx.xyz), written by the node's own launch
    const uint32_t* order;      // the BLAS's nodes by depth, absolute indices
    uint32_t nodeOff, triOff, triCount;
};

// pt_refit_tris, then one pt_refit_level per tree level from the deepest to the root, all on `stream`; levelStart: levels + 1
// boundaries into A.order (host memory).  launches += the kernels launched.
hipError_t pt_launch_refit(const PTRefitArgs& A, const uint32_t* levelStart, uint32_t levels, hipStream_t stream, uint32_t* launches);
// count attribute records (128 B) from src to dst; a record whose materialIndex is >= materialCount keeps dst's index
hipError_t pt_launch_refit_attrs(float4* dst, const float4* src, uint32_t count, uint32_t materialCount, hipStream_t stream);
