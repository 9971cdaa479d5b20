// pt_morph.h — morph targets, then the skin, on the device behind PTMorphGeometry (pt_morph.hip).
#pragma once
#include "pt_skin.h"

// One stream of a morph as PTSetMorph laid it out (morph_rule.h's MorphLayout): slot s of corner c is
// entries[sliceBase[c / 64] + 64 * s + c % 64], {dx, dy, dz, target as bits}, applied only if s < count[c].  entries == null: no stream.
struct PTMorphStream {
    const uint32_t* count;
    const uint32_t* sliceBase;
    const float4* entries;
};

// One BLAS's morph.  Every stored target was checked against targetCount on the host; `weights` holds targetCount floats and is
// the only thing the kernels index with them.
struct PTMorphArgs {
    const float4* rest;         // 3 * triCount rest positions (the morph's own)
    const float4* restAttrs;    // 8 rows per triangle, or null
    PTMorphStream position, normal, tangent;
    const float* weights;
    uint32_t triCount;
};

// floats of work space: 6 results (min.xyz, max.xyz), then 6 per workgroup of pt_morph_vertices
size_t pt_morph_work_floats(uint32_t triCount);
// pt_morph_vertices (3 * triCount vertices into outVerts, one box per workgroup), then pt_skin_bounds_fold (work[0 ... 5]).
// skin: the BLAS's skin and the palette (only joints, weights and palette are read), or null for a plain morph.
hipError_t pt_launch_morph_vertices(const PTMorphArgs& A, const PTSkinArgs* skin, float4* outVerts, float* work, hipStream_t stream);
// pt_morph_attrs: the triCount attribute records of the pose, each written once, to dstAttrs (the BLAS's first record)
hipError_t pt_launch_morph_attrs(const PTMorphArgs& A, const PTSkinArgs* skin, float4* dstAttrs, hipStream_t stream);
