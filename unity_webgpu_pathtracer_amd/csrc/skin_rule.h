// skin_rule.h — linear-blend skinning (include/ptmi_plugin.h Part 11): the one definition of the rule, shared by
// the host twin (skin_host.cpp) and the kernels (pt_skin.hip).  Every operator is one IEEE binary32 operation, left to right;
// both sides are compiled with -ffp-contract=off, so both give the same bytes.  tests/skin_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string>
#include "ptmi_math.h"
#include "ptmi_plugin.h"

#if defined(__HIPCC__)
#define PT_SKIN_HD __host__ __device__ __forceinline__
#else
#define PT_SKIN_HD inline
#endif

namespace ptskin {

// One element of the blend matrix: all four terms, a zero weight is not skipped, the weights are not renormalised.
PT_SKIN_HD float skin_blend(float w0, float m0, float w1, float m1, float w2, float m2, float w3, float m3)
{
    return ((w0 * m0 + w1 * m1) + w2 * m2) + w3 * m3;
}

// B: the 12 elements of the blend matrix, three rows of four.  out = B * (x, y, z, 1)
PT_SKIN_HD void skin_point(const float B[12], float x, float y, float z, float out[3])
{
    for (int r = 0; r < 3; ++r) out[r] = ((B[4 * r] * x + B[4 * r + 1] * y) + B[4 * r + 2] * z) + B[4 * r + 3];
}

// A normal or tangent: v' = B3 * v, then normalize(v') = v' * (1 / sqrt(dot(v', v'))); a dot that is 0 or not
// finite keeps the rest vector.
PT_SKIN_HD void skin_direction(const float B[12], float x, float y, float z, float out[3])
{
    float t[3];
    for (int r = 0; r < 3; ++r) t[r] = (B[4 * r] * x + B[4 * r + 1] * y) + B[4 * r + 2] * z;
    const float d = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    if (d == 0.0f || !(pt_abs(d) <= 3.402823466e38f)) { out[0] = x; out[1] = y; out[2] = z; return; }
    const float s = 1.0f / pt_sqrt(d);
    out[0] = t[0] * s; out[1] = t[1] * s; out[2] = t[2] * s;
}

// compare-and-select, as bvh_refit.h's: defined by the comparison alone on either side
PT_SKIN_HD float skin_min(float acc, float b) { return b < acc ? b : acc; }
PT_SKIN_HD float skin_max(float acc, float b) { return b > acc ? b : acc; }

// ---- host side (skin_host.cpp) ----
// PTSetSkin's checks of the arrays: NULL arrays, jointCount, every joint index, finite weights and rest vertices, and (with
// materialCount != 0xFFFFFFFF and restAttrs) every materialIndex.  false: err has the reason.
bool skin_check(const PTSkinDesc& d, uint32_t triCount, uint32_t materialCount, std::string& err);
// matrices: jointCount x 12 floats, all finite
bool skin_check_palette(const float* matrices, uint32_t jointCount, std::string& err);
// The rule on the host for a checked desc: outVerts 3 * triCount; outAttrs (triCount records) and outBounds (6 floats) may be null.
void skin_host(const PTSkinDesc& d, uint32_t triCount, const float* matrices, PTFloat4* outVerts, PTTriangleAttributes* outAttrs, float* outBounds);

} // namespace ptskin
