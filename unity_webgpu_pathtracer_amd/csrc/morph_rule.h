// morph_rule.h — morph targets (include/ptmi_plugin.h Part 12): the one definition of the rule, shared by the host
// twin (morph_host.cpp) and the kernels (pt_morph.hip).  Every operator is one IEEE binary32 operation, left to right; both sides
// are compiled with -ffp-contract=off, so both give the same bytes.  The skin step is skin_rule.h's.  tests/morph_ref.py restates it.
#pragma once
#include <vector>
#include "skin_rule.h"

namespace ptmorph {

// One listed entry applied to one component: a product, then a sum, never fused.  Only listed entries reach this.
PT_SKIN_HD float morph_step(float acc, float w, float d) { return acc + w * d; }

// A morphed normal or tangent m without a palette: m * (1 / sqrt(dot(m, m))); a dot that is 0 or not finite keeps the REST vector.
PT_SKIN_HD void morph_direction(const float m[3], const float rest[3], float out[3])
{
    const float d = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    if (d == 0.0f || !(pt_abs(d) <= 3.402823466e38f)) { out[0] = rest[0]; out[1] = rest[1]; out[2] = rest[2]; return; }
    const float s = 1.0f / pt_sqrt(d);
    out[0] = m[0] * s; out[1] = m[1] * s; out[2] = m[2] * s;
}

// ... and with a palette: skin_rule.h's skin_direction of m, whose fallback here yields the REST vector, not m.  skin_direction
// falls back exactly when the dot of B3 * m is 0 or not finite, which is what `kept` restates with its operations.
PT_SKIN_HD void morph_skin_direction(const float B[12], const float m[3], const float rest[3], float out[3])
{
    float t[3];
    for (int r = 0; r < 3; ++r) t[r] = (B[4 * r] * m[0] + B[4 * r + 1] * m[1]) + B[4 * r + 2] * m[2];
    const float d = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    const bool kept = d == 0.0f || !(pt_abs(d) <= 3.402823466e38f);
    ptskin::skin_direction(B, m[0], m[1], m[2], out);
    if (kept) { out[0] = rest[0]; out[1] = rest[1]; out[2] = rest[2]; }
}

// ---- host side (morph_host.cpp) ----
// PTSetMorph's checks: NULL arrays, targetCount, every stream (offsets[0] == 0, non-decreasing, targets < targetCount and strictly
// ascending within a corner, finite deltas), finite rest vertices, a normal or tangent stream needs restAttrs, and (with
// materialCount != 0xFFFFFFFF and restAttrs) every materialIndex.  false: err has the reason.
bool morph_check(const PTMorphDesc& d, uint32_t triCount, uint32_t materialCount, std::string& err);
// weights: targetCount floats, all finite
bool morph_check_weights(const float* weights, uint32_t targetCount, std::string& err);
// The rule on the host for a checked desc.  skin and matrices both set: morph, then skin (skin's joints and weights only); both
// null: a plain morph.  outVerts 3 * triCount; outAttrs (triCount records, needs d.restAttrs) and outBounds (6 floats) may be null.
void morph_host(const PTMorphDesc& d, const PTSkinDesc* skin, uint32_t triCount, const float* weights, const float* matrices, PTFloat4* outVerts,
                PTTriangleAttributes* outAttrs, float* outBounds);

// One checked CSR stream as the kernels read it: SELL-64, sliced ELL with one slice per 64 consecutive corners.  Slot s of slice k
// is the 64 contiguous entries from sliceBase[k] + 64 * s, one per corner of the slice; a corner's own length is count[c], and a
// slot at or past it is padding (zeroes) that no lane applies.
struct MorphLayout {
    std::vector<uint32_t> count, sliceBase;
    std::vector<PTMorphEntry> entries;
};
// stored entries (padding included) of the stream's layout
uint64_t morph_layout_size(const uint32_t* offsets, uint32_t cornerCount);
// false: the stored entries do not fit 32 bits
bool morph_layout(const uint32_t* offsets, const PTMorphEntry* entries, uint32_t cornerCount, MorphLayout& out);

} // namespace ptmorph
