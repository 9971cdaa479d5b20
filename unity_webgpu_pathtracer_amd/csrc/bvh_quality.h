// bvh_quality.h — the tree-quality measure of a CWBVH (include/ptmi_plugin.h Part 10): what the host measure
// (bvh_quality.cpp, behind PTMeasureBVHArrays) and the device measure (pt_quality.hip, behind PTMeasureGeometry) share.
//
// cost = 1 + sum over every occupied slot of every reachable node of halfArea(slot) / rootHalfArea * weight(slot), with weight 1
// for an inner slot and popcount(meta >> 5) for a leaf slot; halfArea = ex*ey + ey*ez + ez*ex of the slot's decoded extent
// (q_hi - q_lo) * 2^e; rootHalfArea is that of the fold of the root's occupied slots' decoded boxes lo + q * 2^e.  All float64.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string>
#include "ptmi_layouts.h"

#if defined(__HIPCC__)
#define PT_QUALITY_HD __host__ __device__ __forceinline__
#else
#define PT_QUALITY_HD inline
#endif

namespace ptbvh {

// 2^e of an exponent byte of row n0 (a signed 8-bit value)
PT_QUALITY_HD double quality_cell(uint32_t byte) { return ldexp(1.0, (int)(int8_t)(uint8_t)byte); }

PT_QUALITY_HD float quality_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// One node's 20 words (5 x uint4, PTCwbvhNode).  Returns the node's term: the sum of halfArea * weight over its occupied slots.
// foldHalfArea: the half area of the fold of the occupied slots' decoded boxes (what the root contributes), 0 without any.
PT_QUALITY_HD double quality_node_term(const uint32_t w[20], double& foldHalfArea)
{
    const double cell[3] = {quality_cell(w[3] & 255u), quality_cell((w[3] >> 8) & 255u), quality_cell((w[3] >> 16) & 255u)};
    double sum = 0.0;
    uint32_t foldLo[3] = {255u, 255u, 255u}, foldHi[3] = {0u, 0u, 0u};
    bool any = false;
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s) {
        const uint32_t m = (w[6u + (s >> 2)] >> (8u * (s & 3u))) & 255u;
        if (m == 0u) continue;
        double e[3];
#pragma unroll
        for (uint32_t a = 0; a < 3u; ++a) {
            // byte s of the axis' eight low bytes (row 2 on: lo x, lo y, lo z, hi x, hi y, hi z) and of its high bytes
            const uint32_t lo = (w[8u + 2u * a + (s >> 2)] >> (8u * (s & 3u))) & 255u;
            const uint32_t hi = (w[14u + 2u * a + (s >> 2)] >> (8u * (s & 3u))) & 255u;
            e[a] = ((double)hi - (double)lo) * cell[a];
            foldLo[a] = lo < foldLo[a] ? lo : foldLo[a];
            foldHi[a] = hi > foldHi[a] ? hi : foldHi[a];
        }
        const bool inner = (m & 0x18u) == 0x18u;
        const uint32_t bits = m >> 5;
        const double weight = inner ? 1.0 : (double)((bits & 1u) + ((bits >> 1) & 1u) + ((bits >> 2) & 1u));
        sum += (e[0] * e[1] + e[1] * e[2] + e[2] * e[0]) * weight;
        any = true;
    }
    // lo + q * 2^e per corner: the origin cancels in the extent only in exact arithmetic, so it is added as the rule says
    double ext[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (uint32_t a = 0; a < 3u; ++a) {
        const double origin = (double)quality_f32(w[a]);
        if (any) ext[a] = (origin + (double)foldHi[a] * cell[a]) - (origin + (double)foldLo[a] * cell[a]);
    }
    foldHalfArea = ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0];
    return sum;
}

struct Quality {
    uint32_t nodeCapacity = 0, nodeCount = 0, triangleCount = 0, levels = 0;
    double rootHalfArea = 0.0, sahCost = 0.0;
};

// Host measure of the CWBVH in the arrays (root = node 0, records from row 0).  Walks it as the refit does (plan_refit) and
// refuses, with err set, whatever is not a CWBVH of triCount triangles.
bool measure_cwbvh(const PTFloat4* nodes, uint64_t nodeCount, const PTFloat4* tris, uint64_t triRows, uint32_t triCount, Quality& out, std::string& err);

} // namespace ptbvh
