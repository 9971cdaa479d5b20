// bvh_refit.h — CWBVH refit (include/ptmi_plugin.h Part 9): what the host refit (bvh_refit.cpp) and the
// device refit (pt_refit.hip) share.  A refit keeps the topology (row n1, imask, record order, primIdx) and rewrites the
// triangle records, lo, the exponents and the 48 quantised bytes.  Every operation is exact or correctly rounded and both sides
// are compiled with -ffp-contract=off, so both give the same bytes.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "ptmi_layouts.h"

#if defined(__HIPCC__)
#define PT_REFIT_HD __host__ __device__ __forceinline__
#else
#define PT_REFIT_HD inline
#endif

namespace ptbvh {

// compare-and-select, not fminf / fmaxf: on +-0 and NaN the result is defined by the comparison alone, on either side
PT_REFIT_HD float refit_min(float acc, float b) { return b < acc ? b : acc; }
PT_REFIT_HD float refit_max(float acc, float b) { return b > acc ? b : acc; }

// bvh_builder_gpu.hip's quant_exponent: the smallest e with 255 * 2^e >= extent, clamped to -120 ... 126 (frexpf / ldexpf are
// exact).  An extent past FLT_MAX (finite corners whose difference overflows) takes the largest grid.
PT_REFIT_HD int refit_exponent(float extent)
{
    if (!(extent > 1e-36f)) return -120;
    if (!(extent <= 3.402823466e38f)) return 126;
    int k;
    const float m = frexpf(extent / 255.0f, &k);                   // extent / 255 = m * 2^k, m in [0.5, 1)
    int e = (m == 0.5f) ? k - 1 : k;
    while (extent / ldexpf(1.0f, e) > 255.0f) ++e;                 // rounding of the division above: at most one step
    return e < -120 ? -120 : (e > 126 ? 126 : e);
}

PT_REFIT_HD uint32_t refit_clamp_byte(float v) { return (uint32_t)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v)); }
// floor / ceil of a child's corner against the node's grid (origin lo, cell p = 2^e)
PT_REFIT_HD uint32_t refit_quant_lo(float c, float lo, float p) { return refit_clamp_byte(floorf((c - lo) / p)); }
PT_REFIT_HD uint32_t refit_quant_hi(float c, float lo, float p) { return refit_clamp_byte(ceilf((c - lo) / p)); }

// meta byte of an occupied slot: inner iff bits 3 and 4 are set (cwbvh_node_hitmask, pt_device.h); a leaf holds
// popcount(meta >> 5) records from record (meta & 31) of the node's triangle base
PT_REFIT_HD bool refit_slot_inner(uint32_t meta) { return (meta & 0x18u) == 0x18u; }

// The nodes of one BLAS ordered by depth (root first) and the level boundaries: level d is order[levelStart[d]] ...
// order[levelStart[d + 1] - 1], absolute node indices.  A refit runs the levels from the deepest to the root.
struct RefitPlan {
    std::vector<uint32_t> order;
    std::vector<uint32_t> levelStart;
};

// Walks the BLAS whose root is node nodeOff and whose records start at row triOff, as PTSetScene's validation walks it, and
// refuses (false, err set) whatever a refit could not follow safely: a node or record outside the arrays, a node reached twice,
// a leaf whose triangle bits are not 1, 3 or 7, records that are not exactly the triCount records from row triOff, each
// reached once, or a primIdx >= triCount.  triW: the .w word of triangle row r is triW[r * triWStride].
bool plan_refit(const PTFloat4* nodes, uint64_t nodeCount, const uint32_t* triW, size_t triWStride, uint64_t triRows,
                uint64_t nodeOff, uint64_t triOff, uint32_t triCount, RefitPlan& plan, std::string& err);

// Host refit of one BLAS inside the arrays, in place.  verts: 3 * triCount vertices in primitive order, finite.
bool refit_cwbvh(PTFloat4* nodes, uint64_t nodeCount, PTFloat4* tris, uint64_t triRows, uint64_t nodeOff, uint64_t triOff,
                 const PTFloat4* verts, uint32_t triCount, std::string& err);

} // namespace ptbvh
