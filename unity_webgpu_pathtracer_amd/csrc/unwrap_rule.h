// unwrap_rule.h — lightmap UVs (include/ptmi_plugin.h Part 23): the one definition of the unwrap rule, shared by the
// host twin (unwrap_host.cpp) and the kernels (pt_unwrap.hip).  Charts are decided on bits and integers; every fp32 operator is one
// IEEE binary32 operation, left to right, and both sides are compiled with -ffp-contract=off, so both give the same bytes.
// tests/unwrap_ref.py restates it in numpy.
//
// Corners.  Primitive p of a BLAS of T triangles has corners c0, c1, c2: rows 3p, 3p + 1, 3p + 2 (x, y, z; w is not read) of the
//   caller's vertex array -- the array PTUpdateGeometryDevice takes, NOT checked against what the BLAS holds --, or, without one,
//   v0, v0 + e1, v0 + e2 per component of the current triangle record whose primIdx is p.  Every component then has + 0.0f applied:
//   -0 and +0 are one value.  The record form WELDS LESS: v0 + e1 is not always the float the neighbour's record stores for the
//   same vertex, so some shared edges are not found and a mesh falls into a few more charts (Sponza-class scene: 494 for 483, the
//   material zoo 86 for 54).  The atlas is valid either way.
// Class.  g = cross3(c1 - c0, c2 - c0) (cross3's expression on the differences).  p is EXCLUDED when a corner component is not
//   finite or dot3(g, g) is 0 or not finite.  Otherwise the axis a is the component of largest |g|, a later axis winning only by >,
//   and cls = 2 a + (g[a] < 0): six classes; the front and the back of a thin wall never share a chart.
// Links.  Two included primitives of one class are linked when an edge of one and an edge of the other are the same unordered pair
//   of corner values, all 96 bits of each corner equal.  An edge three or more primitives share links all of them that have the same
//   class.  A chart is a connected component of the links; its label is its lowest primIdx; charts are listed in ascending label, and
//   chartOfPrim[p] is the chart's place in that list, kNoChart for an excluded p.  The result depends on the set of inputs only.
// Extents.  A chart of axis a has U = c[(a + 1) % 3], V = c[(a + 2) % 3]; umin, umax, vmin, vmax are the fp32 minimum and maximum
//   over its corners (exact).  The record is PTUnwrapChart.
// Size.  w = (uint32)ceilf((umax - umin) * tpu) + 1 + 2 * padding, h likewise; a product that is not finite or above 8192 does not fit.
// Packing.  Charts in the order h descending, w descending, label (firstPrim, then place in the list) ascending, on shelves: x = y =
//   shelf = 0; w > width fails; x + w > width opens a shelf (y += shelf; x = 0; shelf = 0); the first chart of a shelf sets shelf = h;
//   y + h > height fails; the origin is (x, y); x += w.  rowsUsed = y + shelf is set whenever every width fits.
// UVs.  u_k = ((((U_k - umin) * tpu) + (float)(ox + padding)) + 0.5f) / (float)width, v_k with V, vmin, oy, height.  umin lands on a
//   texel centre, so an axis-aligned a x b rectangle covers exactly (floor(a tpu) + 1)(floor(b tpu) + 1) texels under
//   PTRasterizeChart's inclusive edges.  No mirroring is undone: the rasteriser takes mirrored charts.  An excluded primitive gets six
//   quiet NaNs (0x7FC00000), which is how PTRasterizeChart leaves a triangle out.
// Not done: overlap detection inside a chart.  A surface that winds over itself while keeping one facing (a helical ramp) projects
//   onto itself, and the lowest primitive owns the texel, as Part 14 says.  No mean-plane or conformal parameterisation: a face
//   tilted 45 degrees gets 0.71 of the density, the worst case 0.58.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string>
#include "ptmi_math.h"
#include "ptmi_plugin.h"

#if defined(__HIPCC__)
#define PT_UNWRAP_HD __host__ __device__ __forceinline__
#else
#define PT_UNWRAP_HD inline
#endif

namespace ptunwrap {

constexpr uint32_t kNoChart = PT_UNWRAP_NO_CHART;
constexpr uint32_t kExcluded = 0xFFu;              // the class word of an excluded primitive
constexpr uint32_t kMaxSize = PT_CHART_MAX_SIZE;
constexpr uint32_t kMaxPadding = PT_UNWRAP_MAX_PADDING;
constexpr uint32_t kQuietNaN = 0x7FC00000u;

PT_UNWRAP_HD bool unwrap_finite(float v) { return pt_abs(v) <= 3.402823466e38f; }

PT_UNWRAP_HD uint32_t unwrap_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
PT_UNWRAP_HD float unwrap_float(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }

// v[a] without an indexed register array
PT_UNWRAP_HD float unwrap_pick(const float v[3], uint32_t a) { return a == 0u ? v[0] : a == 1u ? v[1] : v[2]; }

// bits(n): the width of the largest vertex id, n - 1 (n >= 1)
PT_UNWRAP_HD uint32_t unwrap_id_bits(uint64_t n)
{
    uint32_t b = 1u;
    while (b < 63u && ((uint64_t)1 << b) < n) ++b;
    return b;
}
// an edge key holds two vertex ids below 3 T and a class: 2 * bits(3 T) + 3 <= 64
PT_UNWRAP_HD bool unwrap_count_fits(uint64_t triCount) { return triCount >= 1u && triCount <= 0xFFFFFFFEull / 3u && 2u * unwrap_id_bits(3u * triCount) + 3u <= 64u; }

// c: the three corners, + 0.0f applied here.  kExcluded, or the class 0 .. 5
PT_UNWRAP_HD uint32_t unwrap_class(float c[3][3])
{
    bool ok = true;
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) {
            c[k][a] = c[k][a] + 0.0f;
            ok = unwrap_finite(c[k][a]) && ok;
        }
    if (!ok) return kExcluded;
    const float e1[3] = {c[1][0] - c[0][0], c[1][1] - c[0][1], c[1][2] - c[0][2]};
    const float e2[3] = {c[2][0] - c[0][0], c[2][1] - c[0][1], c[2][2] - c[0][2]};
    float g[3];
    g[0] = e1[1] * e2[2] - e1[2] * e2[1];
    g[1] = e1[2] * e2[0] - e1[0] * e2[2];
    g[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const float d = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    if (!(d != 0.0f && unwrap_finite(d))) return kExcluded;
    uint32_t a = 0u;
    float m = pt_abs(g[0]);
    if (pt_abs(g[1]) > m) { a = 1u; m = pt_abs(g[1]); }
    if (pt_abs(g[2]) > m) a = 2u;
    return 2u * a + (unwrap_pick(g, a) < 0.0f ? 1u : 0u);
}

// (lo id, hi id, class) in 64 bits; idBits = unwrap_id_bits(3 T).  Never all ones: lo < hi for a primitive with area
PT_UNWRAP_HD uint64_t unwrap_edge_key(uint32_t ida, uint32_t idb, uint32_t cls, uint32_t idBits)
{
    const uint64_t lo = ida < idb ? ida : idb, hi = ida < idb ? idb : ida;
    return (lo << (idBits + 3u)) | (hi << 3) | (uint64_t)cls;
}

// an unsigned word that orders as the float does (no NaN comes here; -0 does not exist after + 0.0f), and back
PT_UNWRAP_HD uint32_t unwrap_order_key(float v) { const uint32_t u = unwrap_bits(v); return (u >> 31) ? ~u : (u | 0x80000000u); }
PT_UNWRAP_HD float unwrap_order_value(uint32_t k) { return unwrap_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

// one side of a chart's rectangle in texels; false: it does not fit any atlas
PT_UNWRAP_HD bool unwrap_side(float mn, float mx, float tpu, uint32_t padding, uint32_t& out)
{
    const float s = (mx - mn) * tpu;
    if (!(s >= 0.0f && s <= (float)kMaxSize)) return false;
    out = (uint32_t)ceilf(s) + 1u + 2u * padding;
    return true;
}

PT_UNWRAP_HD float unwrap_coord(float x, float mn, float tpu, int32_t origin, uint32_t padding, uint32_t size)
{
    return ((((x - mn) * tpu) + (float)(origin + (int32_t)padding)) + 0.5f) / (float)size;
}

// The six UVs of a primitive of chart `ch` placed at (ox, oy); c: its corners with + 0.0f applied
PT_UNWRAP_HD void unwrap_uvs(const float c[3][3], const PTUnwrapChart& ch, int32_t ox, int32_t oy, uint32_t width, uint32_t height, uint32_t padding,
                             float tpu, float uv[6])
{
    const uint32_t a = ch.cls >> 1, ua = (a + 1u) % 3u, va = (a + 2u) % 3u;
    for (int k = 0; k < 3; ++k) {
        uv[2 * k] = unwrap_coord(unwrap_pick(c[k], ua), ch.umin, tpu, ox, padding, width);
        uv[2 * k + 1] = unwrap_coord(unwrap_pick(c[k], va), ch.vmin, tpu, oy, padding, height);
    }
}

// v0, e1, e2 of a triangle record -> its corners (before + 0.0f)
PT_UNWRAP_HD void unwrap_record_corners(const float v0[3], const float e1[3], const float e2[3], float c[3][3])
{
    for (int a = 0; a < 3; ++a) { c[0][a] = v0[a]; c[1][a] = v0[a] + e1[a]; c[2][a] = v0[a] + e2[a]; }
}

// ---- what both sides check (the message names the caller) ----
inline bool unwrap_check_atlas(uint32_t width, uint32_t height, uint32_t padding, float tpu, const char* who, std::string& err)
{
    if (width < 1u || width > kMaxSize || height < 1u || height > kMaxSize) {
        err = std::string(who) + ": width x height = " + std::to_string(width) + " x " + std::to_string(height) + " (each 1 ... 8192)";
        return false;
    }
    if (padding > kMaxPadding) { err = std::string(who) + ": padding = " + std::to_string(padding) + " (0 ... 16)"; return false; }
    if (!(tpu > 0.0f && unwrap_finite(tpu))) { err = std::string(who) + ": texelsPerUnit is not finite or <= 0"; return false; }
    return true;
}
inline bool unwrap_check_count(int64_t triCount, const char* who, std::string& err)
{
    if (triCount <= 0) { err = std::string(who) + ": triangleCount <= 0"; return false; }
    if (!unwrap_count_fits((uint64_t)triCount)) {
        err = std::string(who) + ": triangleCount = " + std::to_string(triCount) + " does not fit the edge key (2 * bits(3 T) + 3 <= 64)";
        return false;
    }
    return true;
}

// ---- host side (unwrap_host.cpp) ----
// tris: the BLAS's 3 * triCount rows (may be null with vertices); vertices: 3 * triCount rows or null.  chartOfPrim / charts both
// null: only the count.  false: err has the reason; a count above the capacity is one (count is set, nothing is written).
bool unwrap_charts_host(const PTFloat4* tris, const PTFloat4* vertices, uint32_t triCount, uint32_t* chartOfPrim, PTUnwrapChart* charts, uint32_t capacity,
                        uint32_t& count, PTUnwrapStats* stats, std::string& err);
// origins: x, y per chart.  false with rowsUsed set: the rows do not fit the height; false with rowsUsed = 0: a chart is too wide
bool pack_charts_host(const PTUnwrapChart* charts, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float tpu, int32_t* origins,
                      uint32_t& rowsUsed, std::string& err);
bool emit_uvs_host(const PTFloat4* tris, const PTFloat4* vertices, uint32_t triCount, const uint32_t* chartOfPrim, const PTUnwrapChart* charts,
                   const int32_t* origins, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float tpu, float* uvs, std::string& err);

} // namespace ptunwrap
