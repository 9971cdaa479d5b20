// light_grid_rule.h — the light grid of the culled direct-light calls (include/ptmi_plugin.h Part 25): the one
// definition of which cell a point falls into and of which cells list a light, shared by the build kernels (pt_light_grid.hip),
// the culled pair loop (pt_direct.hip) and the host twin (light_grid_host.cpp).  Every fp32 operator is one IEEE binary32
// operation in the order written, and all sides are compiled with -ffp-contract=off, so all give the same bits.
// tests/light_grid_ref.py restates it from this text.
//
// The grid: dims[0] x dims[1] x dims[2] cubes of cellSize from origin; cells = dims[0] * dims[1] * dims[2].
//
// The cell of a point X.  Per axis a: t = (X[a] - origin[a]) / cellSize (one subtraction, one division); the point is inside on
// the axis iff t >= 0.0f and t < (float)dims[a] (a NaN is outside); i[a] = (uint32_t)t.  Inside on all three axes: cell =
// (i[2] * dims[1] + i[1]) * dims[0] + i[0].  Otherwise cell = cells, the overflow cell, whose list is every light 0 ... L-1.
//
// The box of cell (i0, i1, i2), inflated.  Per axis a: pad = cellSize * 2^-10 + (|origin[a]| + cellSize * (float)dims[a]) * 2^-20
// (the products first, then the inner sum, then the outer); lo = (origin[a] + cellSize * (float)i[a]) - pad; hi = (origin[a] +
// cellSize * (float)(i[a] + 1)) + pad.  DESIGN.md 5.30 derives that every point the cell rule maps to the cell lies inside.
//
// Cell (i0, i1, i2) lists light l unless one of these holds, tested in this order:
//   type       the type is not point, spot or rectangle (a directional light and an unknown type have no pairs);
//   emission   none of emission[c] != 0.0f is true: every channel is +0 or -0, so every Li is 0 (or not finite) whatever the BRDF.
//              (A negative channel stays listed: with a material whose colour is negative too its pair could count);
//   reach      C = position for a point or spot light and position + 0.5f * u + 0.5f * v ((position[a] + 0.5f * u[a]) + 0.5f *
//              v[a]) for a rectangle; R = range, for a rectangle range + 0.5f * (sqrt(dot(u, u)) + sqrt(dot(v, v))); Rr = R *
//              1.0009765625f (1 + 2^-10); R2 = Rr * Rr.  Per axis d[a] = C[a] < lo ? lo - C[a] : (C[a] > hi ? C[a] - hi : 0.0f);
//              d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2].  The light is culled iff d2 > R2 is TRUE: a NaN or an infinity
//              anywhere keeps it listed;
//   half-space a rectangle, or a spot whose outer cosine v[0] >= 0.0f: with c[a] = (lo + hi) * 0.5f, h[a] = (hi - lo) * 0.5f and N
//              the light's derived row (direct_rule.h derive_rows), e[a] = c[a] - position[a]; s = dot(e, N) + ((|N[0]| * h[0] +
//              |N[1]| * h[1]) + |N[2]| * h[2]); the light is culled iff s + Rr * 2^-16 < 0.0f is TRUE.  The margin is for the
//              pair rule's own rounding: it decides by an fp32 cosine, a few 2^-24 off, of a vector no longer than Rr.
// dot is direct_rule.h's: (a0 * b0 + a1 * b1) + a2 * b2.
//
// Why culling is exact: a pair that counts has a positive channel of ((Li * f) * nl) * w, so a nonzero emission channel and a
// nonzero falloff: lsDistance <= range from a point of the light (reach, by the triangle inequality over the rectangle's half
// diagonals), and for a rectangle or a spot with v[0] >= 0 a cosine that is not negative: the true one lies above -2^-20, so the
// point lies less than Rr * 2^-20 behind the light's plane (half-space).  Nothing is assumed of the material.
#pragma once
#include "direct_rule.h"

#define PT_LGRID_HD PT_DIRECT_HD

namespace ptlgrid {

constexpr uint32_t kMaxDim = 256u;
constexpr uint32_t kMaxCells = 1u << 20;
constexpr uint32_t kNoLight = 0xFFFFFFFFu;

struct Grid {
    float origin[3];
    float cellSize;
    uint32_t dims[3];
};

PT_LGRID_HD uint32_t cell_count(const Grid& g) { return g.dims[0] * g.dims[1] * g.dims[2]; }

PT_LGRID_HD uint32_t cell_of(const Grid& g, const float X[3])
{
    uint32_t i[3];
    bool inside = true;
    for (uint32_t a = 0; a < 3u; ++a) {
        const float t = (X[a] - g.origin[a]) / g.cellSize;
        const bool in = t >= 0.0f && t < (float)g.dims[a];
        i[a] = in ? (uint32_t)t : 0u;
        inside = inside && in;
    }
    return inside ? (i[2] * g.dims[1] + i[1]) * g.dims[0] + i[0] : cell_count(g);
}

// the inflated box of cell (i[0], i[1], i[2])
PT_LGRID_HD void cell_box(const Grid& g, const uint32_t i[3], float lo[3], float hi[3])
{
    for (uint32_t a = 0; a < 3u; ++a) {
        const float pad = g.cellSize * 0.0009765625f + (pt_abs(g.origin[a]) + g.cellSize * (float)g.dims[a]) * 9.5367431640625e-07f;
        lo[a] = (g.origin[a] + g.cellSize * (float)i[a]) - pad;
        hi[a] = (g.origin[a] + g.cellSize * (float)(i[a] + 1u)) + pad;
    }
}

// whether the cell with the inflated box [lo, hi] lists the light (N: its derived row)
PT_LGRID_HD bool lists(const ptdirect::Light& l, const float lo[3], const float hi[3])
{
    const bool rect = l.type == PT_LIGHT_TYPE_RECTANGLE, spot = l.type == PT_LIGHT_TYPE_SPOT;
    if (!(rect || spot || l.type == PT_LIGHT_TYPE_POINT)) return false;
    if (!(l.emission[0] != 0.0f || l.emission[1] != 0.0f || l.emission[2] != 0.0f)) return false;
    float R = l.range;
    if (rect) R = l.range + 0.5f * (pt_sqrt(ptdirect::dot(l.u, l.u)) + pt_sqrt(ptdirect::dot(l.v, l.v)));
    const float Rr = R * 1.0009765625f;
    const float R2 = Rr * Rr;
    float d[3];
    for (uint32_t a = 0; a < 3u; ++a) {
        const float C = rect ? (l.position[a] + 0.5f * l.u[a]) + 0.5f * l.v[a] : l.position[a];
        d[a] = C < lo[a] ? lo[a] - C : (C > hi[a] ? C - hi[a] : 0.0f);
    }
    const float d2 = ptdirect::dot(d, d);
    if (d2 > R2) return false;
    if (rect || (spot && l.v[0] >= 0.0f)) {
        float e[3], h[3];
        for (uint32_t a = 0; a < 3u; ++a) {
            e[a] = (lo[a] + hi[a]) * 0.5f - l.position[a];
            h[a] = (hi[a] - lo[a]) * 0.5f;
        }
        const float s = ptdirect::dot(e, l.N) + ((pt_abs(l.N[0]) * h[0] + pt_abs(l.N[1]) * h[1]) + pt_abs(l.N[2]) * h[2]);
        if (s + Rr * 1.52587890625e-05f < 0.0f) return false;
    }
    return true;
}

// ---- the host twin and the checks the entry points share (light_grid_host.cpp); false: err says why ----
bool check_params(const PTLightGridParams* p, std::string& err);
// offsets: cells + 2 words; rectBefore: lightCount + 1 words; indices: indexCapacity words, may be null with a capacity of 0.
// *outTotal (may be null): the entries of all lists; indices are written only when they all fit
bool build_host(const PTLightGridParams* p, const void* lights, uint32_t lightCount, uint32_t* offsets, uint32_t* indices, uint64_t indexCapacity,
                uint32_t* rectBefore, uint64_t* outTotal, std::string& err);

} // namespace ptlgrid
