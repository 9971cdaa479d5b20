// chart_rule.h — lightmap charts (include/ptmi_plugin.h Part 14): the one definition of the rasterisation rule and
// of the resolve's dilation step, shared by the host twin (chart_host.cpp) and the kernels (pt_lightmap.hip).  Coverage is decided
// in integers; every fp32 operator is one IEEE binary32 operation, left to right, and both sides are compiled with
// -ffp-contract=off, so both give the same bytes.  tests/chart_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string>
#include "ptmi_layouts.h"
#include "ptmi_math.h"
#include "ptmi_plugin.h"

#if defined(__HIPCC__)
#define PT_CHART_HD __host__ __device__ __forceinline__
#else
#define PT_CHART_HD inline
#endif

namespace ptchart {

constexpr uint32_t kNoOwner = 0xFFFFFFFFu;         // an owner word no primitive has claimed
constexpr int32_t kSubTexel = 256;                 // 8 sub-texel bits
constexpr int32_t kHalfTexel = 128;                // a texel is sampled at its centre

// A UV triangle snapped to the sub-texel grid.  Every coordinate is within +-2^23, so every difference of two coordinates, and of
// a sample and a coordinate, fits 32 bits; a product of two fits 49 bits; an edge value 50.
struct Snapped {
    int32_t X[3], Y[3];
    int64_t A;              // E(p0, p1; p2), never 0
};

PT_CHART_HD bool chart_finite(float v) { return pt_abs(v) <= 3.402823466e38f; }

// One coordinate: one fp32 multiply, round half even.  false: not finite, or beyond 2^23 (from there on every float is an integer,
// so |rint(s)| > 2^23 exactly when |s| > 2^23)
PT_CHART_HD bool chart_snap(float u, uint32_t size, int32_t& out)
{
    const float s = u * (float)(size * 256u);
    if (!(pt_abs(s) <= 8388608.0f)) return false;
    out = (int32_t)pt_rint(s);
    return true;
}

// E(a, b; s) = (b.X - a.X) * (s.Y - a.Y) - (b.Y - a.Y) * (s.X - a.X), exact
PT_CHART_HD int64_t chart_edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t sx, int32_t sy)
{
    return (int64_t)(bx - ax) * (int64_t)(sy - ay) - (int64_t)(by - ay) * (int64_t)(sx - ax);
}

// uv: u0 v0 u1 v1 u2 v2.  false: the triangle is not in the chart (a UV that does not snap, or no area)
PT_CHART_HD bool chart_setup(const float uv[6], uint32_t width, uint32_t height, Snapped& s)
{
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        ok = chart_snap(uv[2 * k], width, s.X[k]) && ok;
        ok = chart_snap(uv[2 * k + 1], height, s.Y[k]) && ok;
    }
    if (!ok) return false;
    s.A = chart_edge(s.X[0], s.Y[0], s.X[1], s.Y[1], s.X[2], s.Y[2]);
    return s.A != 0;
}

// cross(e1, e2) as cross3 writes it, and its squared length as dot3 does; false: the triangle has no area in space (or not a finite one)
PT_CHART_HD bool chart_geometric_normal(const float e1[3], const float e2[3], float c[3])
{
    c[0] = e1[1] * e2[2] - e1[2] * e2[1];
    c[1] = e1[2] * e2[0] - e1[0] * e2[2];
    c[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const float d = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    return d != 0.0f && chart_finite(d);
}

// The three edge values at the sample (sx, sy) as E gives them: w[k] / A is the weight of corner k.
PT_CHART_HD void chart_edges(const Snapped& s, int32_t sx, int32_t sy, int64_t w[3])
{
    w[0] = chart_edge(s.X[1], s.Y[1], s.X[2], s.Y[2], sx, sy);
    w[1] = chart_edge(s.X[2], s.Y[2], s.X[0], s.Y[0], sx, sy);
    w[2] = chart_edge(s.X[0], s.Y[0], s.X[1], s.Y[1], sx, sy);
}

// texel (x, y) is covered: all three signed edge values >= 0 at its centre
PT_CHART_HD bool chart_covers(const Snapped& s, uint32_t x, uint32_t y)
{
    int64_t w[3];
    chart_edges(s, (int32_t)x * kSubTexel + kHalfTexel, (int32_t)y * kSubTexel + kHalfTexel, w);
    if (s.A < 0) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; }     // a mirrored chart: the sign of A flips all three
    return (w[0] | w[1] | w[2]) >= 0;
}

// floor(a / 256) for a negative a too
PT_CHART_HD int32_t chart_floor256(int32_t a) { return a >> 8; }

// The texels whose centres lie in the snapped bounding box, clipped to the image: x0 <= x <= x1, y0 <= y <= y1; false: none
PT_CHART_HD bool chart_bounds(const Snapped& s, uint32_t width, uint32_t height, int32_t& x0, int32_t& y0, int32_t& x1, int32_t& y1)
{
    int32_t mnx = s.X[0], mxx = s.X[0], mny = s.Y[0], mxy = s.Y[0];
    for (int k = 1; k < 3; ++k) {
        mnx = s.X[k] < mnx ? s.X[k] : mnx; mxx = s.X[k] > mxx ? s.X[k] : mxx;
        mny = s.Y[k] < mny ? s.Y[k] : mny; mxy = s.Y[k] > mxy ? s.Y[k] : mxy;
    }
    // 256 x + 128 >= mn  <=>  x >= ceil((mn - 128) / 256);  256 x + 128 <= mx  <=>  x <= floor((mx - 128) / 256)
    x0 = chart_floor256(mnx - kHalfTexel + kSubTexel - 1); x1 = chart_floor256(mxx - kHalfTexel);
    y0 = chart_floor256(mny - kHalfTexel + kSubTexel - 1); y1 = chart_floor256(mxy - kHalfTexel);
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > (int32_t)width - 1) x1 = (int32_t)width - 1;
    if (y1 > (int32_t)height - 1) y1 = (int32_t)height - 1;
    return x0 <= x1 && y0 <= y1;
}

// normalize3 of pt_device.h: v * (1 / sqrt(dot3(v, v)))
PT_CHART_HD void chart_normalize(float v[3])
{
    const float s = 1.0f / pt_sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] = v[0] * s; v[1] = v[1] * s; v[2] = v[2] * s;
}

// What fetch_hit_attributes_tlas does to the hit's normal: the worldToLocal product (row vector times matrix) and the second
// normalize3, expression for expression.  w2l: the instance's 16 floats, or null (the normal is used as it is).
PT_CHART_HD void chart_instance_normal(const float* w2l, float n[3])
{
    if (!w2l) return;
    float t[3];
    for (int r = 0; r < 3; ++r) t[r] = ((n[0] * w2l[4 * r] + n[1] * w2l[4 * r + 1]) + n[2] * w2l[4 * r + 2]) + 0.0f * w2l[4 * r + 3];
    n[0] = t[0]; n[1] = t[1]; n[2] = t[2];
    chart_normalize(n);
}

// The receiver of texel (x, y) on the primitive that owns it.  v0, e1, e2: the triangle record; n0, n1, n2: the attribute
// record's normals; l2w, w2l: the instance's matrices (element (r, c) at c * 4 + r) or both null.
PT_CHART_HD void chart_receiver(const Snapped& s, uint32_t x, uint32_t y, const float v0[3], const float e1[3], const float e2[3], const float n0[3],
                                const float n1[3], const float n2[3], const float* l2w, const float* w2l, uint32_t seed, PTReceiver& out)
{
    int64_t w[3];
    chart_edges(s, (int32_t)x * kSubTexel + kHalfTexel, (int32_t)y * kSubTexel + kHalfTexel, w);
    // int64 -> double is exact here (50 bits); the divide and the narrowing are each correctly rounded
    const float b1 = (float)((double)w[1] / (double)s.A);
    const float b2 = (float)((double)w[2] / (double)s.A);
    float p[3], n[3];
    for (int a = 0; a < 3; ++a) p[a] = (v0[a] + e1[a] * b1) + e2[a] * b2;
    const float b0 = 1.0f - b1 - b2;                               // interp3
    for (int a = 0; a < 3; ++a) n[a] = (n0[a] * b0 + n1[a] * b1) + n2[a] * b2;
    chart_normalize(n);
    chart_instance_normal(w2l, n);
    if (!(chart_finite(n[0]) && chart_finite(n[1]) && chart_finite(n[2]))) {
        (void)chart_geometric_normal(e1, e2, n);
        chart_normalize(n);
        chart_instance_normal(w2l, n);
    }
    if (l2w) {
        float q[3];
        for (int r = 0; r < 3; ++r) q[r] = ((l2w[r] * p[0] + l2w[4 + r] * p[1]) + l2w[8 + r] * p[2]) + l2w[12 + r];
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
    out.position[0] = p[0]; out.position[1] = p[1]; out.position[2] = p[2];
    out.seed = seed;
    out.normal[0] = n[0]; out.normal[1] = n[1]; out.normal[2] = n[2];
    out.reserved = 0u;
}

// One texel of one dilation pass.  nb: the rgba of the 8 neighbours in the order (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0)
// (1,1) of (dy, dx); inside: bit k set when neighbour k lies in the image.
PT_CHART_HD void chart_dilate(const float self[4], const float nb[8][4], uint32_t inside, float out[4])
{
    if (self[3] != 0.0f) { out[0] = self[0]; out[1] = self[1]; out[2] = self[2]; out[3] = self[3]; return; }
    float acc[3] = {0.0f, 0.0f, 0.0f};
    uint32_t n = 0;
    for (int k = 0; k < 8; ++k)
        if ((inside >> k & 1u) && nb[k][3] != 0.0f) {
            acc[0] = acc[0] + nb[k][0]; acc[1] = acc[1] + nb[k][1]; acc[2] = acc[2] + nb[k][2];
            ++n;
        }
    if (n == 0) { out[0] = out[1] = out[2] = out[3] = 0.0f; return; }
    const float d = (float)n;
    out[0] = acc[0] / d; out[1] = acc[1] / d; out[2] = acc[2] / d; out[3] = 0.5f;
}

// ---- host side (chart_host.cpp) ----
// tris: the BLAS's 3 * triangleCount rows (e2, e1, v0 + primIdx per record); attrs: its triangleCount records, indexed by primIdx;
// uvs: 6 floats per primitive or null (the records' uv0 .. uv2); l2w / w2l: both null, or 16 floats each.
struct ChartInput {
    const PTFloat4* tris;
    const PTTriangleAttributes* attrs;
    const float* uvs;
    const float* l2w;
    const float* w2l;
    uint32_t triCount, width, height, seedBase;
};
// The rule on the host.  texels / recv both null: only the count.  false: err has the reason; a count above the capacity is one
// (count is set, nothing is written).
bool chart_rasterize_host(const ChartInput& in, uint32_t* texels, PTReceiver* recv, uint64_t capacity, uint64_t& count, std::string& err);
// Scatter and dilate on the host; image: width * height RGBA.  false: an index >= width * height, or dilate > kMaxDilate.
constexpr uint32_t kMaxDilate = 16u;
constexpr uint32_t kMaxSize = 8192u;
bool chart_resolve_host(const uint32_t* texels, const PTIrradiance* irr, uint64_t count, uint32_t width, uint32_t height, uint32_t dilate, float* image,
                        std::string& err);

} // namespace ptchart
