// reflection_rule.h — reflection probes (include/ptmi_plugin.h Part 20): the one definition of the rule -- the
// octahedral texel directions at any resolution, the capture's seeding and fold, the GGX prefilter's weight and the trilinear
// lookup with its wrap and box projection -- shared by the kernels (pt_reflection.hip) and the host twins (reflection_host.cpp).
// Every fp32 operator is one IEEE binary32 operation in the order written, and both sides are compiled with -ffp-contract=off, so
// both give the same bits.  tests/reflection_ref.py restates it.  sgn and the RNG are volume_rule.h's and ptmi_math.h's.
#pragma once
#include "volume_rule.h"

#define PT_REFL_HD PT_SH_HD

namespace ptrefl {

using ptvol::sgn;

constexpr uint32_t kMinRes = 8u, kMaxRes = 256u;
constexpr uint64_t kSlabSlots = 1ull << 22;         // PTReflectionCapture: a slab holds floor(2^22 / samples) whole texels

PT_REFL_HD uint32_t log2_res(uint32_t res)
{
    uint32_t l = 0;
    while ((1u << l) < res) ++l;
    return l;
}

// texels before level k of one probe's map, and of the whole map (k = levels)
PT_REFL_HD uint32_t level_offset(uint32_t res, uint32_t k)
{
    uint32_t o = 0;
    for (uint32_t j = 0; j < k; ++j) o += (res >> j) * (res >> j);
    return o;
}

PT_REFL_HD float level_roughness(uint32_t k, uint32_t levels) { return (float)k / (float)(levels - 1u); }

// the direction of the point (u + su, v + sv) of an R x R map; a centre has su = sv = 0.5f.  len: the length before the division
PT_REFL_HD void direction(uint32_t R, uint32_t u, uint32_t v, float su, float sv, float d[3], float& len)
{
    const float a = (((float)u + su) / (float)R) * 2.0f - 1.0f;
    const float b = (((float)v + sv) / (float)R) * 2.0f - 1.0f;
    const float z = (1.0f - pt_abs(a)) - pt_abs(b);
    float x = a, y = b;
    if (z < 0.0f) {
        x = (1.0f - pt_abs(b)) * sgn(a);
        y = (1.0f - pt_abs(a)) * sgn(b);
    }
    len = pt_sqrt((x * x + y * y) + z * z);
    d[0] = x / len;
    d[1] = y / len;
    d[2] = z / len;
}

// the map coordinates (a, b) in [-1, 1]^2 of a direction, which need not be of unit length
PT_REFL_HD void oct_coords(const float D[3], float& a, float& b)
{
    const float s = (pt_abs(D[0]) + pt_abs(D[1])) + pt_abs(D[2]);
    a = D[0] / s;
    b = D[1] / s;
    if (D[2] < 0.0f) {
        const float a2 = (1.0f - pt_abs(b)) * sgn(a);
        const float b2 = (1.0f - pt_abs(a)) * sgn(b);
        a = a2;
        b = b2;
    }
}

// ---- capture ----
// the RNG state sample j (counted from firstSample) of texel t of a probe starts with
PT_REFL_HD uint32_t sample_rng(uint32_t seed, uint32_t t, uint32_t firstSample, uint32_t j)
{
    uint32_t s = seed;
    pt_rng_next(&s);
    s += t;
    pt_rng_next(&s);
    return s + (firstSample + j);
}

// two draws -> a direction inside texel (u, v); rng is left as the path starts with it
PT_REFL_HD void sample_direction(uint32_t R, uint32_t u, uint32_t v, uint32_t& rng, float d[3])
{
    const float r1 = pt_random_float(&rng);
    const float r2 = pt_random_float(&rng);
    float len;
    direction(R, u, v, r1, r2, d, len);
}

// one sample into a texel's four sums
PT_REFL_HD void fold_step(float acc[4], const float L[3])
{
    for (uint32_t c = 0; c < 3u; ++c) acc[c] = acc[c] + L[c];
    const float lum = ptsh::luminance(L);
    acc[3] = acc[3] + lum * lum;
}

// ---- prefilter ----
// g = a2 - 1 of level k
PT_REFL_HD float lobe_g(uint32_t k, uint32_t levels)
{
    const float rho = level_roughness(k, levels);
    const float alpha = rho * rho;
    const float a2 = alpha * alpha;
    return a2 - 1.0f;
}

// base texel s of an R x R map: its centre direction and the solid-angle Jacobian 1 / len^3
PT_REFL_HD void source(uint32_t R, uint32_t s, float l[3], float& J)
{
    float len;
    direction(R, s % R, s / R, 0.5f, 0.5f, l, len);
    J = 1.0f / ((len * len) * len);
}

// false: the source lies behind n and is skipped
PT_REFL_HD bool weight(const float n[3], const float l[3], float J, float g, float& w)
{
    const float c = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
    if (!(c > 0.0f)) return false;
    const float h = (1.0f + c) * 0.5f;
    const float t = h * g + 1.0f;
    w = (c * J) / (t * t);
    return true;
}

// ---- lookup ----
// the direction a box-projected query reads: P the query's position, Q the probe's
PT_REFL_HD void box_project(const float bmin[3], const float bmax[3], const float P[3], const float Q[3], float D[3])
{
    for (uint32_t a = 0; a < 3u; ++a)
        if (!(bmin[a] <= P[a] && P[a] <= bmax[a])) return;
    float t = __builtin_huge_valf();
    for (uint32_t a = 0; a < 3u; ++a) {
        if (D[a] > 0.0f) t = pt_min(t, (bmax[a] - P[a]) / D[a]);
        else if (D[a] < 0.0f) t = pt_min(t, (bmin[a] - P[a]) / D[a]);
    }
    if (!(t > 0.0f && t < __builtin_huge_valf())) return;
    float v[3];
    for (uint32_t a = 0; a < 3u; ++a) v[a] = (P[a] + D[a] * t) - Q[a];
    const float r = pt_sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(r > 0.0f)) return;
    for (uint32_t a = 0; a < 3u; ++a) D[a] = v[a] / r;
}

// the two levels a roughness blends and the fraction between them
PT_REFL_HD void select_levels(float roughness, uint32_t levels, uint32_t& k0, float& f)
{
    float r = roughness > 0.0f ? roughness : 0.0f;             // a NaN lands on 0
    r = r < 1.0f ? r : 1.0f;
    const float lam = r * (float)(levels - 1u);
    const uint32_t k = (uint32_t)lam;
    k0 = k < levels - 2u ? k : levels - 2u;
    f = lam - (float)k0;
}

// a tap outside the map comes back in across the edge it left through
PT_REFL_HD void wrap(int32_t Rk, int32_t& x, int32_t& y)
{
    if (x < 0 || x >= Rk) {
        x = x < 0 ? -1 - x : 2 * Rk - 1 - x;
        y = Rk - 1 - y;
    }
    if (y < 0 || y >= Rk) {
        y = y < 0 ? -1 - y : 2 * Rk - 1 - y;
        x = Rk - 1 - x;
    }
}

// [-1, 1] -> the lower tap and the fraction on one axis.  floor(x) lies in [-1, Rk - 1] for every a in [-1, 1]; a coordinate that
// is not (a NaN direction) is held to that range, so that no tap leaves the map, and its fraction is whatever x - x0 gives
PT_REFL_HD void tap_coord(float a, uint32_t Rk, int32_t& x0, float& fx)
{
    const float x = (a * 0.5f + 0.5f) * (float)Rk - 0.5f;
    float fl = pt_floor(x);
    fl = fl >= -1.0f ? fl : -1.0f;
    fl = fl < (float)Rk - 1.0f ? fl : (float)Rk - 1.0f;
    x0 = (int32_t)fl;
    fx = x - fl;
}

PT_REFL_HD float lerp(float p, float q, float f) { return p + f * (q - p); }

// bilinear in one level: load(texel index within the level, float rgb[3])
template <class Load>
PT_REFL_HD void bilinear(uint32_t Rk, float a, float b, Load load, float out[3])
{
    int32_t x0, y0;
    float fx, fy;
    tap_coord(a, Rk, x0, fx);
    tap_coord(b, Rk, y0, fy);
    float tap[4][3];
    for (int32_t dy = 0; dy < 2; ++dy)
        for (int32_t dx = 0; dx < 2; ++dx) {
            int32_t x = x0 + dx, y = y0 + dy;
            wrap((int32_t)Rk, x, y);
            load((uint32_t)y * Rk + (uint32_t)x, tap[dy * 2 + dx]);
        }
    for (uint32_t c = 0; c < 3u; ++c) out[c] = lerp(lerp(tap[0][c], tap[1][c], fx), lerp(tap[2][c], tap[3][c], fx), fy);
}

// One query, whole, after the probe index was found in range.  load(texel index within the probe's map, float rgb[3]);
// Q, bmin, bmax: the probe's position and box, or null without box projection
template <class Load>
PT_REFL_HD void lookup(uint32_t res, uint32_t levels, const float P[3], float roughness, const float dir[3], const float* Q, const float* bmin,
                       const float* bmax, Load load, float out[4])
{
    float D[3] = {dir[0], dir[1], dir[2]};
    if (bmin) box_project(bmin, bmax, P, Q, D);
    float a, b;
    oct_coords(D, a, b);
    uint32_t k0;
    float f;
    select_levels(roughness, levels, k0, f);
    float A[3], B[3];
    const uint32_t o0 = level_offset(res, k0), o1 = o0 + (res >> k0) * (res >> k0);
    bilinear(res >> k0, a, b, [&](uint32_t t, float rgb[3]) { load(o0 + t, rgb); }, A);
    bilinear(res >> (k0 + 1u), a, b, [&](uint32_t t, float rgb[3]) { load(o1 + t, rgb); }, B);
    for (uint32_t c = 0; c < 3u; ++c) out[c] = lerp(A[c], B[c], f);
    out[3] = 1.0f;
}

// ---- the host twins and the checks the entry points share (reflection_host.cpp); false: err says why ----
bool check_layout(uint32_t res, uint32_t levels, bool needLevels, std::string& err);
bool check_samples(uint32_t samples, std::string& err);
bool directions_host(const PTProbe* probes, uint64_t count, uint32_t res, uint32_t firstSample, uint32_t samples, PTRadianceRay* rays, std::string& err);
bool fold_host(const PTRadiance* radiance, uint64_t count, uint32_t res, uint32_t samples, PTReflectionTexel* out, std::string& err);
bool prefilter_host(const PTReflectionTexel* base, uint64_t count, uint32_t res, uint32_t levels, PTReflectionTexel* out, std::string& err);
bool lookup_host(const PTReflectionTexel* maps, uint64_t probeCount, uint32_t res, uint32_t levels, const PTProbe* probes, const PTReflectionBox* boxes,
                 const PTReflectionQuery* queries, uint64_t count, PTReflectionTexel* out, std::string& err);

} // namespace ptrefl
