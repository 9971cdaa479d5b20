// direct_rule.h — direct light at first hits (include/ptmi_plugin.h Part 24): the one definition of the rule -- an
// entry's constants, the pairs a light contributes, the light sample, the BRDF at the sampled direction, the weight, whether a
// pair counts, and the sum -- shared by the kernels (pt_direct.hip) and the host twins (direct_host.cpp).  Every fp32 operator is
// one IEEE binary32 operation in the order written, and both sides are compiled with -ffp-contract=off, so both give the same
// bits.  tests/direct_ref.py restates it from the header's text.  smith_g, the view vector, the flip and nDotV are shade_rule.h's.
#pragma once
#include "shade_rule.h"

#define PT_DIRECT_HD PT_SHADE_HD

namespace ptdirect {

constexpr float kPi = 3.14159265f;

// One light as the rule reads it: the PTLight record and rows 0 and 3 of derive_light_rows (pt_device.h) -- the kernels load
// them from the scene's derived rows, the host twins derive them from the record with the same expressions (derive_rows).
struct Light {
    float position[3]; uint32_t type;
    float emission[3]; float range;
    float u[3];        float area;
    float v[3];
    float N[3];         // rectangle: normalize(cross(u, v)); spot: normalize(u)
    float NN[3];        // normalize(N)
};

PT_DIRECT_HD float dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// v * (1 / sqrt(v . v)), the render's normalize
PT_DIRECT_HD void normalize(const float v[3], float o[3])
{
    const float s = 1.0f / pt_sqrt(dot(v, v));
    for (uint32_t a = 0; a < 3u; ++a) o[a] = v[a] * s;
}
PT_DIRECT_HD bool finite(float x) { return (pt_asuint(x) & 0x7F800000u) != 0x7F800000u; }

PT_DIRECT_HD void derive_rows(Light& l)
{
    for (uint32_t a = 0; a < 3u; ++a) l.N[a] = l.NN[a] = 0.0f;
    if (l.type == PT_LIGHT_TYPE_RECTANGLE) {
        const float c[3] = {l.u[1] * l.v[2] - l.u[2] * l.v[1], l.u[2] * l.v[0] - l.u[0] * l.v[2], l.u[0] * l.v[1] - l.u[1] * l.v[0]};
        normalize(c, l.N);
        normalize(l.N, l.NN);
    } else if (l.type == PT_LIGHT_TYPE_SPOT) {
        normalize(l.u, l.N);
        normalize(l.N, l.NN);
    }
}

// ---- step 4: pairs ----
PT_DIRECT_HD bool strata_ok(uint32_t strata) { return strata >= 1u && strata <= PT_DIRECT_MAX_STRATA; }
PT_DIRECT_HD uint32_t pairs_of(uint32_t type, uint32_t strata)
{
    if (type == PT_LIGHT_TYPE_POINT || type == PT_LIGHT_TYPE_SPOT) return 1u;
    if (type == PT_LIGHT_TYPE_RECTANGLE) return strata * strata;
    return 0u;
}

// the entry's RNG state (used without PT_DIRECT_CENTERED only)
PT_DIRECT_HD uint32_t entry_state(uint32_t seed, uint64_t i)
{
    uint32_t s = seed;
    pt_rng_next(&s);
    s += (uint32_t)i;
    return s;
}

// ---- step 3: what an entry keeps across its pairs ----
struct Entry {
    float O[3], N[3], Vd[3];
    float alpha, a2, nDotV;
    float diffuse[3], f0[3];
};

// D: the ray's direction; P, N: the receiver's (N already turned towards the viewer)
PT_DIRECT_HD void entry_begin(const PTShadeTerms& T, const float D[3], const float P[3], const float N[3], float minAlpha, Entry& e)
{
    ptshade::view_dot(D, N, e.Vd);
    float alpha = T.rho * T.rho;
    alpha = minAlpha > alpha ? minAlpha : alpha;
    e.alpha = alpha;
    e.a2 = alpha * alpha;
    e.nDotV = T.nDotV;
    for (uint32_t a = 0; a < 3u; ++a) {
        e.N[a] = N[a];
        const float b = N[a] * PT_EPSILON;
        e.O[a] = P[a] + b;
        e.diffuse[a] = T.diffuse[a];
        e.f0[a] = T.f0[a];
    }
}

// ---- step 5: the light sample at scatterPos = O (nee_prepare_light's SampleOneLight and EvalLight) ----
// false: a type that contributes no pair.  A point and a spot light share their expressions: -normalize(O - position) is the
// render's direction for both, and the length of position - O has the bits of the length of O - position.
PT_DIRECT_HD bool light_sample(const Light& l, const float O[3], float r1, float r2, float L[3], float& distance, float Li[3])
{
    const bool rect = l.type == PT_LIGHT_TYPE_RECTANGLE;
    if (!(rect || l.type == PT_LIGHT_TYPE_POINT || l.type == PT_LIGHT_TYPE_SPOT)) return false;
    float q[3];
#pragma unroll
    for (uint32_t a = 0; a < 3u; ++a) {
        const float p = (l.position[a] + l.u[a] * r1) + l.v[a] * r2;
        q[a] = rect ? p - O[a] : O[a] - l.position[a];
    }
    distance = pt_sqrt(dot(q, q));
    const float inv = 1.0f / distance;
#pragma unroll
    for (uint32_t a = 0; a < 3u; ++a) L[a] = rect ? q[a] / distance : -(q[a] * inv);
    // EvalLight
    float falloff = 0.0f;
    if (!(distance > l.range)) {
        const float r = distance / l.range;
        falloff = pt_saturate(1.0f / (1.0f + 25.0f * r * r) * pt_saturate((1.0f - r) * 5.0f));
    }
    if (l.type != PT_LIGHT_TYPE_POINT) {
        const float m[3] = {-L[0], -L[1], -L[2]};
        float mn[3];
        normalize(m, mn);
        const float cosTheta = dot(mn, l.NN);
        if (rect) {
            falloff = cosTheta < 0.0f ? 0.0f : falloff;
        } else {
            if (cosTheta < l.v[0]) falloff = 0.0f;
            else if (cosTheta > l.v[0] && cosTheta < l.v[1]) falloff = falloff * ((cosTheta - l.v[0]) / (l.v[1] - l.v[0]));
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) Li[c] = l.emission[c] * falloff;
    return true;
}

// ---- steps 5 to 7 for pair k of light l: the direction and the contribution; false: the pair does not count (L and c are then
// zero).  x1, x2: the pair's jitter (0.5f each when centred); read only for a rectangle light.
PT_DIRECT_HD bool pair_eval(const Entry& e, const Light& l, uint32_t strata, uint32_t k, float x1, float x2, float L[3], float c[3])
{
    for (uint32_t a = 0; a < 3u; ++a) L[a] = c[a] = 0.0f;
    const uint32_t sb = k / strata, sa = k - sb * strata;
    const float r1 = ((float)sa + x1) / (float)strata;
    const float r2 = ((float)sb + x2) / (float)strata;
    float sL[3], Li[3], distance;
    if (!light_sample(l, e.O, r1, r2, sL, distance, Li)) return false;
    // step 6
    const float nl = dot(e.N, sL);
    if (!(nl > 0.0f)) return false;
    float H[3] = {e.Vd[0] + sL[0], e.Vd[1] + sL[1], e.Vd[2] + sL[2]};
    const float len = pt_sqrt(dot(H, H));
    float sp = 0.0f, Fc = 0.0f;
    const bool lobe = len > 0.0f;
    if (lobe) {
        for (uint32_t a = 0; a < 3u; ++a) H[a] = H[a] / len;
        float nh = dot(e.N, H), vh = dot(e.Vd, H);
        nh = nh > 0.0f ? nh : 0.0f;
        vh = vh > 0.0f ? vh : 0.0f;
        const float t = (nh * nh) * (e.a2 - 1.0f) + 1.0f;
        const float D = e.a2 / ((kPi * t) * t);
        const float G = ptshade::smith_g(e.nDotV, e.alpha) * ptshade::smith_g(nl, e.alpha);
        const float m = 1.0f - vh;
        Fc = ((m * m) * (m * m)) * m;
        sp = (D * G) / ((4.0f * nl) * e.nDotV);
    }
    // step 7
    float w = 1.0f;
    if (l.type == PT_LIGHT_TYPE_RECTANGLE)
        w = ((l.area * pt_abs(dot(l.N, sL))) / (distance * distance)) / (float)(strata * strata);
    float v[3];
    bool allFinite = true, anyPositive = false;
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        float f = e.diffuse[ch] * ptshade::kInvPi;
        if (lobe) {
            const float F = e.f0[ch] + (1.0f - e.f0[ch]) * Fc;
            f = f + F * sp;
        }
        v[ch] = ((Li[ch] * f) * nl) * w;
        allFinite = allFinite && finite(v[ch]);
        anyPositive = anyPositive || v[ch] > 0.0f;
    }
    if (!(allFinite && anyPositive)) return false;
    for (uint32_t a = 0; a < 3u; ++a) { L[a] = sL[a]; c[a] = v[a]; }
    return true;
}

// ---- the host twins and the checks the entry points share (direct_host.cpp); false: err says why ----
bool check_params(const PTDirectParams* p, std::string& err);
bool pair_count_host(const void* lights, uint32_t lightCount, uint32_t strata, uint32_t* outPairsPerEntry, std::string& err);
bool rays_host(const PTDirectParams* p, const void* lights, uint32_t lightCount, const PTRay* rays, const PTShadeTerms* terms, const PTReceiver* receivers,
               uint64_t count, PTRay* outRays, float* outContrib, std::string& err);
bool accumulate_host(const PTShadeTerms* terms, const float* contrib, const PTRayHit* pairHits, uint64_t count, uint32_t pairsPerEntry, float* out,
                     std::string& err);

} // namespace ptdirect
