// shade_rule.h — shading from the bakes (include/ptmi_plugin.h Part 21): the one definition of the rule -- the
// split-sum DFG table's quadrature, the terms a hit gives (view vector, face-forwarded normal, reflection direction, diffuse and
// specular colour), the choice of a reflection probe, the table lookup and the compose step -- shared by the kernels
// (pt_shade_baked.hip) and the host twins (shade_host.cpp).  Every fp32 operator is one IEEE binary32 operation in the order
// written, and both sides are compiled with -ffp-contract=off, so both give the same bits.  tests/shade_ref.py restates it.  The
// fold tree is sh_rule.h's, the lookups are volume_rule.h's and reflection_rule.h's.
#pragma once
#include "reflection_rule.h"

#define PT_SHADE_HD PT_SH_HD

namespace ptshade {

constexpr uint32_t kSamples = 64u;          // radial samples per lane, and lanes (azimuths)
constexpr uint32_t kNoProbe = 0xFFFFFFFFu;
constexpr float kInvPi = 0.31830988618379067f;

PT_SHADE_HD bool dfg_res_ok(uint32_t res) { return res == 16u || res == 32u || res == 64u; }

// cos and sin of 2 pi (q + 0.5) / 64, rounded from float64 (tests/test_shade_baked.py checks every literal)
PT_SHADE_HD float azimuth_cos(uint32_t q)
{
    const float C[64] = {
        0.99879545f, 0.9891765f, 0.97003126f, 0.94154406f, 0.9039893f, 0.8577286f, 0.8032075f, 0.7409511f,
        0.671559f, 0.5956993f, 0.51410276f, 0.42755508f, 0.33688986f, 0.24298018f, 0.14673047f, 0.049067676f,
        -0.049067676f, -0.14673047f, -0.24298018f, -0.33688986f, -0.42755508f, -0.51410276f, -0.5956993f, -0.671559f,
        -0.7409511f, -0.8032075f, -0.8577286f, -0.9039893f, -0.94154406f, -0.97003126f, -0.9891765f, -0.99879545f,
        -0.99879545f, -0.9891765f, -0.97003126f, -0.94154406f, -0.9039893f, -0.8577286f, -0.8032075f, -0.7409511f,
        -0.671559f, -0.5956993f, -0.51410276f, -0.42755508f, -0.33688986f, -0.24298018f, -0.14673047f, -0.049067676f,
        0.049067676f, 0.14673047f, 0.24298018f, 0.33688986f, 0.42755508f, 0.51410276f, 0.5956993f, 0.671559f,
        0.7409511f, 0.8032075f, 0.8577286f, 0.9039893f, 0.94154406f, 0.97003126f, 0.9891765f, 0.99879545f,
    };
    return C[q];
}
PT_SHADE_HD float azimuth_sin(uint32_t q)
{
    const float S[64] = {
        0.049067676f, 0.14673047f, 0.24298018f, 0.33688986f, 0.42755508f, 0.51410276f, 0.5956993f, 0.671559f,
        0.7409511f, 0.8032075f, 0.8577286f, 0.9039893f, 0.94154406f, 0.97003126f, 0.9891765f, 0.99879545f,
        0.99879545f, 0.9891765f, 0.97003126f, 0.94154406f, 0.9039893f, 0.8577286f, 0.8032075f, 0.7409511f,
        0.671559f, 0.5956993f, 0.51410276f, 0.42755508f, 0.33688986f, 0.24298018f, 0.14673047f, 0.049067676f,
        -0.049067676f, -0.14673047f, -0.24298018f, -0.33688986f, -0.42755508f, -0.51410276f, -0.5956993f, -0.671559f,
        -0.7409511f, -0.8032075f, -0.8577286f, -0.9039893f, -0.94154406f, -0.97003126f, -0.9891765f, -0.99879545f,
        -0.99879545f, -0.9891765f, -0.97003126f, -0.94154406f, -0.9039893f, -0.8577286f, -0.8032075f, -0.7409511f,
        -0.671559f, -0.5956993f, -0.51410276f, -0.42755508f, -0.33688986f, -0.24298018f, -0.14673047f, -0.049067676f,
    };
    return S[q];
}

// ---- the DFG table ----
// the arithmetic of smith_g in pt_device.h, which the render's smith_g_aniso reduces to at anisotropic 0
PT_SHADE_HD float smith_g(float c, float alpha)
{
    const float a = alpha * alpha;
    const float b = c * c;
    return (2.0f * c) / (c + pt_sqrt((a + b) - a * b));
}

// lane q's partial sums of entry (i, j): its 64 radial samples in ascending p
PT_SHADE_HD void dfg_lane(uint32_t res, uint32_t i, uint32_t j, uint32_t q, float& a, float& b)
{
    const float mu = ((float)i + 0.5f) / (float)res;
    const float rho = ((float)j + 0.5f) / (float)res;
    const float alpha = rho * rho;
    const float a2 = alpha * alpha;
    const float Vx = pt_sqrt(1.0f - mu * mu), Vz = mu;
    const float gV = smith_g(mu, alpha);
    const float Cq = azimuth_cos(q);
    a = 0.0f;
    b = 0.0f;
    for (uint32_t p = 0; p < kSamples; ++p) {
        const float xi = ((float)p + 0.5f) / 64.0f;
        const float c2 = (1.0f - xi) / (1.0f + (a2 - 1.0f) * xi);
        const float Hx = pt_sqrt(1.0f - c2) * Cq;               // H.y = sqrt(1 - c2) * S[q] meets V.y = 0
        const float Hz = pt_sqrt(c2);
        const float vh = Vx * Hx + Vz * Hz;
        const float nl = (2.0f * vh) * Hz - Vz;
        if (!(nl > 0.0f && vh > 0.0f)) continue;
        const float G = gV * smith_g(nl, alpha);
        const float gv = (G * vh) / (Hz * mu);
        const float m = 1.0f - vh;
        const float m2 = m * m;
        const float Fc = (m2 * m2) * m;
        a = a + (1.0f - Fc) * gv;
        b = b + Fc * gv;
    }
}

PT_SHADE_HD float dfg_scale(float folded) { return folded / 4096.0f; }

// ---- terms ----
// What a hit gives, after the material fetch.  N: the surface record's normal in, the face-forwarded one out; R: the reflection
// direction.  The record's words that no rule names are zero.
// The view vector Vd = (-D) / len and d = N . Vd of the normal as the surface record gives it, before any flip: d < 0 is a hit seen
// from behind (Part 22's side rule reads it here too).
PT_SHADE_HD float view_dot(const float D[3], const float N[3], float Vd[3])
{
    const float len = pt_sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
    for (uint32_t a = 0; a < 3u; ++a) Vd[a] = (-D[a]) / len;
    return (N[0] * Vd[0] + N[1] * Vd[1]) + N[2] * Vd[2];
}

PT_SHADE_HD void terms(const PTShadeMaterial& M, const float D[3], float N[3], float R[3], PTShadeTerms& T)
{
    float Vd[3];
    float d = view_dot(D, N, Vd);
    if (d < 0.0f) {
        for (uint32_t a = 0; a < 3u; ++a) N[a] = -N[a];
        d = (N[0] * Vd[0] + N[1] * Vd[1]) + N[2] * Vd[2];
    }
    const float t = 2.0f * d;
    for (uint32_t a = 0; a < 3u; ++a) R[a] = t * N[a] - Vd[a];
    const float k = 1.0f - M.metallic;
    for (uint32_t c = 0; c < 3u; ++c) {
        T.diffuse[c] = M.baseColor[c] * k;
        T.f0[c] = 0.04f + M.metallic * (M.baseColor[c] - 0.04f);
        T.emission[c] = M.emission[c];
    }
    T.rho = pt_sqrt(M.roughness);
    T.nDotV = pt_max(d, 1e-4f);
    T.occlusion = M.occlusion;
}

// loadProbe(k, float Q[3]); loadBox(k, float bmin[3], float bmax[3]), called only with boxes
template <class LoadProbe, class LoadBox>
PT_SHADE_HD uint32_t choose_probe(const float P[3], uint32_t probeCount, bool boxes, LoadProbe loadProbe, LoadBox loadBox)
{
    uint32_t best = kNoProbe;
    float bestD = 0.0f;
    for (uint32_t pass = boxes ? 0u : 1u; pass < 2u && best == kNoProbe; ++pass)
        for (uint32_t k = 0; k < probeCount; ++k) {
            if (pass == 0u) {
                float bmin[3], bmax[3];
                loadBox(k, bmin, bmax);
                if (!((bmin[0] <= P[0] && P[0] <= bmax[0]) && (bmin[1] <= P[1] && P[1] <= bmax[1]) && (bmin[2] <= P[2] && P[2] <= bmax[2]))) continue;
            }
            float Q[3];
            loadProbe(k, Q);
            const float v[3] = {P[0] - Q[0], P[1] - Q[1], P[2] - Q[2]};
            const float d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
            if (best == kNoProbe || d2 < bestD) {
                best = k;
                bestD = d2;
            }
        }
    return best;
}

PT_SHADE_HD bool is_miss(const PTShadeTerms& T) { return !(T.nDotV > 0.0f); }

// ---- compose ----
// [0, 1] -> the lower entry and the fraction on one table axis
PT_SHADE_HD void table_coord(float v, uint32_t res, uint32_t& x0, float& fx)
{
    float x = v * (float)res - 0.5f;
    x = x > 0.0f ? x : 0.0f;                                    // a NaN lands on 0
    x = x < (float)(res - 1u) ? x : (float)(res - 1u);
    const uint32_t i = (uint32_t)x;
    x0 = i < res - 2u ? i : res - 2u;
    fx = x - (float)x0;
}

// load(entry index, float ab[2])
template <class Load>
PT_SHADE_HD void dfg_lookup(uint32_t res, float nDotV, float rho, Load load, float& A, float& B)
{
    uint32_t x0, y0;
    float fx, fy;
    table_coord(nDotV, res, x0, fx);
    table_coord(rho, res, y0, fy);
    float e[4][2];
    load(y0 * res + x0, e[0]);
    load(y0 * res + x0 + 1u, e[1]);
    load((y0 + 1u) * res + x0, e[2]);
    load((y0 + 1u) * res + x0 + 1u, e[3]);
    A = ptrefl::lerp(ptrefl::lerp(e[0][0], e[1][0], fx), ptrefl::lerp(e[2][0], e[3][0], fx), fy);
    B = ptrefl::lerp(ptrefl::lerp(e[0][1], e[1][1], fx), ptrefl::lerp(e[2][1], e[3][1], fx), fy);
}

// E: the irradiance, spec: the prefiltered radiance; the terms are a hit's
PT_SHADE_HD void compose(const PTShadeTerms& T, const float E[3], const float spec[3], float A, float B, float out[4])
{
    for (uint32_t c = 0; c < 3u; ++c) {
        const float d = (T.diffuse[c] * E[c]) * kInvPi;
        const float s = spec[c] * (T.f0[c] * A + B);
        out[c] = T.emission[c] + T.occlusion * (d + s);
    }
    out[3] = 1.0f;
}

// ---- the host twins and the checks the entry points share (shade_host.cpp); false: err says why ----
bool check_dfg_res(uint32_t res, std::string& err);
bool bake_dfg_host(uint32_t res, PTShadeDFG* out, std::string& err);
bool terms_host(const PTShadeMaterial* materials, const PTRay* rays, const PTRaySurface* surface, uint64_t count, const PTProbe* probes,
                const PTReflectionBox* boxes, uint32_t probeCount, PTShadeTerms* outTerms, PTReceiver* outReceivers, PTReflectionQuery* outQueries,
                std::string& err);
bool compose_host(const PTShadeTerms* terms, const PTIrradiance* irradiance, const PTReflectionTexel* reflection, uint64_t count, const PTShadeDFG* dfg,
                  uint32_t dfgRes, float* out, std::string& err);

} // namespace ptshade
