// sh_rule.h — SH light probes (include/ptmi_plugin.h Part 15): the one definition of the probe rule -- seeding,
// sphere direction, basis, a lane's accumulation step, the fold tree, the scaling, the delta-light add and the evaluation -- shared
// by the kernels (pt_probe.hip) and the host twins (probe_host.cpp).  Every fp32 operator is one IEEE binary32 operation in the
// order written, and both sides are compiled with -ffp-contract=off, so both give the same bits.  tests/probe_ref.py restates it.
#pragma once
#include <stdint.h>
#include <string>
#include "ptmi_layouts.h"
#include "ptmi_math.h"
#include "ptmi_plugin.h"

#if defined(__HIPCC__)
#define PT_SH_HD __host__ __device__ __forceinline__
#else
#define PT_SH_HD inline
#endif

namespace ptsh {

constexpr uint32_t kLanes = 64u;            // partial sums per probe: lane l owns the samples j = l (mod 64)
constexpr uint32_t kCoeffs = 9u;            // bands 0, 1, 2
constexpr uint32_t kSums = 28u;             // 9 x 3 coefficient sums, then the luminance moment
constexpr float kFourPi = 12.566371f;       // 1 / pdf of a uniform direction

// the RNG state sample j of a probe starts with (Part 13's seeding)
PT_SH_HD uint32_t sample_rng(uint32_t seed, uint32_t firstSample, uint32_t j)
{
    uint32_t s = seed;
    pt_rng_next(&s);
    return s + (firstSample + j);
}

// two draws -> a uniform direction on the sphere; rng is left as the path starts with it
PT_SH_HD void direction(uint32_t& rng, float w[3])
{
    const float r1 = pt_random_float(&rng);
    const float r2 = pt_random_float(&rng);
    const float z = 1.0f - 2.0f * r1;
    const float rho = pt_sqrt(pt_max(1.0f - z * z, 0.0f));
    const float phi = PT_TWO_PI * r2;
    w[0] = rho * pt_cos(phi);
    w[1] = rho * pt_sin(phi);
    w[2] = z;
}

PT_SH_HD void basis(const float w[3], float Y[9])
{
    const float x = w[0], y = w[1], z = w[2];
    Y[0] = 0.28209479f;
    Y[1] = 0.48860251f * y;
    Y[2] = 0.48860251f * z;
    Y[3] = 0.48860251f * x;
    Y[4] = 1.09254843f * (x * y);
    Y[5] = 1.09254843f * (y * z);
    Y[6] = 0.31539157f * (3.0f * (z * z) - 1.0f);
    Y[7] = 1.09254843f * (x * z);
    Y[8] = 0.54627422f * (x * x - y * y);
}

PT_SH_HD float luminance(const float L[3]) { return (L[0] * 0.299f + L[1] * 0.587f) + L[2] * 0.114f; }

// one sample into a lane's 28 partial sums: acc[3 k + c] and acc[27] = m2
PT_SH_HD void accumulate(float acc[28], const float L[3], const float w[3])
{
    float Y[9];
    basis(w, Y);
    for (uint32_t k = 0; k < kCoeffs; ++k)
        for (uint32_t c = 0; c < 3u; ++c) acc[3u * k + c] = acc[3u * k + c] + L[c] * Y[k];
    const float lum = luminance(L);
    acc[27] = acc[27] + lum * lum;
}

// The fold of the 64 lane partials of one sum, in place: v[0] receives the value.  The kernel runs the same tree as an xor
// butterfly across the wave: lane l < h adds lane l ^ h = l + h, and an fp32 add does not depend on the order of its operands.
PT_SH_HD float fold(float v[64])
{
    for (uint32_t h = 32u; h >= 1u; h >>= 1)
        for (uint32_t l = 0; l < h; ++l) v[l] = v[l] + v[l + h];
    return v[0];
}

PT_SH_HD float scale(float v0, uint32_t samples) { return (v0 * kFourPi) / (float)samples; }

// a visible point or spot light: sh[3 k + c] += Li[c] * Y_k(dir)
PT_SH_HD void add_delta(float sh[27], const float Li[3], const float dir[3])
{
    float Y[9];
    basis(dir, Y);
    for (uint32_t k = 0; k < kCoeffs; ++k)
        for (uint32_t c = 0; c < 3u; ++c) sh[3u * k + c] = sh[3u * k + c] + Li[c] * Y[k];
}

// E(N): the cosine lobe's band factors PI, 2 PI / 3, PI / 4
PT_SH_HD void irradiance(const float sh[27], const float N[3], float E[3])
{
    float Y[9];
    basis(N, Y);
    for (uint32_t c = 0; c < 3u; ++c) {
        float e = 0.0f;
        for (uint32_t k = 0; k < kCoeffs; ++k) {
            const float A = k == 0u ? 3.14159265f : k < 4u ? 2.09439510f : 0.78539816f;
            e = e + (A * sh[3u * k + c]) * Y[k];
        }
        E[c] = e;
    }
}

// ---- the host twins (probe_host.cpp); false: err says why ----
bool probe_directions_host(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, PTRadianceRay* rays, std::string& err);
bool probe_project_host(const float* directions, const float* colours, uint64_t count, uint32_t samples, PTProbeCoeffs* out, std::string& err);
bool probe_irradiance_host(const PTProbeCoeffs* sh, uint64_t probeCount, const PTProbeQuery* queries, uint64_t count, PTIrradiance* out, std::string& err);

} // namespace ptsh
