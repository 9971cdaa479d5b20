/*
 * pt_env_cdf.h — the CDF of HAS_ENVIRONMENT_TEXTURE, built on the host (plain C++, no HIP).
 *
 * OnEnvTexReadback (PathTracer.cs:297-306): a running fp32 sum of Color.grayscale = 0.299 r + 0.587 g + 0.114 b over the texels
 * in memory order, cdf[i] = the sum after texel i.  PTSetScene (pt_api_context.hip) uploads it; the environment probe of the tests
 * (env_probe.hip) uploads the same bytes.
 */
#pragma once
#include <cstddef>

/* texels: n x RGBA float32; cdf: n floats out.  Returns the sum (0 for n == 0). */
inline float pt_env_build_cdf(const float* texels, size_t n, float* cdf)
{
    float cdfSum = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float* px = texels + 4 * i;
        cdfSum += 0.299f * px[0] + 0.587f * px[1] + 0.114f * px[2];
        cdf[i] = cdfSum;
    }
    return cdfSum;
}
