/*
 * env_probe.hip — evaluates the environment-map functions of pt_device.h ON THE DEVICE, one element per lane (test infrastructure:
 * libpt-env-probe.so, `make env-probe`; not part of the product library).
 *
 * tests/test_gpu_env.py compares the bits this returns with the oracle's (oracle_env_probe), which runs its own restatement of
 * util/sky.hlsl on the host.  The functions are pt_device.h's own -- env_sample_level, env_binary_search, eval_env_map,
 * sample_env_map -- over a DScene that has only its environment fields set; the CDF is the one PTSetScene uploads (pt_env_cdf.h).
 *
 * `what` follows oracle_env_probe; floats in, floats out, per element:
 *   0  in: index i                 out: envCdf[i]
 *   1  in: value                   out: env_binary_search(value) -> u, v
 *   2  in: direction x, y, z       out: eval_env_map(direction, 1) -> r, g, b, pdf
 *   3  in: RNG state (its bits)    out: sample_env_map -> direction x, y, z, pdf, colour r, g, b, 0
 *   4  in: u, v                    out: env_sample_level(u, v) -> r, g, b
 *
 * Compiled twice, as the product's kernels are: this file with HIPFLAGS holds the entry point and the kernel of unit 0;
 * with HIPFLAGS_A and -DPT_ENV_PROBE_UNIT_A (the flags of the default schedule's unit) it holds the kernel of unit 1 only.
 */
#include <hip/hip_runtime.h>

#include "pt_device.h"

#ifdef PT_ENV_PROBE_UNIT_A
#define PROBE_KERNEL pt_env_probe_kernel_a
#define PROBE_LAUNCH pt_env_probe_launch_a
#else
#define PROBE_KERNEL pt_env_probe_kernel
#define PROBE_LAUNCH pt_env_probe_launch
#endif

/* every index the four functions form is clamped to the map (env_sample_level) or stays inside the search bounds
 * (env_binary_search); what 0 indexes with the caller's value, which the entry point has checked against W x H */
__global__ __launch_bounds__(256) void PROBE_KERNEL(DScene S, PTFrameParams P, int what, const float* __restrict__ in, uint64_t n,
                                                    float* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (what == 0) {
        out[i] = S.envCdf[(size_t)in[i]];
    } else if (what == 1) {
        float u, v;
        env_binary_search(S, in[i], u, v);
        out[2 * i] = u; out[2 * i + 1] = v;
    } else if (what == 2) {
        const v4 r = eval_env_map(S, P, mk3(in[3 * i], in[3 * i + 1], in[3 * i + 2]), 1.0f);
        float* o = out + 4 * i;
        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
    } else if (what == 3) {
        uint32_t rng = ((const uint32_t*)in)[i];
        v3 col = mk3(0.0f);
        const v4 r = sample_env_map(S, P, col, rng);
        float* o = out + 8 * i;
        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w; o[4] = col.x; o[5] = col.y; o[6] = col.z; o[7] = 0.0f;
    } else {
        const v3 c = env_sample_level(S, in[2 * i], in[2 * i + 1]);
        float* o = out + 3 * i;
        o[0] = c.x; o[1] = c.y; o[2] = c.z;
    }
}

hipError_t PROBE_LAUNCH(const DScene& S, const PTFrameParams& P, int what, const float* in, uint64_t n, float* out)
{
    PROBE_KERNEL<<<dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, 0>>>(S, P, what, in, n, out);
    return hipGetLastError();
}

#ifndef PT_ENV_PROBE_UNIT_A
#include <cstring>
#include <vector>

#include "pt_env_cdf.h"

hipError_t pt_env_probe_launch_a(const DScene& S, const PTFrameParams& P, int what, const float* in, uint64_t n, float* out);

/* Host arrays in and out; 0 on success, a hipError_t otherwise (unit: 0 = HIPFLAGS, 1 = HIPFLAGS_A; anything else is an error).
 * texels: H rows of W RGBA float32 texels, in the order PTSceneDesc.envTexture has them. */
extern "C" __attribute__((visibility("default")))
int PTEnvProbe(int unit, int what, const float* texels, int32_t W, int32_t H, float rotation, const float* in, uint64_t n, float* out)
{
    static const size_t perIn[5] = {1, 1, 3, 1, 2}, perOut[5] = {1, 2, 4, 8, 3};
    if ((unit != 0 && unit != 1) || what < 0 || what > 4 || !texels || W < 1 || H < 1 || W > 4096 || H > 4096 || !in || !out || n > (1ull << 24))
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const size_t texelCount = (size_t)W * (size_t)H;
    if (what == 0)
        for (uint64_t k = 0; k < n; ++k)
            if (!(in[k] >= 0.0f && in[k] < (float)texelCount)) return (int)hipErrorInvalidValue;
    std::vector<float> cdf(texelCount);
    const float cdfSum = pt_env_build_cdf(texels, texelCount, cdf.data());
    const size_t inBytes = (size_t)n * perIn[what] * sizeof(float), outBytes = (size_t)n * perOut[what] * sizeof(float);
    float4* dTex = nullptr;
    float *dCdf = nullptr, *dIn = nullptr, *dOut = nullptr;
    hipError_t e = hipSetDevice(0);
    if (e == hipSuccess) e = hipMalloc(&dTex, texelCount * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc(&dCdf, texelCount * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dIn, inBytes);
    if (e == hipSuccess) e = hipMalloc(&dOut, outBytes);
    if (e == hipSuccess) e = hipMemcpy(dTex, texels, texelCount * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dCdf, cdf.data(), texelCount * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dIn, in, inBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        DScene S;
        memset(&S, 0, sizeof(S));
        S.envTex = dTex; S.envCdf = dCdf; S.envW = W; S.envH = H; S.envCdfSum = cdfSum; S.hasEnvTex = 1u;
        PTFrameParams P;
        memset(&P, 0, sizeof(P));
        P.EnvironmentMapRotation = rotation;
        e = unit ? pt_env_probe_launch_a(S, P, what, dIn, n, dOut) : pt_env_probe_launch(S, P, what, dIn, n, dOut);
    }
    if (e == hipSuccess) e = hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost);      /* synchronises with the kernel */
    (void)hipFree(dTex);
    (void)hipFree(dCdf);
    (void)hipFree(dIn);
    (void)hipFree(dOut);
    return (int)e;
}
#endif
