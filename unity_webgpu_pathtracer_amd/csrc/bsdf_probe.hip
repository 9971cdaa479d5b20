/*
 * bsdf_probe.hip — evaluates the material fetch and the BSDF functions of pt_device.h ON THE DEVICE, one element per lane (test
 * infrastructure: libpt-bsdf-probe.so, `make bsdf-probe`; not part of the product library).
 *
 * tests/test_gpu_bsdf.py compares the bits this returns with the oracle's (oracle_bsdf_probe), which runs its own restatement of
 * util/material.hlsl, util/texture.hlsl, util/sampling.hlsl and util/brdf.hlsl on the host.  The functions are pt_device.h's own --
 * get_material, sample_texture, sample_textures4, the sampling helpers, tint_colors, lobe_weights, make_onb, onb_of_normal, eval_brdf_onb,
 * sample_brdf -- over a DScene that has only materials, materialCount, tex and hasTextures set.
 *
 * `what` follows oracle_bsdf_probe; floats in, floats out, per element (an RNG state travels as its bits):
 *   0  in: material index, u, v, ray direction xyz, normal xyz                 (9)
 *      out: the 24 floats of Material from get_material<true>, the 24 from get_material<false>, then materialFetches, texDescFetches,
 *           texelFetches of the <true> form                                    (51)
 *   1  in: texture index, u, v                                                 (3)
 *      out: sample_texture<false> -> rgba, then sample_textures4<false> with that texture wanted in slot 0, 1, 2, 3 in turn (the
 *           other three unwanted) -> the wanted slot's rgba each time          (20)
 *   2  in: function id, seven operands                                         (8)
 *      out: nine floats, the unused ones 0.  0 gtr1(a0, a1)  1 sample_gtr1(a0, a1, a2)  2 sample_ggx_vndf(V = a0..2, a3, a4, a5, a6)
 *           3 gtr2_aniso(a0..4)  4 smith_g(a0, a1)  5 smith_g_aniso(a0..4)  6 schlick_weight(a0)  7 dielectric_fresnel(a0, a1)
 *           8 cosine_sample_hemisphere(a0, a1)  9 power_heuristic(a0, a1)  10 reflect3(i = a0..2, n = a3..5)
 *           11 refract3(i = a0..2, n = a3..5, a6)  12 make_onb(a0..2) -> x, y, z  13 luminance3(a0..2)
 *   3  in: material index, u, v, V xyz, hit normal xyz, roughness floor        (10)
 *      out: F0, Csheen, Cspec0, the eight Lobes values at V.z in the basis of the face-forward normal    (15)
 *   4  in: as 3, then L xyz and a flag: 0 = the basis of ffnormal, otherwise the basis of normal through onb_of_normal   (14)
 *      out: eval_brdf_onb -> f xyz, pdf                                        (4)
 *   5  in: as 3, then an RNG state                                             (11)
 *      out: sample_brdf -> L xyz, f xyz, pdf, the RNG state after              (8)
 * What 3 to 5 run in path_shade_hit's setting: the ray direction is -V, ffnormal = dot(normal, dir) <= 0 ? normal : -normal
 * (fetch_hit_attributes), get_material, material.roughness = max(floor, roughness), tint_colors(material, material.eta),
 * ffOnb = make_onb(ffnormal).
 *
 * Compiled twice, as the product's kernels are: this file with HIPFLAGS holds the entry point and the kernel of unit 0;
 * with HIPFLAGS_A and -DPT_BSDF_PROBE_UNIT_A (the flags of the default schedule's unit) it holds the kernel of unit 1 only.
 */
#include <hip/hip_runtime.h>

#include "pt_device.h"

#ifdef PT_BSDF_PROBE_UNIT_A
#define PROBE_KERNEL pt_bsdf_probe_kernel_a
#define PROBE_LAUNCH pt_bsdf_probe_launch_a
#else
#define PROBE_KERNEL pt_bsdf_probe_kernel
#define PROBE_LAUNCH pt_bsdf_probe_launch
#endif

#define PT_BSDF_PROBE_WHATS 6

PT_DEV void probe_store_material(float* o, const Material& m)
{
    o[0] = m.baseColor.x; o[1] = m.baseColor.y; o[2] = m.baseColor.z; o[3] = m.opacity;
    o[4] = m.emission.x; o[5] = m.emission.y; o[6] = m.emission.z; o[7] = m.alphaMode;
    o[8] = m.alphaCutoff; o[9] = m.anisotropic; o[10] = m.metallic; o[11] = m.roughness;
    o[12] = m.subsurface; o[13] = m.specularTint; o[14] = m.sheen; o[15] = m.sheenTint;
    o[16] = m.clearcoat; o[17] = m.clearcoatRoughness; o[18] = m.specTrans; o[19] = m.ior;
    o[20] = m.ax; o[21] = m.ay; o[22] = m.eta; o[23] = m.occlusion;
}

/* sample_textures4 with texture `index` wanted in slot SLOT alone */
template <int SLOT>
PT_DEV v4 probe_one_of_four(const DScene& S, int32_t index, v2 uv, Counters& cn)
{
    const bool want[4] = {SLOT == 0, SLOT == 1, SLOT == 2, SLOT == 3};
    const int32_t idx[4] = {index, index, index, index};
    const v2 uvs[4] = {uv, uv, uv, uv};
    v4 out[4];
    sample_textures4<false>(S, want, idx, uvs, out, cn);
    return out[SLOT];
}

/* every index the functions form is clamped to its texture (texture_pixel, sample_textures4); the material and texture indices
 * of the elements, the texture indices inside the materials and the descriptors have been checked by the entry point */
__global__ __launch_bounds__(256) void PROBE_KERNEL(DScene S, int what, const float* __restrict__ in, uint64_t n, float* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    Counters cn = {};
    if (what == 0) {
        const float* a = in + 9 * i;
        SurfHit hit = {};
        hit.uv = {a[1], a[2]};
        hit.normal = mk3(a[6], a[7], a[8]);
        const v3 dir = mk3(a[3], a[4], a[5]);
        float* o = out + 51 * i;
        probe_store_material(o, get_material<true>(S, (int32_t)a[0], dir, hit, cn));
        o[48] = (float)cn.materialFetches; o[49] = (float)cn.texDescFetches; o[50] = (float)cn.texelFetches;
        probe_store_material(o + 24, get_material<false>(S, (int32_t)a[0], dir, hit, cn));
    } else if (what == 1) {
        const float* a = in + 3 * i;
        const int32_t t = (int32_t)a[0];
        const v2 uv = {a[1], a[2]};
        float* o = out + 20 * i;
        const v4 r = sample_texture<false>(S, t, uv, cn);
        const v4 r0 = probe_one_of_four<0>(S, t, uv, cn), r1 = probe_one_of_four<1>(S, t, uv, cn);
        const v4 r2 = probe_one_of_four<2>(S, t, uv, cn), r3 = probe_one_of_four<3>(S, t, uv, cn);
        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
        o[4] = r0.x; o[5] = r0.y; o[6] = r0.z; o[7] = r0.w;
        o[8] = r1.x; o[9] = r1.y; o[10] = r1.z; o[11] = r1.w;
        o[12] = r2.x; o[13] = r2.y; o[14] = r2.z; o[15] = r2.w;
        o[16] = r3.x; o[17] = r3.y; o[18] = r3.z; o[19] = r3.w;
    } else if (what == 2) {
        const float* a = in + 8 * i;
        const int fn = (int)a[0];
        const float a0 = a[1], a1 = a[2], a2 = a[3], a3 = a[4], a4 = a[5], a5 = a[6], a6 = a[7];
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f, r4 = 0.0f, r5 = 0.0f, r6 = 0.0f, r7 = 0.0f, r8 = 0.0f;
        v3 t = mk3(0.0f);
        switch (fn) {
        case 0: r0 = gtr1(a0, a1); break;
        case 1: t = sample_gtr1(a0, a1, a2); r0 = t.x; r1 = t.y; r2 = t.z; break;
        case 2: t = sample_ggx_vndf(mk3(a0, a1, a2), a3, a4, a5, a6); r0 = t.x; r1 = t.y; r2 = t.z; break;
        case 3: r0 = gtr2_aniso(a0, a1, a2, a3, a4); break;
        case 4: r0 = smith_g(a0, a1); break;
        case 5: r0 = smith_g_aniso(a0, a1, a2, a3, a4); break;
        case 6: r0 = schlick_weight(a0); break;
        case 7: r0 = dielectric_fresnel(a0, a1); break;
        case 8: t = cosine_sample_hemisphere(a0, a1); r0 = t.x; r1 = t.y; r2 = t.z; break;
        case 9: r0 = power_heuristic(a0, a1); break;
        case 10: t = reflect3(mk3(a0, a1, a2), mk3(a3, a4, a5)); r0 = t.x; r1 = t.y; r2 = t.z; break;
        case 11: t = refract3(mk3(a0, a1, a2), mk3(a3, a4, a5), a6); r0 = t.x; r1 = t.y; r2 = t.z; break;
        case 12: {
            const Onb b = make_onb(mk3(a0, a1, a2));
            r0 = b.x.x; r1 = b.x.y; r2 = b.x.z; r3 = b.y.x; r4 = b.y.y; r5 = b.y.z; r6 = b.z.x; r7 = b.z.y; r8 = b.z.z;
            break;
        }
        case 13: r0 = luminance3(mk3(a0, a1, a2)); break;
        default: break;
        }
        float* o = out + 9 * i;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4; o[5] = r5; o[6] = r6; o[7] = r7; o[8] = r8;
    } else {
        const size_t per = what == 3 ? 10u : what == 4 ? 14u : 11u;
        const float* a = in + per * i;
        const v3 V = mk3(a[3], a[4], a[5]);
        const v3 rayDir = -V;
        SurfHit hit = {};
        hit.uv = {a[1], a[2]};
        hit.normal = mk3(a[6], a[7], a[8]);
        hit.ffnormal = dot3(hit.normal, rayDir) <= 0.0f ? hit.normal : -hit.normal;          // fetch_hit_attributes
        Material material = get_material<false>(S, (int32_t)a[0], rayDir, hit, cn);
        float maxRoughness = a[9];                                                            // path_shade_hit
        maxRoughness = pt_max(maxRoughness, material.roughness);
        material.roughness = maxRoughness;
        BsdfShared sh;
        tint_colors(material, material.eta, sh.F0, sh.Csheen, sh.Cspec0);
        const Onb ffOnb = make_onb(hit.ffnormal);
        if (what == 3) {
            const Lobes w = lobe_weights(material, sh.Cspec0, onb_to_local(ffOnb, -rayDir).z);
            float* o = out + 15 * i;
            o[0] = sh.F0; o[1] = sh.Csheen.x; o[2] = sh.Csheen.y; o[3] = sh.Csheen.z; o[4] = sh.Cspec0.x; o[5] = sh.Cspec0.y; o[6] = sh.Cspec0.z;
            o[7] = w.dielectricWt; o[8] = w.metalWt; o[9] = w.glassWt; o[10] = w.diffPr; o[11] = w.dielectricPr; o[12] = w.metalPr;
            o[13] = w.glassPr; o[14] = w.clearCtPr;
        } else if (what == 4) {
            const v3 L = mk3(a[10], a[11], a[12]);
            float pdf = 0.0f;
            v3 f;
            if (a[13] == 0.0f) f = eval_brdf_onb(material, -rayDir, L, ffOnb, pdf, sh);                                       // nee_prepare_environment
            else f = eval_brdf_onb(material, -rayDir, L, onb_of_normal(hit.normal, hit.ffnormal, ffOnb), pdf, sh);            // nee_prepare_light
            float* o = out + 4 * i;
            o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = pdf;
        } else {
            uint32_t rng = pt_asuint(a[10]);
            v3 L = mk3(0.0f);
            float pdf = 0.0f;
            const v3 f = sample_brdf(material, -rayDir, ffOnb, L, pdf, rng, sh);
            float* o = out + 8 * i;
            o[0] = L.x; o[1] = L.y; o[2] = L.z; o[3] = f.x; o[4] = f.y; o[5] = f.z; o[6] = pdf; o[7] = pt_asfloat(rng);
        }
    }
}

hipError_t PROBE_LAUNCH(const DScene& S, int what, const float* in, uint64_t n, float* out)
{
    PROBE_KERNEL<<<dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, 0>>>(S, what, in, n, out);
    return hipGetLastError();
}

#ifndef PT_BSDF_PROBE_UNIT_A
#include <cstring>

hipError_t pt_bsdf_probe_launch_a(const DScene& S, int what, const float* in, uint64_t n, float* out);

/* a whole number in [0, count) */
static bool probe_index_ok(float v, uint32_t count) { return v >= 0.0f && v < (float)count && v == (float)(uint32_t)v; }

/* Host arrays in and out; 0 on success, a hipError_t otherwise (unit: 0 = HIPFLAGS, 1 = HIPFLAGS_A; anything else is an error).
 * materials: materialCount x 32 floats (PTMaterialData); tex: TextureData (texUints words, 0 = a scene without textures: the
 * materials' texture slots are then never looked at).  Everything an element or a material can index with is checked here. */
extern "C" __attribute__((visibility("default")))
int PTBsdfProbe(int unit, int what, const float* materials, uint32_t materialCount, const uint32_t* tex, uint64_t texUints,
                const float* in, uint64_t n, float* out)
{
    static const size_t perIn[PT_BSDF_PROBE_WHATS] = {9, 3, 8, 10, 14, 11}, perOut[PT_BSDF_PROBE_WHATS] = {51, 20, 9, 15, 4, 8};
    if ((unit != 0 && unit != 1) || what < 0 || what >= PT_BSDF_PROBE_WHATS || !materials || materialCount < 1 || materialCount > (1u << 16) ||
        (texUints != 0 && !tex) || texUints > (1ull << 24) || !in || !out || n > (1ull << 24))
        return (int)hipErrorInvalidValue;
    // the descriptors: 4 words per texture in front of the texels, the first texture's texels right behind them
    uint32_t texCount = 0;
    if (texUints != 0) {
        if (texUints < 5 || tex[2] % 4u != 0 || tex[2] < 4 || tex[2] > texUints) return (int)hipErrorInvalidValue;
        texCount = tex[2] / 4u;
        for (uint32_t t = 0; t < texCount; ++t) {
            const uint64_t w = tex[4 * t], h = tex[4 * t + 1], off = tex[4 * t + 2];
            if (w < 1 || h < 1 || w > 4096 || h > 4096 || off < 4ull * texCount || off + w * h > texUints) return (int)hipErrorInvalidValue;
        }
        for (uint32_t m = 0; m < materialCount; ++m) {
            const float slots[4] = {materials[32 * m + 22], materials[32 * m + 23], materials[32 * m + 25], materials[32 * m + 26]};
            for (float s : slots)
                if (!(s < 0.0f) && !probe_index_ok(s, texCount)) return (int)hipErrorInvalidValue;     // get_material wants a slot that is not < 0
        }
    }
    if (what == 1 && texCount == 0) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (what != 2)
        for (uint64_t k = 0; k < n; ++k)
            if (!probe_index_ok(in[k * perIn[what]], what == 1 ? texCount : materialCount)) return (int)hipErrorInvalidValue;
    const size_t matBytes = (size_t)materialCount * 32 * sizeof(float), texBytes = (size_t)texUints * sizeof(uint32_t);
    const size_t inBytes = (size_t)n * perIn[what] * sizeof(float), outBytes = (size_t)n * perOut[what] * sizeof(float);
    float4* dMat = nullptr;
    uint32_t* dTex = nullptr;
    float *dIn = nullptr, *dOut = nullptr;
    hipError_t e = hipSetDevice(0);
    if (e == hipSuccess) e = hipMalloc(&dMat, matBytes);
    if (e == hipSuccess && texBytes) e = hipMalloc(&dTex, texBytes);
    if (e == hipSuccess) e = hipMalloc(&dIn, inBytes);
    if (e == hipSuccess) e = hipMalloc(&dOut, outBytes);
    if (e == hipSuccess) e = hipMemcpy(dMat, materials, matBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && texBytes) e = hipMemcpy(dTex, tex, texBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dIn, in, inBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        DScene S;
        memset(&S, 0, sizeof(S));
        S.materials = dMat; S.materialCount = materialCount; S.tex = dTex; S.hasTextures = texUints != 0 ? 1u : 0u;
        e = unit ? pt_bsdf_probe_launch_a(S, what, dIn, n, dOut) : pt_bsdf_probe_launch(S, what, dIn, n, dOut);
    }
    if (e == hipSuccess) e = hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost);      /* synchronises with the kernel */
    (void)hipFree(dMat);
    (void)hipFree(dTex);
    (void)hipFree(dIn);
    (void)hipFree(dOut);
    return (int)e;
}
#endif
