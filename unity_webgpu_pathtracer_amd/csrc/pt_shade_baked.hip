// pt_shade_baked.hip — shading from the bakes (include/ptmi_plugin.h Part 21).
//
//     pt_shade_dfg          one WAVE per table entry, lane q = azimuth q: 64 radial samples per lane in registers, an xor butterfly
//                           folds the two sums, lane 0 stores 8 bytes
//     pt_shade_surfaces     one lane per entry: the render's material fetch (get_material, called, not restated), the terms, the
//                           probe choice (the probes and boxes walked through wave-uniform scalar loads); up to four record stores
//     pt_shade_compose      one lane per entry: three 16-byte loads of terms, one each of irradiance and radiance, four 8-byte
//                           table entries
//     pt_shade_baked[_placed]  the fused call: the front of pt_shade_surfaces, volume_rule.h's lookup with pt_volume_loads.h's
//                           loads, reflection_rule.h's lookup, the compose step -- nothing between them leaves the registers.  The
//                           grid, the sizes and every base pointer arrive by value in the kernel arguments (scalar registers)
//                           (the lane's text is pt_shade_hit.h's, which Part 22's kernels share)
//     pt_shade_frame_rays   one lane per pixel: the guides' pinhole ray at one sample per pixel (pt_denoise.hip's expressions)
//
// The arithmetic is shade_rule.h's, which the host twins evaluate too.
#include "pt_device.h"
#include "pt_launch.h"
#include "shade_rule.h"
#include "pt_shade_hit.h"

namespace {

// Four entries per workgroup; a wave is whole in or whole out.
__global__ __launch_bounds__(256) void pt_shade_dfg(uint32_t res, PTShadeDFG* __restrict__ out)
{
    const uint32_t entry = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (entry >= res * res) return;
    float a, b;
    ptshade::dfg_lane(res, entry % res, entry / res, lane, a, b);
#pragma unroll
    for (uint32_t h = 32u; h >= 1u; h >>= 1) {
        a = a + __shfl_xor(a, (int)h, 64);
        b = b + __shfl_xor(b, (int)h, 64);
    }
    if (lane == 0u) ((float2*)out)[entry] = make_float2(ptshade::dfg_scale(a), ptshade::dfg_scale(b));
}

__global__ __launch_bounds__(256) void pt_shade_surfaces(DScene S, const PTRay* __restrict__ rays, const PTRayHit* __restrict__ hits,
                                                         const PTRaySurface* __restrict__ surfaces, uint32_t count, const PTProbe* __restrict__ probes,
                                                         const PTReflectionBox* __restrict__ boxes, uint32_t probeCount, PTShadeMaterial* __restrict__ outMaterial,
                                                         PTShadeTerms* __restrict__ outTerms, PTReceiver* __restrict__ outReceivers,
                                                         PTReflectionQuery* __restrict__ outQueries)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    HitRecords h;
    hit_records(S, rays, hits, surfaces, i, probes, boxes, probeCount, h);
    if (outMaterial) {
        float4* o = (float4*)outMaterial + (size_t)i * 3;
        o[0] = make_float4(h.M.baseColor[0], h.M.baseColor[1], h.M.baseColor[2], h.M.metallic);
        o[1] = make_float4(h.M.emission[0], h.M.emission[1], h.M.emission[2], h.M.roughness);
        o[2] = make_float4(h.M.occlusion, h.M.opacity, pt_asfloat(h.M.materialIndex), pt_asfloat(h.M.flags));
    }
    if (outTerms) {
        float4* o = (float4*)outTerms + (size_t)i * 3;
        o[0] = make_float4(h.T.diffuse[0], h.T.diffuse[1], h.T.diffuse[2], h.T.rho);
        o[1] = make_float4(h.T.f0[0], h.T.f0[1], h.T.f0[2], h.T.nDotV);
        o[2] = make_float4(h.T.emission[0], h.T.emission[1], h.T.emission[2], h.T.occlusion);
    }
    if (outReceivers) {
        float4* o = (float4*)outReceivers + (size_t)i * 2;
        o[0] = make_float4(h.P[0], h.P[1], h.P[2], pt_asfloat(0u));
        o[1] = make_float4(h.N[0], h.N[1], h.N[2], pt_asfloat(0u));
    }
    if (outQueries) {
        float4* o = (float4*)outQueries + (size_t)i * 2;
        o[0] = make_float4(h.P[0], h.P[1], h.P[2], h.T.rho);
        o[1] = make_float4(h.R[0], h.R[1], h.R[2], pt_asfloat(h.probe));
    }
}

__global__ __launch_bounds__(256) void pt_shade_compose(const PTShadeTerms* __restrict__ terms, const PTIrradiance* __restrict__ irradiance,
                                                        const PTReflectionTexel* __restrict__ reflection, uint32_t count, const PTShadeDFG* __restrict__ dfg,
                                                        uint32_t dfgRes, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const float4* tp = (const float4*)terms + (size_t)i * 3;
    const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
    const PTShadeTerms T = {{t0.x, t0.y, t0.z}, t0.w, {t1.x, t1.y, t1.z}, t1.w, {t2.x, t2.y, t2.z}, t2.w};
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!ptshade::is_miss(T)) {
        const float4 e = ((const float4*)irradiance)[i], s = ((const float4*)reflection)[i];
        const float E[3] = {e.x, e.y, e.z}, spec[3] = {s.x, s.y, s.z};
        float A, B;
        ptshade::dfg_lookup(dfgRes, T.nDotV, T.rho, [&](uint32_t k, float ab[2]) { dfg_entry(dfg, k, ab); }, A, B);
        ptshade::compose(T, E, spec, A, B, o);
    }
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void pt_shade_baked(DScene S, PTShadeInputs A, uint32_t mapTexels, const PTRay* __restrict__ rays,
                                                      const PTRayHit* __restrict__ hits, const PTRaySurface* __restrict__ surfaces, uint32_t count,
                                                      float4* __restrict__ out)
{
    shade_baked_body<false>(S, A, mapTexels, rays, hits, surfaces, count, out, [](uint32_t, float*) { return false; });
}

__global__ __launch_bounds__(256) void pt_shade_baked_placed(DScene S, PTShadeInputs A, uint32_t mapTexels, const PTRay* __restrict__ rays,
                                                             const PTRayHit* __restrict__ hits, const PTRaySurface* __restrict__ surfaces, uint32_t count,
                                                             float4* __restrict__ out)
{
    shade_baked_body<true>(S, A, mapTexels, rays, hits, surfaces, count, out, [](uint32_t, float*) { return false; });
}

// pixel first + k of the frame: pt_denoise.hip's guide ray with n = 1 (the offset (0 + 0.5f) / 1.0f is 0.5f)
__global__ __launch_bounds__(256) void pt_shade_frame_rays(PTFrameParams P, uint32_t first, uint32_t count, PTRay* __restrict__ rays)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= count) return;
    const uint32_t W = P.OutputWidth, H = P.OutputHeight;
    const uint32_t pix = first + k, x = pix % W, y = pix / W;
    const v4 o4 = mul44(P.CamToWorld, v4{0.0f, 0.0f, 0.0f, 1.0f});
    const float pcx = (float)x + 0.5f, pcy = (float)y + 0.5f;
    const float uvx = pcx / (float)W * 2.0f - 1.0f;
    const float uvy = pcy / (float)H * 2.0f - 1.0f;
    const v4 d4 = mul44(P.CamInvProj, v4{uvx, uvy, 0.0f, 1.0f});
    const v4 w4 = mul44(P.CamToWorld, v4{d4.x, d4.y, d4.z, 0.0f});
    const v3 d = normalize3(mk3(w4.x, w4.y, w4.z));
    float4* e = (float4*)(rays + k);
    e[0] = make_float4(o4.x, o4.y, o4.z, d.x);
    e[1] = make_float4(d.y, d.z, PT_FAR_PLANE, pt_asfloat(0u));
}

} // namespace

hipError_t pt_launch_shade_dfg(uint32_t res, PTShadeDFG* out, hipStream_t stream)
{
    if (!ptshade::dfg_res_ok(res)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_shade_dfg, dim3((res * res + 3u) / 4u), dim3(256), 0, stream, res, out);
    return hipGetLastError();
}

hipError_t pt_launch_shade_surfaces(const DScene& S, const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces, uint32_t count, const PTProbe* probes,
                                    const PTReflectionBox* boxes, uint32_t probeCount, PTShadeMaterial* outMaterial, PTShadeTerms* outTerms,
                                    PTReceiver* outReceivers, PTReflectionQuery* outQueries, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    if ((probeCount && !probes) || (boxes && !probes)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_shade_surfaces, dim3((count + 255u) / 256u), dim3(256), 0, stream, S, rays, hits, surfaces, count, probes, boxes, probeCount,
                       outMaterial, outTerms, outReceivers, outQueries);
    return hipGetLastError();
}

hipError_t pt_launch_shade_compose(const PTShadeTerms* terms, const PTIrradiance* irradiance, const PTReflectionTexel* reflection, uint32_t count,
                                   const PTShadeDFG* dfg, uint32_t dfgRes, float4* out, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    if (!ptshade::dfg_res_ok(dfgRes)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_shade_compose, dim3((count + 255u) / 256u), dim3(256), 0, stream, terms, irradiance, reflection, count, dfg, dfgRes, out);
    return hipGetLastError();
}

hipError_t pt_launch_shade_baked(const DScene& S, const PTShadeInputs& in, const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces, uint32_t count,
                                 float4* out, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    if (!ptshade::dfg_res_ok(in.dfgRes) || ((in.grid.flags & PT_GRID_VISIBILITY) && !in.dDepth) || (in.probeCount && (!in.dProbes || !in.dMaps)) ||
        (in.dBoxes && !in.dProbes))
        return hipErrorInvalidValue;
    const uint32_t mapTexels = ptrefl::level_offset(in.res, in.levels);
    if (in.dPlacement)
        hipLaunchKernelGGL(pt_shade_baked_placed, dim3((count + 255u) / 256u), dim3(256), 0, stream, S, in, mapTexels, rays, hits, surfaces, count, out);
    else
        hipLaunchKernelGGL(pt_shade_baked, dim3((count + 255u) / 256u), dim3(256), 0, stream, S, in, mapTexels, rays, hits, surfaces, count, out);
    return hipGetLastError();
}

hipError_t pt_launch_shade_frame_rays(const PTFrameParams& P, uint32_t first, uint32_t count, PTRay* rays, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_shade_frame_rays, dim3((count + 255u) / 256u), dim3(256), 0, stream, P, first, count, rays);
    return hipGetLastError();
}
