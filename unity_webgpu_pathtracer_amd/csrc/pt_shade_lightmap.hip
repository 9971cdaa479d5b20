// pt_shade_lightmap.hip — first hits shaded from baked lightmaps (include/ptmi_plugin.h Part 22).
//
//     pt_lightmap_lookup    one lane per entry: the hit record, rows 1 and 2 of the surface record and the ray's direction (16-byte
//                           loads), the binding walk (record k is the same in every lane of the wave: three 16-byte scalar loads, the
//                           match a few VALU operations per lane; the walk ends once every lane of the wave has its binding), the
//                           three corners' UVs (three 8-byte loads from the binding's array, or rows 6 and 7 of the attribute
//                           record), the four taps (clamped into the image, so all four are requested before the first is used; the
//                           two of a row are 32 contiguous bytes), the filter over the valid ones
//     pt_shade_lightmapped[_placed]  pt_shade_baked[_placed] with that lookup in front of the volume's: pt_shade_hit.h's front, the
//                           lightmap lookup, the volume lookup under "not found" (a wave pays for it when one of its lanes needs
//                           it), the reflection lookup, the compose step -- the functions the separate kernels call
//
// The arithmetic is lightmap_lookup_rule.h's, which the host twin evaluates too.
#include "pt_device.h"
#include "pt_launch.h"
#include "pt_shade_hit.h"
#include "lightmap_lookup_rule.h"

namespace {

// The table hands the images and UV arrays over as integers: without the address space their loads would be flat ones.
typedef float pt_vec2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) pt_vec4 pt_global_vec4;
typedef __attribute__((address_space(1))) pt_vec2 pt_global_vec2;

// steps 2 to 6 of the rule for one lane; every lane of the wave that is still in the kernel calls it
PT_DEV uint32_t lightmap_lane(const float4* __restrict__ attrs, const float4* __restrict__ table, uint32_t bindingCount, bool miss, bool back, uint32_t prim,
                              float bu, float bv, uint32_t instance, float E[4])
{
    return ptlm::lookup(miss, back, prim, bu, bv, instance, bindingCount,
                        [&](uint32_t k) {
                            const float4 r0 = pt_uniform_load(table, 3u * (size_t)k), r1 = pt_uniform_load(table, 3u * (size_t)k + 1u),
                                         r2 = pt_uniform_load(table, 3u * (size_t)k + 2u);
                            PTLightmapBinding b;
                            b.firstPrim = pt_asuint(r0.x); b.primCount = pt_asuint(r0.y); b.instance = pt_asuint(r0.z); b.flags = pt_asuint(r0.w);
                            b.width = pt_asuint(r1.x); b.height = pt_asuint(r1.y); b.reserved[0] = b.reserved[1] = 0u;
                            b.dImage = (const void*)(uintptr_t)((uint64_t)pt_asuint(r2.x) | ((uint64_t)pt_asuint(r2.y) << 32));
                            b.dUvs = (const float*)(uintptr_t)((uint64_t)pt_asuint(r2.z) | ((uint64_t)pt_asuint(r2.w) << 32));
                            return b;
                        },
                        [](bool done) { return __all(done) != 0; },
                        [&](const ptlm::Chosen& c, uint32_t p, float uv[6]) {
                            if (c.uvs) {
                                const pt_global_vec2* q = (const pt_global_vec2*)(uintptr_t)c.uvs + 3u * (size_t)(p - c.firstPrim);
                                const pt_vec2 a = q[0], b = q[1], d = q[2];
                                uv[0] = a.x; uv[1] = a.y; uv[2] = b.x; uv[3] = b.y; uv[4] = d.x; uv[5] = d.y;
                            } else {
                                const float4 uv01 = attrs[(size_t)p * 8u + 6u], uv2m = attrs[(size_t)p * 8u + 7u];
                                uv[0] = uv01.x; uv[1] = uv01.y; uv[2] = uv01.z; uv[3] = uv01.w; uv[4] = uv2m.x; uv[5] = uv2m.y;
                            }
                        },
                        [](const ptlm::Chosen& c, const uint32_t index[4], float t[4][4]) {
                            const pt_global_vec4* image = (const pt_global_vec4*)(uintptr_t)c.image;
                            pt_vec4 v0 = image[index[0]], v1 = image[index[1]], v2 = image[index[2]], v3 = image[index[3]];
                            asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));          // all four taps requested before the first is used
                            const pt_vec4 v[4] = {v0, v1, v2, v3};
                            for (uint32_t k = 0; k < 4u; ++k) { t[k][0] = v[k].x; t[k][1] = v[k].y; t[k][2] = v[k].z; t[k][3] = v[k].w; }
                        },
                        E);
}

// step 1 of the rule for entry i: the words of the hit, the surface record and the ray that the lookup reads
struct LightmapHit {
    bool miss, back;
    uint32_t prim, instance;
    float bu, bv;
};

PT_DEV LightmapHit lightmap_hit(uint32_t materialCount, const PTRay* __restrict__ rays, const PTRayHit* __restrict__ hits, const PTRaySurface* __restrict__ surfaces,
                                uint32_t i)
{
    const float4 hr = ((const float4*)hits)[i];
    LightmapHit l = {pt_asuint(hr.w) == 0xFFFFFFFFu, false, pt_asuint(hr.w), 0u, hr.y, hr.z};
    if (l.miss) return l;
    const float4* sp = (const float4*)surfaces + (size_t)i * 3;
    const float4 s1 = sp[1], s2 = sp[2];
    l.miss = pt_asuint(s1.w) >= materialCount;
    if (l.miss) return l;
    l.instance = pt_asuint(s2.z);
    const float4 r0 = ((const float4*)rays)[(size_t)i * 2], r1 = ((const float4*)rays)[(size_t)i * 2 + 1];
    const float D[3] = {r0.w, r1.x, r1.y}, N[3] = {s1.x, s1.y, s1.z};
    l.back = ptlm::seen_from_behind(D, N);
    return l;
}

__global__ __launch_bounds__(256) void pt_lightmap_lookup(const float4* __restrict__ attrs, uint32_t materialCount, const float4* __restrict__ table,
                                                          uint32_t bindingCount, const PTRay* __restrict__ rays, const PTRayHit* __restrict__ hits,
                                                          const PTRaySurface* __restrict__ surfaces, uint32_t count, float4* __restrict__ out,
                                                          uint32_t* __restrict__ outBinding)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const LightmapHit l = lightmap_hit(materialCount, rays, hits, surfaces, i);
    float E[4];
    const uint32_t k = lightmap_lane(attrs, table, bindingCount, l.miss, l.back, l.prim, l.bu, l.bv, l.instance, E);
    out[i] = make_float4(E[0], E[1], E[2], E[3]);
    if (outBinding) outBinding[i] = k;
}

__global__ __launch_bounds__(256) void pt_shade_lightmapped(DScene S, PTShadeInputs A, uint32_t mapTexels, const float4* __restrict__ table,
                                                            uint32_t bindingCount, const PTRay* __restrict__ rays, const PTRayHit* __restrict__ hits,
                                                            const PTRaySurface* __restrict__ surfaces, uint32_t count, float4* __restrict__ out)
{
    // the body's front has taken step 1 of this hit already: a lane that gets here is no miss, and the loads repeat its own
    shade_baked_body<false>(S, A, mapTexels, rays, hits, surfaces, count, out, [&](uint32_t i, float E[4]) {
        const LightmapHit l = lightmap_hit(S.materialCount, rays, hits, surfaces, i);
        return lightmap_lane(S.attrs, table, bindingCount, l.miss, l.back, l.prim, l.bu, l.bv, l.instance, E) != PT_LIGHTMAP_NONE;
    });
}

__global__ __launch_bounds__(256) void pt_shade_lightmapped_placed(DScene S, PTShadeInputs A, uint32_t mapTexels, const float4* __restrict__ table,
                                                                   uint32_t bindingCount, const PTRay* __restrict__ rays, const PTRayHit* __restrict__ hits,
                                                                   const PTRaySurface* __restrict__ surfaces, uint32_t count, float4* __restrict__ out)
{
    // the body's front has taken step 1 of this hit already: a lane that gets here is no miss, and the loads repeat its own
    shade_baked_body<true>(S, A, mapTexels, rays, hits, surfaces, count, out, [&](uint32_t i, float E[4]) {
        const LightmapHit l = lightmap_hit(S.materialCount, rays, hits, surfaces, i);
        return lightmap_lane(S.attrs, table, bindingCount, l.miss, l.back, l.prim, l.bu, l.bv, l.instance, E) != PT_LIGHTMAP_NONE;
    });
}

} // namespace

hipError_t pt_launch_lightmap_lookup(const DScene& S, const PTLightmapBinding* table, uint32_t bindingCount, const PTRay* rays, const PTRayHit* hits,
                                     const PTRaySurface* surfaces, uint32_t count, PTIrradiance* out, uint32_t* outBinding, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    if (bindingCount > PT_LIGHTMAP_MAX_BINDINGS || (bindingCount && !table)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_lightmap_lookup, dim3((count + 255u) / 256u), dim3(256), 0, stream, S.attrs, S.materialCount, (const float4*)table, bindingCount, rays,
                       hits, surfaces, count, (float4*)out, outBinding);
    return hipGetLastError();
}

hipError_t pt_launch_shade_lightmapped(const DScene& S, const PTShadeInputs& in, const PTLightmapBinding* table, uint32_t bindingCount, const PTRay* rays,
                                       const PTRayHit* hits, const PTRaySurface* surfaces, uint32_t count, float4* out, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    if (!ptshade::dfg_res_ok(in.dfgRes) || ((in.grid.flags & PT_GRID_VISIBILITY) && !in.dDepth) || (in.probeCount && (!in.dProbes || !in.dMaps)) ||
        (in.dBoxes && !in.dProbes) || bindingCount > PT_LIGHTMAP_MAX_BINDINGS || (bindingCount && !table))
        return hipErrorInvalidValue;
    const uint32_t mapTexels = ptrefl::level_offset(in.res, in.levels);
    const dim3 grid((count + 255u) / 256u);
    if (in.dPlacement)
        hipLaunchKernelGGL(pt_shade_lightmapped_placed, grid, dim3(256), 0, stream, S, in, mapTexels, (const float4*)table, bindingCount, rays, hits, surfaces,
                           count, out);
    else
        hipLaunchKernelGGL(pt_shade_lightmapped, grid, dim3(256), 0, stream, S, in, mapTexels, (const float4*)table, bindingCount, rays, hits, surfaces, count,
                           out);
    return hipGetLastError();
}
