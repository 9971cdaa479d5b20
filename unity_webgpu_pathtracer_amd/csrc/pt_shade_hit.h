// pt_shade_hit.h — what the baked-light shading kernels share (pt_shade_baked.hip, Part 21; pt_shade_lightmap.hip, Part 22): the
// front of a lane -- the records of entry i, the material fetch, the terms, the probe choice --, the DFG table's load and the body
// of the fused kernels.  One text for both compile units, so the fused kernels of both run the same steps.
#pragma once
#include "pt_device.h"
#include "shade_rule.h"
#include "pt_volume_loads.h"

namespace {

struct HitRecords {
    bool miss;
    PTShadeMaterial M;
    PTShadeTerms T;
    float P[3], N[3], R[3];
    uint32_t probe;
};

// Steps 2 of the rule for entry i.  A surface record whose material index lies outside the scene's materials is taken as a miss:
// nothing is read through it.
PT_DEV void hit_records(const DScene& S, const PTRay* __restrict__ rays, const PTRayHit* __restrict__ hits, const PTRaySurface* __restrict__ surfaces,
                        uint32_t i, const PTProbe* __restrict__ probes, const PTReflectionBox* __restrict__ boxes, uint32_t probeCount, HitRecords& h)
{
    h.M = {};
    h.T = {};
    for (uint32_t a = 0; a < 3u; ++a) h.P[a] = h.N[a] = h.R[a] = 0.0f;
    h.probe = ptshade::kNoProbe;
    const float4 hr = ((const float4*)hits)[i];
    h.miss = pt_asuint(hr.w) == 0xFFFFFFFFu;
    uint32_t materialIndex = 0xFFFFFFFFu;
    float4 s0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), s1 = s0, s2 = s0;
    if (!h.miss) {
        const float4* sp = (const float4*)surfaces + (size_t)i * 3;
        s0 = sp[0]; s1 = sp[1]; s2 = sp[2];
        materialIndex = pt_asuint(s1.w);
        h.miss = materialIndex >= S.materialCount;
    }
    if (h.miss) {
        h.M.materialIndex = 0xFFFFFFFFu;
        h.M.flags = PT_SHADE_MISS;
        return;
    }
    const float4 r0 = ((const float4*)rays)[(size_t)i * 2], r1 = ((const float4*)rays)[(size_t)i * 2 + 1];
    const float D[3] = {r0.w, r1.x, r1.y};
    SurfHit sh = {};
    sh.position = mk3(s0.x, s0.y, s0.z);
    sh.distance = s0.w;
    sh.normal = mk3(s1.x, s1.y, s1.z);
    sh.uv = {s2.x, s2.y};
    sh.materialIndex = (int32_t)materialIndex;
    Counters cn = {};
    const Material m = get_material<false>(S, sh.materialIndex, mk3(D[0], D[1], D[2]), sh, cn);
    h.M.baseColor[0] = m.baseColor.x; h.M.baseColor[1] = m.baseColor.y; h.M.baseColor[2] = m.baseColor.z;
    h.M.metallic = m.metallic;
    h.M.emission[0] = m.emission.x; h.M.emission[1] = m.emission.y; h.M.emission[2] = m.emission.z;
    h.M.roughness = m.roughness;
    h.M.occlusion = m.occlusion;
    h.M.opacity = m.opacity;
    h.M.materialIndex = materialIndex;
    h.M.flags = 0u;
    h.P[0] = s0.x; h.P[1] = s0.y; h.P[2] = s0.z;
    h.N[0] = s1.x; h.N[1] = s1.y; h.N[2] = s1.z;
    ptshade::terms(h.M, D, h.N, h.R, h.T);
    // k is the same in every lane of the wave: scalar loads
    h.probe = ptshade::choose_probe(h.P, probeCount, boxes != nullptr,
                                    [&](uint32_t k, float Q[3]) {
                                        const float4 p = pt_uniform_load((const float4*)probes, k);
                                        Q[0] = p.x; Q[1] = p.y; Q[2] = p.z;
                                    },
                                    [&](uint32_t k, float bmin[3], float bmax[3]) {
                                        const float4 b0 = pt_uniform_load((const float4*)boxes, 2u * (size_t)k), b1 = pt_uniform_load((const float4*)boxes, 2u * (size_t)k + 1u);
                                        bmin[0] = b0.x; bmin[1] = b0.y; bmin[2] = b0.z;
                                        bmax[0] = b1.x; bmax[1] = b1.y; bmax[2] = b1.z;
                                    });
}

PT_DEV void dfg_entry(const PTShadeDFG* __restrict__ dfg, uint32_t e, float ab[2])
{
    const float2 v = ((const float2*)dfg)[e];
    ab[0] = v.x; ab[1] = v.y;
}

// The fused kernels' lane.  lightmap(i, E): Part 22's lookup of hit i -- true: E is the lightmap's and the volume is not asked; Part
// 21's kernels pass one that finds nothing, which leaves their code as it was.
template <bool PLACED, class Lightmap>
PT_DEV void shade_baked_body(const DScene& S, const PTShadeInputs& A, uint32_t mapTexels, const PTRay* __restrict__ rays, const PTRayHit* __restrict__ hits,
                             const PTRaySurface* __restrict__ surfaces, uint32_t count, float4* __restrict__ out, Lightmap lightmap)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    HitRecords h;
    hit_records(S, rays, hits, surfaces, i, A.dProbes, A.dBoxes, A.probeCount, h);
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!h.miss) {
        float E[4];
        if (!lightmap(i, E)) {
            const auto loadSH = [&](uint32_t probe, float co[27]) { pt_load_probe_sh(A.dSH, probe, co); };
            const auto loadDepth = [&](uint32_t probe, uint32_t texel, float& mean, float& mean2) { pt_load_probe_depth(A.dDepth, probe, texel, mean, mean2); };
            if constexpr (PLACED)
                ptvol::lookup(A.grid, h.P, h.N, loadSH, loadDepth,
                              [&](uint32_t probe, float off[3], uint32_t& state) {
                                  const float4 v = ((const float4*)A.dPlacement)[probe];
                                  off[0] = v.x; off[1] = v.y; off[2] = v.z;
                                  state = pt_asuint(v.w);
                              },
                              E);
            else
                ptvol::lookup(A.grid, h.P, h.N, loadSH, loadDepth, E);
        }
        float spec[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (h.probe < A.probeCount) {
            const float4* map = (const float4*)A.dMaps + (size_t)h.probe * mapTexels;
            const auto load = [&](uint32_t t, float rgb[3]) {
                const float4 v = map[t];
                rgb[0] = v.x; rgb[1] = v.y; rgb[2] = v.z;
            };
            if (A.dBoxes) {
                const float4 pr = ((const float4*)A.dProbes)[h.probe];
                const float4 b0 = ((const float4*)A.dBoxes)[2u * (size_t)h.probe], b1 = ((const float4*)A.dBoxes)[2u * (size_t)h.probe + 1u];
                const float Q[3] = {pr.x, pr.y, pr.z}, bmin[3] = {b0.x, b0.y, b0.z}, bmax[3] = {b1.x, b1.y, b1.z};
                ptrefl::lookup(A.res, A.levels, h.P, h.T.rho, h.R, Q, bmin, bmax, load, spec);
            } else {
                ptrefl::lookup(A.res, A.levels, h.P, h.T.rho, h.R, nullptr, nullptr, nullptr, load, spec);
            }
        }
        float Ad, Bd;
        ptshade::dfg_lookup(A.dfgRes, h.T.nDotV, h.T.rho, [&](uint32_t k, float ab[2]) { dfg_entry(A.dDFG, k, ab); }, Ad, Bd);
        ptshade::compose(h.T, E, spec, Ad, Bd, o);
    }
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
}

} // namespace
