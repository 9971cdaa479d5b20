// pt_probe.hip — SH light probes (include/ptmi_plugin.h Part 15): the two kernels that turn the ray list's launch
// sequence (pt_wavefront.hip) into probes x samples, and the kernels of PTProbeRays, of the delta lights and of PTProbeIrradiance.
//
//     pt_wf_probe_init       one lane per slot = (probe, sample): the sphere direction, then the state a radiance query starts
//                            the ray {P, w} with
//     [ trace ; shade ] ...  the PTRayMap instantiations of pt_wavefront.hip, unchanged, one sample per slot
//     pt_wf_probe_resolve    one WAVE per probe: lane l projects the samples j = l (mod 64) onto the nine basis functions -- a
//                            contiguous 1 KB of colours per load --, an xor butterfly folds the 28 sums, the delta lights are added
//
// The arithmetic is sh_rule.h's, which the host twins evaluate too; a direction is made from the seed wherever it is needed.
#include "pt_device.h"
#include "pt_launch.h"
#include "pt_wf_state.h"
#include "sh_rule.h"

namespace {

// {position.xyz, seed}: one 16-byte load.  Neighbouring lanes read the same probe (entry-major slots)
struct Probe { v3 P; uint32_t seed; };
PT_DEV Probe load_probe(const PTProbe* probes, uint32_t entry)
{
    const float4 a = ((const float4*)probes)[entry];
    return {mk3(a.x, a.y, a.z), pt_asuint(a.w)};
}

// entry and sample of a slot; false: the slot is past the end
PT_DEV bool probe_slot(const PTProbeMap& pm, uint32_t slot, uint32_t& entry, uint32_t& sample)
{
    entry = slot / pm.samples;
    sample = slot - entry * pm.samples;
    return entry < pm.entries;
}

// the direction of sample j (counted from firstSample) and the RNG state its path starts with
PT_DEV v3 probe_direction(const PTProbeMap& pm, uint32_t seed, uint32_t j, uint32_t& rng)
{
    rng = ptsh::sample_rng(seed, pm.firstSample, j);
    float w[3];
    ptsh::direction(rng, w);
    return mk3(w[0], w[1], w[2]);
}

// The state ray_path_init (pt_wavefront.hip) leaves for the list entry {P, w, rng}: depth 0, nothing pending, no NEE.
PT_DEV void probe_path_init(v3 P, v3 w, uint32_t rng, PathRegs& r, Counters& cn)
{
    r.rng = rng;
    r.sampleIdx = 0u;
    r.color = mk3(0.0f);
    r.env.valid = 0u; r.light.valid = 0u;
    r.env.dir = mk3(0.0f); r.light.dir = mk3(0.0f);
    r.env.contribution = mk3(0.0f); r.light.contribution = mk3(0.0f);
    r.neeOrigin = mk3(0.0f); r.pendThroughput = mk3(0.0f);
    r.hasPending = false; r.green = false;
    path_reset_sample(r);
    cn.paths++;
    r.scatterPdf = 0.0f;
    r.maxRoughness = 0.0f;
    r.ro = P;
    r.rd = w;
    r.state = PS_TRACE;
}

__global__ __launch_bounds__(256) void pt_wf_probe_init(PTProbeMap pm, PTWfBuffers B)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0u && threadIdx.x < PT_WF_SHARDS) B.chunkHeads[threadIdx.x * 32u] = 0u;
    if (slot >= B.numSlots) return;
    uint32_t entry, sample;
    Counters cn = {};
    if (!probe_slot(pm, slot, entry, sample)) B.flags[slot] = PS_DONE;
    else {
        const Probe pr = load_probe(pm.probes, entry);
        uint32_t rng;
        const v3 w = probe_direction(pm, pr.seed, sample, rng);
        PathRegs r;
        probe_path_init(pr.P, w, rng, r, cn);
        store_path(B, slot, r, false);
    }
    // every lane of the wave takes part in the reduction (numSlots is a multiple of 256: no lane has returned)
    flush_counters<false>(cn, B.statRows, blockIdx.x * 4u + (threadIdx.x >> 6), threadIdx.x & 63u);
}

// PTProbeRays: the same ray and RNG state into the caller's array
__global__ __launch_bounds__(256) void pt_wf_probe_rays(PTProbeMap pm, PTRadianceRay* __restrict__ rays)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t entry, sample;
    if (!probe_slot(pm, slot, entry, sample)) return;
    const Probe pr = load_probe(pm.probes, entry);
    uint32_t rng;
    const v3 w = probe_direction(pm, pr.seed, sample, rng);
    float4* e = (float4*)(rays + slot);
    e[0] = make_float4(pr.P.x, pr.P.y, pr.P.z, w.x);
    e[1] = make_float4(w.y, w.z, pt_asfloat(rng), pt_asfloat(0u));
}

// One wave per probe, four probes per workgroup.  The 28 sums stay in registers (every loop over them is unrolled); the butterfly
// leaves the tree's value in every lane, so lanes 0 to 6 can each store one 16-byte row of the record.
__global__ __launch_bounds__(256) void pt_wf_probe_resolve(PTProbeMap pm, PTWfBuffers B, PTProbeCoeffs* __restrict__ out)
{
    const uint32_t entry = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (entry >= pm.entries) return;                             // the whole wave
    const Probe pr = load_probe(pm.probes, entry);
    const float4* c = B.color + (size_t)entry * pm.samples;
    float acc[ptsh::kSums];
#pragma unroll
    for (uint32_t t = 0; t < ptsh::kSums; ++t) acc[t] = 0.0f;
    for (uint32_t j = lane; j < pm.samples; j += ptsh::kLanes) {
        const float4 cj = c[j];
        uint32_t rng;
        const v3 w = probe_direction(pm, pr.seed, j, rng);
        const float L[3] = {cj.x, cj.y, cj.z}, wv[3] = {w.x, w.y, w.z};
        ptsh::accumulate(acc, L, wv);
    }
#pragma unroll
    for (uint32_t h = 32u; h >= 1u; h >>= 1) {
#pragma unroll
        for (uint32_t t = 0; t < ptsh::kSums; ++t) acc[t] = acc[t] + __shfl_xor(acc[t], (int)h, 64);
    }
#pragma unroll
    for (uint32_t t = 0; t < 27u; ++t) acc[t] = ptsh::scale(acc[t], pm.samples);
    // the delta lights of this probe, in ascending light index (wave-uniform reads)
    for (uint32_t l = 0; l < pm.lightCount; ++l) {
        const size_t pair = (size_t)entry * pm.lightCount + l;
        const float4 r0 = pm.deltaRays[2u * pair], r1 = pm.deltaRays[2u * pair + 1u];
        const float4 hit = pm.deltaHits[pair];
        if (!(r1.z > 0.0f) || pt_asuint(hit.w) != 0xFFFFFFFFu) continue;          // skipped (tmax = 0), or occluded
        const float4 li = pm.deltaLi[pair];
        const float Li[3] = {li.x, li.y, li.z}, dir[3] = {r0.w, r1.x, r1.y};
        ptsh::add_delta(acc, Li, dir);
    }
    float4* o = (float4*)(out + entry);
#pragma unroll
    for (uint32_t t = 0; t < 7u; ++t)
        if (lane == t) o[t] = make_float4(acc[4u * t], acc[4u * t + 1u], acc[4u * t + 2u], acc[4u * t + 3u]);
}

// lsDirection, lsDistance and Li of a point or spot light at scatterPos = P: the POINT / SPOT branches and the EvalLight block of
// nee_prepare_light (pt_device.h), restated -- that function's kernels are not touched.  false: another light type
PT_DEV bool probe_light_sample(const DLight& light, float4 lcNN, v3 P, v3& lsDirection, float& lsDistance, v3& Li)
{
    if (light.type == PT_LIGHT_TYPE_SPOT) {
        lsDirection = -normalize3(P - light.position);
        lsDistance = length3(light.position - P);
    } else if (light.type == PT_LIGHT_TYPE_POINT) {
        const v3 lsNormal = normalize3(P - light.position);
        lsDirection = -lsNormal;
        lsDistance = length3(P - light.position);
    } else {
        return false;
    }
    // EvalLight
    float falloff = 1.0f;
    if (lsDistance > light.range) falloff = 0.0f;
    else {
        float r = lsDistance / light.range;
        float atten = pt_saturate(1.0f / (1.0f + 25.0f * r * r) * pt_saturate((1.0f - r) * 5.0f));
        falloff *= atten;
    }
    if (light.type == PT_LIGHT_TYPE_SPOT) {
        const v3 lsNormalN = mk3(lcNN.x, lcNN.y, lcNN.z);        // normalize(normalize(light.u))
        float cosTheta = dot3(normalize3(-lsDirection), lsNormalN);
        if (cosTheta < light.v.x) falloff = 0.0f;
        else if (cosTheta > light.v.x && cosTheta < light.v.y) falloff *= (cosTheta - light.v.x) / (light.v.y - light.v.x);
    }
    Li = light.emission * falloff;
    return true;
}

// one lane per (probe, light) pair: the any-hit ray and Li.  Another light type or an all-zero Li: tmax = 0 (Part 3: a miss
// without a walk), which the resolve skips
__global__ __launch_bounds__(256) void pt_probe_delta_rays(DScene S, const PTProbe* __restrict__ probes, uint32_t pairs, float4* __restrict__ rays,
                                                           float4* __restrict__ li)
{
    const uint32_t pair = blockIdx.x * 256u + threadIdx.x;
    if (pair >= pairs) return;
    const uint32_t lightCount = (uint32_t)S.lightCount;
    const uint32_t entry = pair / lightCount, l = pair - entry * lightCount;
    const Probe pr = load_probe(probes, entry);
    const DLight light = load_light(S, (int)l);
    const float4 lcNN = S.lightConst[(size_t)l * 4 + 3];
    v3 dir = mk3(0.0f), Li = mk3(0.0f);
    float dist = 0.0f, tmax = 0.0f;
    if (probe_light_sample(light, lcNN, pr.P, dir, dist, Li) && (Li.x != 0.0f || Li.y != 0.0f || Li.z != 0.0f)) tmax = PT_FAR_PLANE;
    else { dir = mk3(0.0f); Li = mk3(0.0f); }
    rays[2u * pair] = make_float4(pr.P.x, pr.P.y, pr.P.z, dir.x);
    rays[2u * pair + 1u] = make_float4(dir.y, dir.z, tmax, pt_asfloat(0u));
    li[pair] = make_float4(Li.x, Li.y, Li.z, 0.0f);
}

// one lane per query {normal, probe}: E(N) of that probe's coefficients; a probe index past the array gives zeros and reads nothing
__global__ __launch_bounds__(256) void pt_probe_irradiance(const PTProbeCoeffs* __restrict__ sh, uint64_t probeCount, const PTProbeQuery* __restrict__ queries,
                                                           uint32_t count, PTIrradiance* __restrict__ out)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= count) return;
    const float4 qu = ((const float4*)queries)[q];
    const uint32_t probe = pt_asuint(qu.w);
    float E[3] = {0.0f, 0.0f, 0.0f};
    if (probe < probeCount) {
        const float4* s = (const float4*)(sh + probe);
        float co[28];
#pragma unroll
        for (uint32_t t = 0; t < 7u; ++t) {
            const float4 v = s[t];
            co[4u * t] = v.x; co[4u * t + 1u] = v.y; co[4u * t + 2u] = v.z; co[4u * t + 3u] = v.w;
        }
        const float N[3] = {qu.x, qu.y, qu.z};
        ptsh::irradiance(co, N, E);
    }
    ((float4*)out)[q] = make_float4(E[0], E[1], E[2], 0.0f);
}

bool probe_map_fits(const PTProbeMap& pm, const PTWfBuffers& B) { return pm.samples != 0u && (uint64_t)pm.entries * pm.samples <= B.numSlots; }

} // namespace

hipError_t pt_launch_probe_init(const PTProbeMap& pm, const PTWfBuffers& B, hipStream_t stream)
{
    if (!probe_map_fits(pm, B)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_wf_probe_init, dim3(B.numSlots >> 8), dim3(256), 0, stream, pm, B);
    return hipGetLastError();
}

hipError_t pt_launch_probe_resolve(const PTProbeMap& pm, const PTWfBuffers& B, PTProbeCoeffs* out, hipStream_t stream)
{
    if (!probe_map_fits(pm, B)) return hipErrorInvalidValue;
    if (pm.lightCount && (!pm.deltaRays || !pm.deltaLi || !pm.deltaHits)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_wf_probe_resolve, dim3((pm.entries + 3u) / 4u), dim3(256), 0, stream, pm, B, out);
    return hipGetLastError();
}

hipError_t pt_launch_probe_rays(const PTProbeMap& pm, PTRadianceRay* rays, hipStream_t stream)
{
    const uint64_t slots = (uint64_t)pm.entries * pm.samples;
    if (pm.samples == 0u || slots > (1ull << 31)) return hipErrorInvalidValue;
    if (slots == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_wf_probe_rays, dim3((uint32_t)((slots + 255u) / 256u)), dim3(256), 0, stream, pm, rays);
    return hipGetLastError();
}

hipError_t pt_launch_probe_delta_rays(const DScene& S, const PTProbe* probes, uint32_t entries, float4* rays, float4* li, hipStream_t stream)
{
    const uint64_t pairs = (uint64_t)entries * (uint64_t)(S.lightCount > 0 ? S.lightCount : 0);
    if (pairs > (1ull << 28)) return hipErrorInvalidValue;
    if (pairs == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_probe_delta_rays, dim3((uint32_t)((pairs + 255u) / 256u)), dim3(256), 0, stream, S, probes, (uint32_t)pairs, rays, li);
    return hipGetLastError();
}

hipError_t pt_launch_probe_irradiance(const PTProbeCoeffs* sh, uint64_t probeCount, const PTProbeQuery* queries, uint32_t count, PTIrradiance* out,
                                      hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_probe_irradiance, dim3((count + 255u) / 256u), dim3(256), 0, stream, sh, probeCount, queries, count, out);
    return hipGetLastError();
}
