// pt_gather.hip — irradiance gathers (include/ptmi_plugin.h Part 13): the two kernels that turn the ray list's
// launch sequence (pt_wavefront.hip) into a gather over receivers x samples, and the kernel of PTGatherRays.
//
//     pt_wf_gather_init      one lane per slot = (entry, sample): the receiver step -- both NEE preparations with a Lambert BSDF
//                            and the cosine-weighted gather direction -- into the slot's full path state
//     [ trace ; shade ] ...  the PTRayMap instantiations of pt_wavefront.hip, unchanged, one sample per slot
//     pt_wf_gather_resolve   one lane per entry: E = PI x the mean of its samples' radiance, and the luminance moment
//
// The receiver step is written once (receiver_step) from the device functions the render's material branch calls, so every draw,
// the light pick and the EvalLight arithmetic are the render's; only the BSDF differs (LambertBsdf, pt_device.h).
#include "pt_device.h"
#include "pt_launch.h"
#include "pt_wf_state.h"

namespace {

// The receiver of slot s: two 16-byte loads {position.xyz, seed} {normal.xyz, reserved}.  Neighbouring lanes read the same entry
// (entry-major slots): a wave touches at most two records when samples >= 64.
struct Receiver { v3 P, N; uint32_t seed; };
PT_DEV Receiver load_receiver(const PTReceiver* recv, uint32_t entry)
{
    const float4* e = (const float4*)(recv + entry);
    const float4 a = e[0], b = e[1];
    return {mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), pt_asuint(a.w)};
}

// The receiver step (ptmi_plugin.h Part 13), in the order of path_shade_hit's material branch: NEE origin, environment NEE, light
// NEE, then the scatter direction -- cosine-weighted, two draws -- in place of sample_brdf.  Leaves the complete state of a path
// that has just shaded its first bounce: depth 1, the receiver's NEE pending with throughput 1, radiance 0.
template <bool STATS>
PT_DEV void receiver_step(const DScene& S, const PTFrameParams& P, const Receiver& rc, uint32_t sample, PathRegs& r, Counters& cn)
{
    uint32_t s = rc.seed;
    pt_rng_next(&s);
    r.rng = s + sample;
    r.sampleIdx = 0u;
    r.color = mk3(0.0f);
    r.green = false;
    r.radiance = mk3(0.0f);
    r.throughput = mk3(1.0f);
    cn.paths++;

    SurfHit hit;
    hit.distance = 0.0f;
    hit.isLight = 0u;
    hit.triIndex = 0u;
    hit.materialIndex = 0;
    hit.uv = {0.0f, 0.0f};
    hit.position = rc.P;
    hit.normal = rc.N;
    hit.ffnormal = rc.N;
    const Material noMaterial = {};              // the Lambert term reads neither the material nor the tints
    const BsdfShared noTints = {};
    const v3 rayDir = -rc.N;                     // V = N: read by no term of the Lambert BSDF
    const LambertBsdf lambert = {rc.N};

    r.neeOrigin = nee_scatter_pos(hit);
    const Onb onb = make_onb(hit.ffnormal);
    nee_prepare_environment(S, P, rayDir, hit, noMaterial, r.rng, r.env, noTints, onb, lambert);
    nee_prepare_light<STATS>(S, rayDir, hit, noMaterial, r.neeOrigin, r.rng, r.light, cn, noTints, onb, lambert);
    // (a NEE ray that is not valid leaves its direction unset in the render, where nobody reads it; here it is stored)
    if (r.env.valid == 0u) r.env.dir = mk3(0.0f);
    if (r.light.valid == 0u) r.light.dir = mk3(0.0f);
    r.pendThroughput = r.throughput;
    r.hasPending = true;

    const float r1 = rnd(r.rng);
    const float r2 = rnd(r.rng);
    const v3 local = cosine_sample_hemisphere(r1, r2);
    const v3 L = onb_to_world(onb, local);
    const float pdf = local.z / PT_PI;
    r.scatterPdf = pdf;
    r.maxRoughness = 1.0f;
    r.depth = 1u;
    r.rd = L;
    r.ro = hit.position + r.rd * PT_EPSILON;
    r.state = pdf > 0.0f ? PS_TRACE : PS_ENDING;       // throughput stays (1, 1, 1): f / pdf of the Lambert term, never divided out
}

// entry and sample of a slot; false: the slot is past the end
PT_DEV bool gather_slot(const PTGatherMap& gm, uint32_t slot, uint32_t& entry, uint32_t& sample)
{
    entry = slot / gm.samples;
    sample = gm.firstSample + (slot - entry * gm.samples);
    return entry < gm.entries;
}

template <bool STATS>
__global__ __launch_bounds__(256) void pt_wf_gather_init(DScene S, PTFrameParams P, PTGatherMap gm, PTWfBuffers B)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0u && threadIdx.x < PT_WF_SHARDS) B.chunkHeads[threadIdx.x * 32u] = 0u;
    if (slot >= B.numSlots) return;
    uint32_t entry, sample;
    Counters cn = {};
    if (!gather_slot(gm, slot, entry, sample)) B.flags[slot] = PS_DONE;
    else {
        PathRegs r;
        receiver_step<STATS>(S, P, load_receiver(gm.recv, entry), sample, r, cn);
        store_path(B, slot, r, true);
    }
    // every lane of the wave takes part in the reduction (numSlots is a multiple of 256: no lane has returned)
    flush_counters<STATS>(cn, B.statRows, blockIdx.x * 4u + (threadIdx.x >> 6), threadIdx.x & 63u);
}

// PTGatherRays: the same body, the ray and the RNG state into the caller's array instead of a state set
__global__ __launch_bounds__(256) void pt_wf_gather_rays(DScene S, PTFrameParams P, PTGatherMap gm, PTRadianceRay* __restrict__ rays)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t entry, sample;
    if (!gather_slot(gm, slot, entry, sample)) return;
    PathRegs r;
    Counters cn = {};
    receiver_step<false>(S, P, load_receiver(gm.recv, entry), sample, r, cn);
    if (r.state != PS_TRACE) r.rd = mk3(pt_asfloat(0x7FC00000u));                // the sample ended at the receiver
    float4* e = (float4*)(rays + slot);
    e[0] = make_float4(r.ro.x, r.ro.y, r.ro.z, r.rd.x);
    e[1] = make_float4(r.rd.y, r.rd.z, pt_asfloat(r.rng), pt_asfloat(0u));
}

// One lane per entry: its samples' colours in ascending order.  e_j = c_j * PI, rgb = sum / (float)samples, m2 = sum of lum(e_j)^2.
__global__ __launch_bounds__(256) void pt_wf_gather_resolve(PTGatherMap gm, PTWfBuffers B, PTIrradiance* __restrict__ out)
{
    const uint32_t entry = blockIdx.x * 256u + threadIdx.x;
    if (entry >= gm.entries) return;
    const float4* c = B.color + (size_t)entry * gm.samples;
    v3 sum = mk3(0.0f);
    float m2 = 0.0f;
    for (uint32_t j = 0; j < gm.samples; ++j) {
        const v3 e = xyz(c[j]) * PT_PI;
        sum = sum + e;
        const float lum = luminance3(e);
        m2 = m2 + lum * lum;
    }
    const v3 mean = sum / (float)gm.samples;
    ((float4*)out)[entry] = make_float4(mean.x, mean.y, mean.z, m2);
}

} // namespace

hipError_t pt_launch_gather_init(const DScene& S, const PTFrameParams& P, const PTGatherMap& gm, const PTWfBuffers& B, bool fullStats, hipStream_t stream)
{
    if (gm.samples == 0u || (uint64_t)gm.entries * gm.samples > B.numSlots) return hipErrorInvalidValue;
    const dim3 grid(B.numSlots >> 8), block(256);
    if (fullStats) hipLaunchKernelGGL(pt_wf_gather_init<true>, grid, block, 0, stream, S, P, gm, B);
    else hipLaunchKernelGGL(pt_wf_gather_init<false>, grid, block, 0, stream, S, P, gm, B);
    return hipGetLastError();
}

hipError_t pt_launch_gather_resolve(const PTGatherMap& gm, const PTWfBuffers& B, PTIrradiance* out, hipStream_t stream)
{
    if (gm.samples == 0u || (uint64_t)gm.entries * gm.samples > B.numSlots) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_wf_gather_resolve, dim3((gm.entries + 255u) / 256u), dim3(256), 0, stream, gm, B, out);
    return hipGetLastError();
}

hipError_t pt_launch_gather_rays(const DScene& S, const PTFrameParams& P, const PTGatherMap& gm, PTRadianceRay* rays, hipStream_t stream)
{
    const uint64_t slots = (uint64_t)gm.entries * gm.samples;
    if (gm.samples == 0u || slots > (1ull << 31)) return hipErrorInvalidValue;
    if (slots == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_wf_gather_rays, dim3((uint32_t)((slots + 255u) / 256u)), dim3(256), 0, stream, S, P, gm, rays);
    return hipGetLastError();
}
