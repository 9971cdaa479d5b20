// pt_query.hip — batched ray queries (include/ptmi_plugin.h Part 3: PTTraceRays / PTTraceRaysHost).
//
// One ray per lane, 64-lane waves, one wave per workgroup.  The grid is capped at the waves the device keeps resident for
// the kernel (occupancy x CUs, pt_query_grid_caps); each wave walks the batch in 64-ray chunks, grid-stride, so a ray's
// result lands in hits[i] for rays[i] and nothing is sorted.  Rays are read as two float4 and hits written as one float4
// (surface records as three), all coalesced across the wave.
//
// The traversal is the render's own device code (pt_device.h): traverse_cwbvh / traverse_tlas, fetch_hit_attributes /
// fetch_hit_attributes_tlas.  A query therefore returns the bits the render's walk would, and counts the same nodeVisits,
// triTests, ... (STATS instantiations).  The CWBVH stack keeps PT_Q_LDS_STACK entries per lane in LDS ([entry][lane]); deeper
// entries go to a slab in HBM (one row of 32 - PT_Q_LDS_STACK entries per resident lane, owned by the context), addressed
// through spill_row on the wave index held in LDS -- no private array, so the CWBVH kernels have no scratch.  The HAS_TLAS
// kernels keep traverse_tlas's private 32-entry TLAS stack (scratch, see DESIGN.md "Ray queries").
#include "pt_device.h"
#include "pt_launch.h"

namespace {

enum : uint32_t { Q_CLOSEST = 0u, Q_ANY_HIT = 1u, Q_SURFACE = 2u };

template <uint32_t MODE, bool STATS, bool TLAS>
PT_DEV void query_body(const DScene& S, const float4* __restrict__ rays, uint32_t count, float4* __restrict__ hits,
                       float4* __restrict__ surface, uint2* __restrict__ slab, unsigned long long* __restrict__ gstats)
{
    const uint32_t lane = threadIdx.x;
    Counters cn = {};
    TravStackT<PT_Q_LDS_STACK, true> st;
    resident_wave_stack(st, slab);

    for (uint32_t base = blockIdx.x * 64u; base < count; base += gridDim.x * 64u) {
        const uint32_t i = base + lane;
        if (i >= count) break;
        const float4 r0 = rays[(size_t)i * 2], r1 = rays[(size_t)i * 2 + 1];
        const v3 o = mk3(r0.x, r0.y, r0.z), d = mk3(r0.w, r1.x, r1.y);
        const float tmax = r1.z;
        if (STATS) { if (MODE == Q_ANY_HIT) cn.shadowRays++; else cn.closestRays++; }
        // tmax NaN or <= 0: a miss by definition, no walk (the comparison is false for NaN)
        const bool walk = tmax > 0.0f;
        HitRecord rec = miss_record(tmax);
        bool found = false;
        if (walk) {
            if (TLAS) {
                traverse_tlas<STATS>(S, o, d, MODE == Q_ANY_HIT, rec, st, cn);
                // closest: an instance that improved the hit records itself; any-hit: the walk ends at the first accepted triangle
                found = MODE == Q_ANY_HIT ? rec.h.t < tmax : rec.inst != 0xFFFFFFFFu;
            } else {
                traverse_cwbvh<STATS>(S, o, d, MODE == Q_ANY_HIT, rec.h, st, cn, tmax);
                found = rec.h.t < tmax;
            }
        }
        hits[i] = make_float4(rec.h.t, rec.h.u, rec.h.v, pt_asfloat(rec.h.triIndex));
        if (MODE == Q_SURFACE && found) {
            SurfHit sh;
            if (TLAS) fetch_hit_attributes_tlas(S, d, rec, sh);
            else fetch_hit_attributes<STATS>(S, o, d, rec.h, sh, cn);
            float4* sp = surface + (size_t)i * 3;
            sp[0] = make_float4(sh.position.x, sh.position.y, sh.position.z, sh.distance);
            sp[1] = make_float4(sh.normal.x, sh.normal.y, sh.normal.z, pt_asfloat((uint32_t)sh.materialIndex));
            sp[2] = make_float4(sh.uv.x, sh.uv.y, pt_asfloat(rec.inst), pt_asfloat(sh.triIndex));
        }
    }

    if (STATS) {                                                        // one atomic per wave per counter
        uint32_t vals[PT_NUM_COUNTERS];
        counters_to_array(cn, vals);
#pragma unroll
        for (int k = 1; k < PT_NUM_COUNTERS; ++k) {
            if (k >= 6 && k <= 11) continue;                            // shading / frame counters: never touched by a query
            if (k == 12) {
                const uint32_t m = wave_max_u32(vals[k]);
                if (lane == 0u && m) atomicMax(&gstats[k], (unsigned long long)m);
            } else {
                const uint32_t s = wave_sum_u32(vals[k]);
                if (lane == 0u && s) atomicAdd(&gstats[k], (unsigned long long)s);
            }
        }
    }
}

} // namespace

// Stable, unmangled kernel names (rocprofv3 --kernel-trace lists them as they are written here).
#define PT_Q_KERNEL(name, MODE, STATS, TLAS)                                                                                    \
    extern "C" __global__ __launch_bounds__(64) void name(DScene S, const float4* __restrict__ rays, uint32_t count,            \
                                                          float4* __restrict__ hits, float4* __restrict__ surface,             \
                                                          uint2* __restrict__ slab, unsigned long long* __restrict__ gstats)   \
    {                                                                                                                           \
        query_body<MODE, STATS, TLAS>(S, rays, count, hits, surface, slab, gstats);                                            \
    }
PT_Q_KERNEL(pt_query_closest, Q_CLOSEST, false, false)
PT_Q_KERNEL(pt_query_closest_stats, Q_CLOSEST, true, false)
PT_Q_KERNEL(pt_query_anyhit, Q_ANY_HIT, false, false)
PT_Q_KERNEL(pt_query_anyhit_stats, Q_ANY_HIT, true, false)
PT_Q_KERNEL(pt_query_surface, Q_SURFACE, false, false)
PT_Q_KERNEL(pt_query_surface_stats, Q_SURFACE, true, false)
PT_Q_KERNEL(pt_query_tlas_closest, Q_CLOSEST, false, true)
PT_Q_KERNEL(pt_query_tlas_closest_stats, Q_CLOSEST, true, true)
PT_Q_KERNEL(pt_query_tlas_anyhit, Q_ANY_HIT, false, true)
PT_Q_KERNEL(pt_query_tlas_anyhit_stats, Q_ANY_HIT, true, true)
PT_Q_KERNEL(pt_query_tlas_surface, Q_SURFACE, false, true)
PT_Q_KERNEL(pt_query_tlas_surface_stats, Q_SURFACE, true, true)
#undef PT_Q_KERNEL

namespace {
typedef void (*QueryKernel)(DScene, const float4*, uint32_t, float4*, float4*, uint2*, unsigned long long*);
// index = (tlas * 3 + mode) * 2 + stats
const QueryKernel kQueryKernels[PT_QUERY_KERNELS] = {
    pt_query_closest, pt_query_closest_stats, pt_query_anyhit, pt_query_anyhit_stats, pt_query_surface, pt_query_surface_stats,
    pt_query_tlas_closest, pt_query_tlas_closest_stats, pt_query_tlas_anyhit, pt_query_tlas_anyhit_stats,
    pt_query_tlas_surface, pt_query_tlas_surface_stats,
};
} // namespace

size_t pt_resident_wave_slab_bytes() { return (size_t)64 * PT_Q_SLAB_ENTRIES * sizeof(uint2); }

hipError_t pt_query_grid_caps(int device, uint32_t caps[PT_QUERY_KERNELS])
{
    return pt_resident_wave_caps(device, kQueryKernels, PT_QUERY_KERNELS, caps);
}

hipError_t pt_launch_query(const DScene& S, const float4* rays, uint32_t count, uint32_t mode, bool stats, float4* hits,
                           float4* surface, uint2* slab, uint32_t gridCap, unsigned long long* gstats, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    const QueryKernel k = kQueryKernels[pt_query_kernel_index(S.hasTlas != 0u, mode, stats)];
    const uint32_t chunks = (count + 63u) / 64u;
    const uint32_t grid = chunks < gridCap ? chunks : gridCap;
    hipLaunchKernelGGL(k, dim3(grid), dim3(64), 0, stream, S, rays, count, hits, surface, slab, gstats);
    return hipGetLastError();
}
