// pt_wf_state.h — how a slot's path state is packed and stored (PTWfBuffers, pt_launch.h): shared by the kernel files that start
// paths in a state set -- pt_wavefront.hip (camera rays, ray lists), pt_gather.hip (irradiance gathers) and pt_probe.hip (SH probes).
#pragma once
#include "pt_device.h"
#include "pt_launch.h"

#define PT_WF_SHARDS 8u         // chunk counters of the persistent trace kernel, one per XCD; the kernel that starts a sequence clears them

// flags word: [1:0] state | [2] hasPending | [4:3] env.valid | [5] light.valid | [6] green | [18:7] sampleIdx | [31:19] depth
// The overlapped state of pt_device.h ("tracing, previous sample's finish pending") is state TRACE + hasPending + depth 0, with
// green and sampleIdx still the previous sample's: no bit and no state code of its own (code 3 stays unused), unambiguous at any
// spp and bounce limit, and ray_exists() reports its three rays as it reports everyone's.
PT_DEV uint32_t pack_flags(const PathRegs& r)
{
    return (r.state & 3u) | ((r.hasPending ? 1u : 0u) << 2) | ((r.env.valid & 3u) << 3) | ((r.light.valid & 1u) << 5) |
           ((r.green ? 1u : 0u) << 6) | ((r.sampleIdx & 0xFFFu) << 7) | ((r.depth & 0x1FFFu) << 19);
}
PT_DEV uint32_t fl_state(uint32_t f) { return f & 3u; }
PT_DEV bool fl_pending(uint32_t f) { return (f >> 2) & 1u; }
PT_DEV uint32_t fl_env(uint32_t f) { return (f >> 3) & 3u; }
PT_DEV uint32_t fl_light(uint32_t f) { return (f >> 5) & 1u; }

PT_DEV float4 f4(v3 v, float w) { return make_float4(v.x, v.y, v.z, w); }
PT_DEV v3 xyz(float4 v) { return mk3(v.x, v.y, v.z); }

// The packed layout of a repacked sequence (PACKED; pt_repack.hip's kernels only): four words ride in lanes that
// are dead everywhere else, and B.rng and B.pthr drop out of the step --
//     rad.w = the RNG state          envC.w = pendThroughput.x          lightC.w = pendThroughput.y          thr.w = pendThroughput.z
// radW: what goes into rad.w.  0 for everyone but pt_wf_init over PTTileMap, whose sequence may be a repacked one: it passes the
// RNG state there as well.  A sequence that does not repack ignores the lane and overwrites it with 0.
PT_DEV void store_path(const PTWfBuffers& B, uint32_t slot, const PathRegs& r, bool writeNee, float radW = 0.0f)
{
    B.flags[slot] = pack_flags(r);
    B.rng[slot] = r.rng;
    B.ray[0][2u * slot] = f4(r.ro, r.scatterPdf);
    B.ray[0][2u * slot + 1u] = f4(r.rd, r.maxRoughness);
    B.rad[slot] = f4(r.radiance, radW);
    B.thr[slot] = f4(r.throughput, 0.0f);
    B.color[slot] = f4(r.color, 0.0f);
    if (writeNee) {
        B.ray[1][2u * slot] = f4(r.neeOrigin, 0.0f);
        B.ray[1][2u * slot + 1u] = f4(r.env.dir, 0.0f);
        B.ray[2][2u * slot] = f4(r.neeOrigin, 0.0f);
        B.ray[2][2u * slot + 1u] = f4(r.light.dir, 0.0f);
        B.envC[slot] = f4(r.env.contribution, 0.0f);
        B.lightC[slot] = f4(r.light.contribution, 0.0f);
        B.pthr[slot] = f4(r.pendThroughput, 0.0f);
    }
}

// per-wave counter rows: one wave owns a row, so a plain read-modify-write is race-free across launches of one stream
template <bool STATS>
PT_DEV void flush_counters(const Counters& cn, unsigned long long* rows, uint32_t row, uint32_t lane)
{
    uint32_t vals[PT_NUM_COUNTERS];
    counters_to_array(cn, vals);
    unsigned long long* p = rows + (size_t)row * 16u;
#pragma unroll
    for (int i = 0; i < PT_NUM_COUNTERS; ++i) {
        if (!STATS && (i >= 3 && i <= 9)) continue;
        if (!STATS && i >= 12) continue;
        if (i == 12) {
            uint32_t m = wave_max_u32(vals[i]);
            if (lane == 0 && m > p[i]) p[i] = m;
        } else {
            uint32_t s = wave_sum_u32(vals[i]);
            if (lane == 0 && s) p[i] += s;
        }
    }
}
