// pt_compact.h — the device side of a stable stream compaction in three launches, written once for the lightmap
// charts (pt_lightmap.hip), the adaptive gather's select (pt_adaptive_gather.hip) and the mid-pass slot repack (pt_repack.hip):
//     count   one workgroup of 256 per block of 256 entries: the block's kept entries      compact_rank_in_block (its total)
//     scan    one workgroup of 1024: the block counts become their exclusive prefix        compact_scan_blocks
//     emit    the same workgroups as count: entry -> prefix[block] + its rank in the block  compact_rank_in_block (its rank)
// One form for the block step: the count kernels take the total from the very function that ranks the lanes in the emit kernels,
// so what is counted is what is ranked.  No atomics: the same input gives the same order, whatever the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// number of set bits of a wave mask below this lane (v_mbcnt: no per-lane 64-bit "lanes below me" mask to keep in registers)
__device__ __forceinline__ uint32_t rank_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Rank of the lane among the lanes of its 256-thread block whose `kept` is true, and their number.  Every lane of the block calls
// it (it holds a barrier); s_wave: four words of LDS that the block does not touch until its next barrier.
__device__ __forceinline__ uint32_t compact_rank_in_block(bool kept, uint32_t* s_wave, uint32_t& total)
{
    const unsigned long long m = __ballot(kept);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) s_wave[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t i = 0; i < 4u; ++i) if (i < w) before += s_wave[i];
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return before + rank_below(m);
}

// inclusive prefix sum of v over the lanes of a wave
__device__ __forceinline__ uint32_t compact_scan_wave(uint32_t v)
{
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if ((threadIdx.x & 63u) >= off) v += o;
    }
    return v;
}

// Exclusive prefix sum of v over the 1024 threads of a workgroup, and the sum (below 2^32) to every thread.  All threads call it
// (it holds a barrier); s_sum: sixteen words of LDS.  Every wave scans the sixteen wave sums the way it scanned its own values,
// one sum per lane: with sixteen words in the registers of every lane, or the lane constants of a scan of another width,
// pt_ag_scan does not keep its 20 VGPRs (tests/test_adaptive_gather.py).
__device__ __forceinline__ uint32_t compact_scan_threads(uint32_t v, uint32_t* s_sum, uint32_t& all)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t incl = compact_scan_wave(v);
    if (lane == 63u) s_sum[w] = incl;
    __syncthreads();
    const uint32_t mine = lane < 16u ? s_sum[lane] : 0u;
    const uint32_t upto = compact_scan_wave(mine);                  // lane i < 16: waves 0 .. i; the other lanes: all of them
    all = (uint32_t)__builtin_amdgcn_readlane((int)upto, 63);
    return (uint32_t)__builtin_amdgcn_readlane((int)(upto - mine), __builtin_amdgcn_readfirstlane((int)w)) + incl - v;
}

// counts[0, blocks) becomes its exclusive prefix; every thread gets the total.  The 1024 threads of the one workgroup call it, as
// they call compact_scan_threads.  Thread t owns the run of ceil(blocks / 1024) consecutive counts from t times that number,
// clamped to `blocks` at both ends: past the last count a thread owns nothing.  It sums its run -- first(block, count) sees every
// count of the run there, before any is rewritten --, and walks it again from where the runs before it end.  blocks <= 2^23, so
// that a run's start fits 32 bits.
template <class First>
__device__ __forceinline__ uint32_t compact_scan_blocks(uint32_t* __restrict__ counts, uint32_t blocks, uint32_t* s_sum, First first)
{
    const uint32_t per = (blocks + 1023u) / 1024u;
    const uint32_t lo = threadIdx.x * per < blocks ? threadIdx.x * per : blocks, hi = lo + per < blocks ? lo + per : blocks;
    uint32_t sum = 0u, all;
    for (uint32_t b = lo; b < hi; ++b) { const uint32_t c = counts[b]; sum += c; first(b, c); }
    uint32_t running = compact_scan_threads(sum, s_sum, all);
    for (uint32_t b = lo; b < hi; ++b) {
        const uint32_t c = counts[b];
        counts[b] = running;
        running += c;
    }
    return all;
}
