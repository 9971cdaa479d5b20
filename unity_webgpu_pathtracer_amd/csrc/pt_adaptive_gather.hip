// pt_adaptive_gather.hip — adaptive gathers on the MI355X (include/ptmi_plugin.h Part 19): the rule of
// adaptive_gather_rule.h in kernels.  Select: one lane per active entry reads its 4-byte index and, through it, the 16 bytes of
// accumulated irradiance, and decides; the survivors are compacted in the three steps of pt_compact.h -- pt_ag_count (which also
// counts the block's stops by reason), pt_ag_scan (which also sums them), pt_ag_emit (it writes the index and copies the receiver
// as two 16-byte loads and stores).  Fold and equalise are one lane per entry with 16-byte accesses.  No atomics at all, so the
// same input gives the same bytes whatever the launch geometry.
#include "pt_adaptive_gather.h"
#include "pt_compact.h"
#include "adaptive_gather_rule.h"

using namespace ptag;

namespace {

// what step 2 makes of list position k; idx: its entry
__device__ __forceinline__ uint32_t decide(const PTAgSelectArgs& A, uint32_t k, uint32_t& idx)
{
    idx = 0u;
    if (k >= A.activeCount) return kLeftOut;
    idx = A.active ? A.active[k] : k;
    if (idx >= A.entryCount) return kLeftOut;
    const float4 a = A.acc[idx];
    const float e[4] = {a.x, a.y, a.z, a.w};
    const Select s = {A.n, A.addSamples, A.maxSamples, A.threshold2, A.darkFloor};
    return select_entry(s, e);
}

__global__ __launch_bounds__(256) void pt_ag_count(PTAgSelectArgs A, uint32_t blocks)
{
    __shared__ uint32_t waveCount[4][4];
    uint32_t idx;
    const uint32_t r = decide(A, blockIdx.x * 256u + threadIdx.x, idx);
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {                             // column q: the block's entries with decision q
        uint32_t total;
        compact_rank_in_block(r == q, waveCount[q], total);
        if (threadIdx.x == 0u) A.blockCounts[(size_t)blocks * q + blockIdx.x] = total;
    }
}
static_assert(kActive == 0u && kByThreshold == 1u && kByMaxSamples == 2u && kNonFinite == 3u, "the columns of blockCounts and the words of totals");

// The survivor counts become their exclusive prefix; the three stop counts, a stride of `blocks` apart, are only summed, each in
// a walk of its own, one count at a time: four columns in one walk, or two counts at once, and the kernel takes 34 or 25 VGPRs,
// not its 20 (tests/test_adaptive_gather.py).  At most 2^31 / 256 counts: 8,192 per thread.
__global__ __launch_bounds__(1024) void pt_ag_scan(uint32_t* __restrict__ blockCounts, uint32_t blocks, uint64_t* __restrict__ totals)
{
    __shared__ uint32_t waveSum[4][16];
    uint32_t all = compact_scan_blocks(blockCounts, blocks, waveSum[0], [](uint32_t, uint32_t) {});
    if (threadIdx.x == 0u) totals[0] = all;
    for (uint32_t q = 1u; q < 4u; ++q) {
        uint32_t stops = 0u;
#pragma clang loop vectorize(disable)
        for (uint32_t b = threadIdx.x; b < blocks; b += 1024u) stops += blockCounts[(size_t)blocks * q + b];
        compact_scan_threads(stops, waveSum[q], all);
        if (threadIdx.x == 0u) totals[q] = all;
    }
}

__global__ __launch_bounds__(256) void pt_ag_emit(PTAgSelectArgs A)
{
    __shared__ uint32_t waveCount[4];
    uint32_t idx, total;
    const bool kept = decide(A, blockIdx.x * 256u + threadIdx.x, idx) == kActive;
    const uint32_t rank = A.blockCounts[blockIdx.x] + compact_rank_in_block(kept, waveCount, total);
    if (!kept) return;
    if (rank >= A.activeCount) return;                              // cannot happen: the counts are of these very decisions
    const float4 r0 = A.recv[(size_t)idx * 2u], r1 = A.recv[(size_t)idx * 2u + 1u];
    A.outActive[rank] = idx;
    A.outRecv[(size_t)rank * 2u] = r0;
    A.outRecv[(size_t)rank * 2u + 1u] = r1;
}

__global__ __launch_bounds__(256) void pt_ag_fold(const uint32_t* __restrict__ active, uint32_t activeCount, uint32_t entryCount, const float4* __restrict__ fresh,
                                                  uint32_t m, uint32_t n, float4* __restrict__ acc, uint32_t* __restrict__ counts)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= activeCount) return;
    const uint32_t idx = active ? active[k] : k;
    if (idx >= entryCount) return;
    const float4 f = fresh[k];
    if (n == 0u) {
        acc[idx] = f;
    } else {
        const float4 a = acc[idx];
        float e[4] = {a.x, a.y, a.z, a.w};
        const float g[4] = {f.x, f.y, f.z, f.w};
        fold_entry(e, n, g, m);
        acc[idx] = make_float4(e[0], e[1], e[2], e[3]);
    }
    if (counts) counts[idx] = n + m;
}

__global__ __launch_bounds__(256) void pt_ag_equalise(const float4* irr, const uint32_t* __restrict__ counts, uint32_t count, uint32_t samplesEq, float4* out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    float4 a = irr[i];
    const float e[4] = {a.x, a.y, a.z, a.w};
    float m2;
    if (equalise_entry(e, counts[i], samplesEq, m2)) a.w = m2;
    out[i] = a;
}

} // namespace

size_t pt_ag_blocks(uint64_t activeCount) { return (size_t)((activeCount + 255u) / 256u); }

hipError_t pt_launch_ag_select(const PTAgSelectArgs& A, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)pt_ag_blocks(A.activeCount);
    hipLaunchKernelGGL(pt_ag_count, dim3(blocks), dim3(256), 0, stream, A, blocks);
    hipLaunchKernelGGL(pt_ag_scan, dim3(1), dim3(1024), 0, stream, A.blockCounts, blocks, A.totals);
    hipLaunchKernelGGL(pt_ag_emit, dim3(blocks), dim3(256), 0, stream, A);
    return hipGetLastError();
}

hipError_t pt_launch_ag_fold(const uint32_t* active, uint32_t activeCount, uint32_t entryCount, const PTIrradiance* fresh, uint32_t m, uint32_t n,
                             PTIrradiance* acc, uint32_t* counts, hipStream_t stream)
{
    hipLaunchKernelGGL(pt_ag_fold, dim3((uint32_t)pt_ag_blocks(activeCount)), dim3(256), 0, stream, active, activeCount, entryCount, (const float4*)fresh, m, n,
                       (float4*)acc, counts);
    return hipGetLastError();
}

hipError_t pt_launch_ag_equalise(const PTIrradiance* irr, const uint32_t* counts, uint32_t count, uint32_t samplesEq, PTIrradiance* out, hipStream_t stream)
{
    hipLaunchKernelGGL(pt_ag_equalise, dim3((uint32_t)pt_ag_blocks(count)), dim3(256), 0, stream, (const float4*)irr, counts, count, samplesEq, (float4*)out);
    return hipGetLastError();
}
