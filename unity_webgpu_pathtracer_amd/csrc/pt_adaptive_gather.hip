// pt_adaptive_gather.hip — adaptive gathers on the MI355X (include/ptmi_plugin.h Part 19): the rule of
// adaptive_gather_rule.h in kernels.  Select: one lane per active entry reads its 4-byte index and, through it, the 16 bytes of
// accumulated irradiance, and decides; the survivors are compacted in the three steps of pt_lightmap.hip -- pt_ag_count (per
// 256-entry block, which also counts the block's stops by reason), pt_ag_scan (one workgroup: the exclusive prefix of the block
// counts, the totals), pt_ag_emit (a lane's rank is the block's base plus the earlier waves' counts plus the popcount of the
// ballot below its lane; it writes the index and copies the receiver as two 16-byte loads and stores).  Fold and equalise are
// one lane per entry with 16-byte accesses.  No atomics at all, so the same input gives the same bytes whatever the launch
// geometry.
#include "pt_adaptive_gather.h"
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
    uint32_t idx;
    const uint32_t r = decide(A, blockIdx.x * 256u + threadIdx.x, idx);
    const int kept = __syncthreads_count(r == kActive);
    const int byThreshold = __syncthreads_count(r == kByThreshold);
    const int byMax = __syncthreads_count(r == kByMaxSamples);
    const int nonFinite = __syncthreads_count(r == kNonFinite);
    if (threadIdx.x == 0u) {
        A.blockCounts[blockIdx.x] = (uint32_t)kept;
        A.blockCounts[(size_t)blocks + blockIdx.x] = (uint32_t)byThreshold;
        A.blockCounts[(size_t)blocks * 2u + blockIdx.x] = (uint32_t)byMax;
        A.blockCounts[(size_t)blocks * 3u + blockIdx.x] = (uint32_t)nonFinite;
    }
}

// One workgroup: thread k owns a contiguous run of block counts; the runs' sums are scanned across the workgroup, then every run
// of the survivor counts is rewritten as the exclusive prefix.  The three stop counts are only summed.  At most 2^31 / 256 counts:
// 8,192 per thread.  Every total is below 2^32.
__global__ __launch_bounds__(1024) void pt_ag_scan(uint32_t* __restrict__ blockCounts, uint32_t blocks, uint64_t* __restrict__ totals)
{
    __shared__ uint32_t waveSum[4][16];
    const uint32_t per = (blocks + 1023u) / 1024u;
    const uint32_t lo = threadIdx.x * per < blocks ? threadIdx.x * per : blocks, hi = lo + per < blocks ? lo + per : blocks;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t sum[4] = {0u, 0u, 0u, 0u};
    for (int q = 0; q < 4; ++q)
        for (uint32_t j = lo; j < hi; ++j) sum[q] += blockCounts[(size_t)blocks * q + j];
    uint32_t incl[4] = {sum[0], sum[1], sum[2], sum[3]};           // inclusive scans within the wave
    for (int off = 1; off < 64; off <<= 1)
        for (int q = 0; q < 4; ++q) {
            const uint32_t v = __shfl_up(incl[q], off, 64);
            if (lane >= (uint32_t)off) incl[q] += v;
        }
    if (lane == 63u)
        for (int q = 0; q < 4; ++q) waveSum[q][wave] = incl[q];
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += waveSum[0][w];
    uint32_t running = before + incl[0] - sum[0];
    for (uint32_t j = lo; j < hi; ++j) {
        const uint32_t c = blockCounts[j];
        blockCounts[j] = running;
        running += c;
    }
    if (threadIdx.x < 4u) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < 16u; ++w) all += waveSum[threadIdx.x][w];
        totals[threadIdx.x] = all;
    }
}

__global__ __launch_bounds__(256) void pt_ag_emit(PTAgSelectArgs A)
{
    __shared__ uint32_t waveCount[4];
    uint32_t idx;
    const bool kept = decide(A, blockIdx.x * 256u + threadIdx.x, idx) == kActive;
    const unsigned long long mask = __ballot(kept);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) waveCount[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (!kept) return;
    uint32_t rank = A.blockCounts[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) rank += waveCount[w];
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
