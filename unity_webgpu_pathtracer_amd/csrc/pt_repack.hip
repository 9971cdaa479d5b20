// pt_repack.hip — the mid-pass slot repack of schedule 1 over PTTileMap (sets of pt_wf_repack_slots() slots or more):
// the four kernels that move the live slots of a state set to its front, and the shade and cleanup kernels of a sequence that
// does so.  pt_wavefront.hip's launch sequence enters through the three launchers at the end (pt_launch.h); its own kernels, and
// every sequence that does not repack, are what they were.
#include "pt_device.h"
#include "pt_launch.h"
#include "pt_wf_state.h"
#include "pt_wf_shade.h"
#include "pt_compact.h"
#include "repack_rule.h"

namespace {

// ------------------------------------------------------------------------------------------
// The four kernels of a repack candidate.
//
// A slot is alive for 17 of the 52 iterations of the Sponza-class pass on average, but the 64 pixels of a shade wave finish
// iterations apart, and the wave pays the whole step until its LAST pixel is done: the shade launches execute 1.5 lane-slots per
// live one, and late trace ranges hold a handful of rays (profiles/slot_repack_ab.md).  An index list of the live slots was
// measured twice and lost 20 % both times, because the state was then gathered through the list in EVERY iteration
// (DESIGN.md 5.1).  Here the state itself is moved, after the shade launch of a few candidate iterations (pt_launch.h
// PT_WF_REPACK_*), when the live set has shrunk enough: slot order is dense again, every later access is as coalesced as before,
// and the gather is paid once per repack.  Four small launches, no host synchronisation; the rule is repack_rule.h's:
//     count      live slots per block of 256
//     scan       one workgroup: exclusive prefix over the blocks, L, E, the decision -- and the four counters of PTGetRepackStats
//     move out   the r-th live slot of block b -> position prefix[b] + r of the temporary SoA region (stable: still screen order)
//     move back  temporary [0, L) -> slots [0, L); every slot of [L, E) becomes DONE
// Both moves exit at once when the decision word says no.  What moves is what is live between a shade and a trace launch: flags,
// the three ray records, rad, thr, color, envC, lightC and the slot's pixel index (184 bytes); the RNG state and the pending
// throughput of a repacked sequence ride in the fourth lanes of rad, envC, lightC and thr (pt_wf_state.h), so B.rng and B.pthr hold
// nothing of it; hit, hit2, occl and the suspension records are dead there.  Going through a temporary and BACK, not switching
// regions, keeps every other kernel as it is: no second set of base pointers, no extent.  The temporary holds numSlots / 2 slots
// and aliases stackSpill + susp, which the trace launches fill before they read them (pt_wf_arena_layout, pt_wavefront.hip,
// proves the room or carves new memory).
// ------------------------------------------------------------------------------------------
static_assert(PT_REPACK_STATE_DONE == PS_DONE && PT_REPACK_BLOCK == 256u, "repack_rule.h restates the state code and the block");

// the SoA layout of the temporary region for rpCapacity slots: eleven float4 planes in PT_F4_* order (a ray record takes two),
// then two planes of 32-bit words (flags, pixelOf)
PT_DEV uint32_t* rp_u32(const PTWfBuffers& B, uint32_t k) { return (uint32_t*)((float4*)B.rpTemp + (size_t)PT_F4_PTHR * B.rpCapacity) + (size_t)k * B.rpCapacity; }
static_assert(PT_F4_PTHR == 11u && PT_F4_LIGHTC + 1u == PT_F4_PTHR && PT_F4_PTHR * 16u + 2u * 4u == PT_WF_REPACK_SLOT_BYTES,
              "the moved state is the eleven float4 planes before PT_F4_PTHR and two words");

// count and scan: the first two steps of pt_compact.h over the live slots
__global__ __launch_bounds__(256) void pt_wf_repack_count(PTWfBuffers B)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;                 // numSlots is a multiple of 256
    uint32_t blockLive;
    compact_rank_in_block(ptrepack::slot_live(B.flags[slot]), s_wave, blockLive);
    if (threadIdx.x == 0u) B.rpPrefix[blockIdx.x] = blockLive;
}

// ... which also finds the highest live block, decides, and counts for PTGetRepackStats
__global__ __launch_bounds__(1024) void pt_wf_repack_scan(PTWfBuffers B, uint32_t fillNum, uint32_t fillDen, uint32_t firstOfSequence, unsigned long long* stats)
{
    __shared__ uint32_t s_sum[16], s_hi[16];
    uint32_t hi = 0u;                                                      // highest live block + 1 (0: none)
    const uint32_t L = compact_scan_blocks(B.rpPrefix, B.numSlots >> 8, s_sum, [&](uint32_t b, uint32_t c) { if (c) hi = b + 1u; });
#pragma unroll
    for (uint32_t off = 32u; off > 0u; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)hi, (int)off, 64); hi = o > hi ? o : hi; }
    if ((threadIdx.x & 63u) == 0u) s_hi[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t top = 0u;
        for (uint32_t i = 0; i < 16u; ++i) top = s_hi[i] > top ? s_hi[i] : top;
        const uint32_t E = ptrepack::extent_of(top != 0u, top - 1u);
        const bool go = ptrepack::decide(L, E, B.rpCapacity, fillNum, fillDen);
        B.rpCtl[ptrepack::PT_REPACK_GO] = go ? 1u : 0u;
        B.rpCtl[ptrepack::PT_REPACK_LIVE] = L;
        B.rpCtl[ptrepack::PT_REPACK_EXTENT] = E;
        if (stats) {                                                       // sets in flight share the context's counters
            if (firstOfSequence) atomicAdd(stats + ptrepack::PT_REPACK_STAT_SEQUENCES, 1ull);
            atomicAdd(stats + ptrepack::PT_REPACK_STAT_CANDIDATES, 1ull);
            if (go) { atomicAdd(stats + ptrepack::PT_REPACK_STAT_REPACKS, 1ull); atomicAdd(stats + ptrepack::PT_REPACK_STAT_MOVED, (unsigned long long)L); }
        }
    }
}

// One slot's moved state, from one layout to the other: eleven float4 planes at a stride (PT_F4_* order: a ray record is two
// consecutive float4 at index 2 * slot of a plane two strides wide) and two planes of words.  All loads are requested before the
// first store; spelled out plane by plane, so that nothing is indexed at run time and nothing goes to scratch.
struct RpLayout { float4* f4; size_t stride; uint32_t *flags, *pixelOf; };
PT_DEV RpLayout rp_set_layout(const PTWfBuffers& B) { return RpLayout{B.f4base, B.f4stride, B.flags, B.pixelOf}; }
PT_DEV RpLayout rp_temp_layout(const PTWfBuffers& B) { return RpLayout{(float4*)B.rpTemp, B.rpCapacity, rp_u32(B, 0u), rp_u32(B, 1u)}; }
PT_DEV void rp_copy(const RpLayout& s, size_t si, const RpLayout& d, size_t di, uint32_t flagsWord)
{
    const float4* s0 = s.f4 + PT_F4_RAY0 * s.stride + 2u * si;
    const float4* s1 = s.f4 + PT_F4_RAY1 * s.stride + 2u * si;
    const float4* s2 = s.f4 + PT_F4_RAY2 * s.stride + 2u * si;
    const float4 a0 = s0[0], a1 = s0[1], b0 = s1[0], b1 = s1[1], c0 = s2[0], c1 = s2[1];
    const float4 rad = s.f4[PT_F4_RAD * s.stride + si], thr = s.f4[PT_F4_THR * s.stride + si], col = s.f4[PT_F4_COLOR * s.stride + si];
    const float4 envC = s.f4[PT_F4_ENVC * s.stride + si], lightC = s.f4[PT_F4_LIGHTC * s.stride + si];
    const uint32_t pix = s.pixelOf[si];
    float4* d0 = d.f4 + PT_F4_RAY0 * d.stride + 2u * di;
    float4* d1 = d.f4 + PT_F4_RAY1 * d.stride + 2u * di;
    float4* d2 = d.f4 + PT_F4_RAY2 * d.stride + 2u * di;
    d0[0] = a0; d0[1] = a1; d1[0] = b0; d1[1] = b1; d2[0] = c0; d2[1] = c1;
    d.f4[PT_F4_RAD * d.stride + di] = rad; d.f4[PT_F4_THR * d.stride + di] = thr; d.f4[PT_F4_COLOR * d.stride + di] = col;
    d.f4[PT_F4_ENVC * d.stride + di] = envC; d.f4[PT_F4_LIGHTC * d.stride + di] = lightC;
    d.flags[di] = flagsWord; d.pixelOf[di] = pix;
}

__global__ __launch_bounds__(256) void pt_wf_repack_out(PTWfBuffers B)
{
    __shared__ uint32_t s_wave[4];
    if (B.rpCtl[ptrepack::PT_REPACK_GO] == 0u) return;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= B.rpCtl[ptrepack::PT_REPACK_EXTENT]) return;              // workgroup-uniform: E is a multiple of 256
    const uint32_t f = B.flags[slot];
    const bool live = ptrepack::slot_live(f);
    uint32_t blockLive;
    const uint32_t rank = compact_rank_in_block(live, s_wave, blockLive);
    if (!live) return;
    const uint32_t d = ptrepack::destination(B.rpPrefix[blockIdx.x], rank);
    if (d >= B.rpCapacity) return;                                         // never: the decision admits L <= capacity only
    rp_copy(rp_set_layout(B), slot, rp_temp_layout(B), d, f);
}

__global__ __launch_bounds__(256) void pt_wf_repack_back(PTWfBuffers B)
{
    if (B.rpCtl[ptrepack::PT_REPACK_GO] == 0u) return;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const ptrepack::After w = ptrepack::after_move(slot, B.rpCtl[ptrepack::PT_REPACK_LIVE], B.rpCtl[ptrepack::PT_REPACK_EXTENT]);
    if (w == ptrepack::After::Done) B.flags[slot] = PS_DONE;
    if (w != ptrepack::After::Live) return;
    const RpLayout T = rp_temp_layout(B);
    rp_copy(T, slot, rp_set_layout(B), slot, T.flags[slot]);
}

// ------------------------------------------------------------------------------------------
// shade and cleanup of a repacked sequence: pt_wf_shade / pt_wf_cleanup over PTTileMap (pt_wavefront.hip) with the pixel slot taken
// from B.pixelOf -- a slot's path belongs to the pixel that array says -- and a finished pixel's sample sum left in
// B.pixsum[that pixel slot], because the slot itself may be given to another path (shade_slot's PIXSUM, as in schedule 4).  Only
// these kernels exist for a repacked sequence, so its state has a layout of its own (shade_slot's PACKED, cleanup_slots' REPACK):
// 45 bytes fewer per live slot and step (profiles/packed_state_ab.md).
// Same line as the shade kernel's: <= 128 VGPRs, no scratch, four waves per SIMD (tests/test_repack.py).
// ------------------------------------------------------------------------------------------
template <bool STATS>
__global__ __launch_bounds__(PT_WF_SHADE_BLOCK, PT_WF_SHADE_MIN_WAVES) void pt_wf_shade_repack(DScene S, PTFrameParams P, PTTileMap tm, PTWfBuffers B,
                                                                                uint32_t iteration)
{
    const uint32_t vb = blockIdx.x;
    const uint32_t slot = vb * PT_WF_SHADE_BLOCK + threadIdx.x;
    if (vb == 0u && threadIdx.x < PT_WF_SHARDS) B.chunkHeads[threadIdx.x * 32u] = 0u;   // as pt_wf_shade does
    const uint32_t f = B.flags[slot];
    Counters cn = {};
    if (fl_state(f) != PS_DONE) shade_slot<STATS, true, PTTileMap, true>(S, P, tm, B, slot, B.pixelOf[slot], f, cn, vb * PT_WF_SHADE_BLOCK);
    flush_counters<STATS>(cn, B.statRows, vb * (PT_WF_SHADE_BLOCK / 64u) + (threadIdx.x >> 6), threadIdx.x & 63u);
}

template <bool STATS, bool TLAS>
__global__ __launch_bounds__(256, 2) void pt_wf_cleanup_repack(DScene S, PTFrameParams P, PTTileMap tm, PTWfBuffers B)
{
    __shared__ uint2 s_stack[PT_LDS_STACK][256];
    cleanup_slots<STATS, TLAS, true, PTTileMap>(S, P, tm, B, s_stack);
}

} // namespace

hipError_t pt_launch_repack(const PTWfBuffers& B, uint32_t fillNum, uint32_t fillDen, bool firstOfSequence, unsigned long long* stats, hipStream_t stream)
{
    const uint32_t nb = B.numSlots >> 8;
    hipLaunchKernelGGL(pt_wf_repack_count, dim3(nb), dim3(256), 0, stream, B);
    hipLaunchKernelGGL(pt_wf_repack_scan, dim3(1), dim3(1024), 0, stream, B, fillNum, fillDen, firstOfSequence ? 1u : 0u, stats);
    hipLaunchKernelGGL(pt_wf_repack_out, dim3(nb), dim3(256), 0, stream, B);
    hipLaunchKernelGGL(pt_wf_repack_back, dim3(nb), dim3(256), 0, stream, B);
    return hipGetLastError();
}

hipError_t pt_launch_repack_shade(const DScene& S, const PTFrameParams& P, const PTTileMap& tm, const PTWfBuffers& B, bool fullStats, uint32_t iteration,
                                  hipStream_t stream)
{
    const dim3 grid(B.numSlots / PT_WF_SHADE_BLOCK), block(PT_WF_SHADE_BLOCK);
    if (fullStats) hipLaunchKernelGGL(pt_wf_shade_repack<true>, grid, block, 0, stream, S, P, tm, B, iteration);
    else hipLaunchKernelGGL(pt_wf_shade_repack<false>, grid, block, 0, stream, S, P, tm, B, iteration);
    return hipGetLastError();
}

hipError_t pt_launch_repack_cleanup(const DScene& S, const PTFrameParams& P, const PTTileMap& tm, const PTWfBuffers& B, bool fullStats, uint32_t blocks,
                                    hipStream_t stream)
{
    const bool tlas = S.hasTlas != 0u;
    if (fullStats) {
        if (tlas) hipLaunchKernelGGL((pt_wf_cleanup_repack<true, true>), dim3(blocks), dim3(256), 0, stream, S, P, tm, B);
        else hipLaunchKernelGGL((pt_wf_cleanup_repack<true, false>), dim3(blocks), dim3(256), 0, stream, S, P, tm, B);
    } else {
        if (tlas) hipLaunchKernelGGL((pt_wf_cleanup_repack<false, true>), dim3(blocks), dim3(256), 0, stream, S, P, tm, B);
        else hipLaunchKernelGGL((pt_wf_cleanup_repack<false, false>), dim3(blocks), dim3(256), 0, stream, S, P, tm, B);
    }
    return hipGetLastError();
}
