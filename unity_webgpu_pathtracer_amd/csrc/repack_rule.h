// repack_rule.h — where the live path slots of a wavefront state set go when the set is repacked mid-pass (pt_repack.hip,
// DESIGN.md 5.1): the one definition of the rule, shared by the repack kernels and the host twin (repack_host.cpp).  All of it
// is 32-bit integer arithmetic on slot indices, so both sides give the same numbers by construction.
//
//   count   live slots per block of PT_REPACK_BLOCK consecutive slots (a slot is live when its state is not DONE)
//   scan    prefix[b] = live slots of the blocks before b;  L = all live slots;  E = end of the highest block with a live slot
//   decide  repack iff 0 < L <= capacity and L <= fill * E  (the temporary region holds `capacity` slots; fill = num / den)
//   move    the r-th live slot of block b (r counted in slot order) goes to position prefix[b] + r: stable, so slot order stays
//           screen order; afterwards slots [0, L) are the live ones and every slot of [L, E) is DONE.  Slots >= E were DONE already.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_REPACK_HD __host__ __device__ __forceinline__
#else
#define PT_REPACK_HD inline
#endif

#define PT_REPACK_BLOCK 256u        // slots per counted block = threads per workgroup of the count and move kernels
#define PT_REPACK_STATE_DONE 2u     // PS_DONE of pt_device.h (checked by a static_assert in pt_repack.hip)

namespace ptrepack {

// words of the decision record the scan kernel leaves for the two move kernels
enum : uint32_t { PT_REPACK_GO = 0, PT_REPACK_LIVE, PT_REPACK_EXTENT, PT_REPACK_CTL_WORDS };
// the counters PTGetRepackStats reports (PTRepackStats order)
enum : uint32_t { PT_REPACK_STAT_SEQUENCES = 0, PT_REPACK_STAT_CANDIDATES, PT_REPACK_STAT_REPACKS, PT_REPACK_STAT_MOVED, PT_REPACK_STAT_WORDS };

PT_REPACK_HD bool slot_live(uint32_t flagsWord) { return (flagsWord & 3u) != PT_REPACK_STATE_DONE; }

// E from the highest block with a live slot (blocks are numbered from 0; none: 0)
PT_REPACK_HD uint32_t extent_of(bool anyLive, uint32_t highestLiveBlock) { return anyLive ? (highestLiveBlock + 1u) * PT_REPACK_BLOCK : 0u; }

// 64-bit products: L * den and E * num do not fit 32 bits for every set a batch can make
PT_REPACK_HD bool decide(uint32_t L, uint32_t E, uint32_t capacity, uint32_t fillNum, uint32_t fillDen)
{
    return L > 0u && L <= capacity && (uint64_t)L * fillDen <= (uint64_t)E * fillNum;
}

PT_REPACK_HD uint32_t destination(uint32_t blockPrefix, uint32_t rankInBlock) { return blockPrefix + rankInBlock; }

// after the move: what becomes of slot s
enum class After : uint32_t { Live, Done, Untouched };
PT_REPACK_HD After after_move(uint32_t slot, uint32_t L, uint32_t E) { return slot < L ? After::Live : slot < E ? After::Done : After::Untouched; }

// ---- host side (repack_host.cpp) ----
struct Plan {
    uint32_t go;            // 1: the set is repacked
    uint32_t live, extent;  // L, E
};
// The rule over a host copy of the flag words (numSlots a multiple of PT_REPACK_BLOCK): the plan, and with dest != NULL the
// destination of every slot (0xFFFFFFFF for a slot that is not live), whether or not the plan says go.
// blockPrefix (may be NULL): numSlots / PT_REPACK_BLOCK words.  false: numSlots is not a multiple of the block or fillDen == 0.
bool plan_host(const uint32_t* flags, uint32_t numSlots, uint32_t capacity, uint32_t fillNum, uint32_t fillDen, Plan& plan, uint32_t* dest,
               uint32_t* blockPrefix);
// Applies a plan that says go to one array of `stride`-byte records in place, through a temporary of plan.live records -- the two
// moves of the kernels -- and, for the flag words themselves (isFlags), writes DONE into [L, E).
void move_host(const Plan& plan, const uint32_t* dest, uint32_t numSlots, void* array, uint32_t stride, bool isFlags);

} // namespace ptrepack
