// repack_host.cpp — the host twin of the repack kernels of pt_repack.hip: the rule of repack_rule.h applied block by block in
// the kernels' order (count, scan and decide, move out, move back).  No GPU involved; tests/test_repack.py and the stand-alone
// sanitizer program (repack_sanitize_main.cpp) run it.
#include <cstring>
#include <vector>
#include "repack_rule.h"

namespace ptrepack {

bool plan_host(const uint32_t* flags, uint32_t numSlots, uint32_t capacity, uint32_t fillNum, uint32_t fillDen, Plan& plan, uint32_t* dest,
               uint32_t* blockPrefix)
{
    plan = Plan{0u, 0u, 0u};
    if (numSlots % PT_REPACK_BLOCK != 0u || fillDen == 0u || (numSlots != 0u && !flags)) return false;
    const uint32_t blocks = numSlots / PT_REPACK_BLOCK;
    // count
    std::vector<uint32_t> count(blocks, 0u);
    for (uint32_t b = 0; b < blocks; ++b)
        for (uint32_t t = 0; t < PT_REPACK_BLOCK; ++t) count[b] += slot_live(flags[b * PT_REPACK_BLOCK + t]) ? 1u : 0u;
    // scan and decide
    std::vector<uint32_t> prefix(blocks, 0u);
    uint32_t L = 0u, highest = 0u;
    bool any = false;
    for (uint32_t b = 0; b < blocks; ++b) {
        prefix[b] = L;
        L += count[b];
        if (count[b] != 0u) { any = true; highest = b; }
    }
    plan.live = L;
    plan.extent = extent_of(any, highest);
    plan.go = decide(L, plan.extent, capacity, fillNum, fillDen) ? 1u : 0u;
    if (blockPrefix) std::memcpy(blockPrefix, prefix.data(), (size_t)blocks * sizeof(uint32_t));
    // the destinations the move-out kernel forms: block prefix + rank among the block's live slots
    if (dest) {
        for (uint32_t b = 0; b < blocks; ++b) {
            uint32_t rank = 0u;
            for (uint32_t t = 0; t < PT_REPACK_BLOCK; ++t) {
                const uint32_t s = b * PT_REPACK_BLOCK + t;
                if (slot_live(flags[s])) dest[s] = destination(prefix[b], rank++);
                else dest[s] = 0xFFFFFFFFu;
            }
        }
    }
    return true;
}

void move_host(const Plan& plan, const uint32_t* dest, uint32_t numSlots, void* array, uint32_t stride, bool isFlags)
{
    if (!plan.go) return;
    std::vector<unsigned char> tmp((size_t)plan.live * stride);
    unsigned char* a = (unsigned char*)array;
    // move out: every live slot below the extent (there is none above it)
    for (uint32_t s = 0; s < plan.extent && s < numSlots; ++s)
        if (dest[s] != 0xFFFFFFFFu) std::memcpy(&tmp[(size_t)dest[s] * stride], a + (size_t)s * stride, stride);
    // move back, and DONE into the rest of the extent
    for (uint32_t s = 0; s < plan.extent && s < numSlots; ++s) {
        const After w = after_move(s, plan.live, plan.extent);
        if (w == After::Live) std::memcpy(a + (size_t)s * stride, &tmp[(size_t)s * stride], stride);
        else if (w == After::Done && isFlags) {
            const uint32_t done = PT_REPACK_STATE_DONE;
            std::memcpy(a + (size_t)s * stride, &done, sizeof(done) < stride ? sizeof(done) : stride);
        }
    }
}

} // namespace ptrepack
