// repack_sanitize_main.cpp — the host twin of the repack kernels (repack_host.cpp) in a stand-alone program for `make repack-sanitize`
// (AddressSanitizer + UBSan, host code only, no GPU): plans and moves generated flag arrays in exactly sized heap arrays, checks
// every result against a plain loop over the slots, and walks the edges of the decision.  Prints "repack ok" and returns 0, or
// says what went wrong.
#include <cstdio>
#include <cstring>
#include <vector>
#include "repack_rule.h"

namespace {

uint32_t g_state = 2463534242u;
uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 17; g_state ^= g_state << 5; return g_state; }

int bad(const char* what) { std::printf("repack-sanitize: %s\n", what); return 1; }

// one array of flag words: plan it, compare with the plain loop, move a payload and the flags, compare again
int run(const std::vector<uint32_t>& flags, uint32_t capacity, uint32_t num, uint32_t den, int expectGo)
{
    using namespace ptrepack;
    const uint32_t n = (uint32_t)flags.size();
    // the plain loop: live slots in slot order, the last live slot
    std::vector<uint32_t> liveSlots;
    for (uint32_t s = 0; s < n; ++s) if ((flags[s] & 3u) != 2u) liveSlots.push_back(s);
    const uint32_t L = (uint32_t)liveSlots.size();
    const uint32_t E = L ? (liveSlots.back() / PT_REPACK_BLOCK + 1u) * PT_REPACK_BLOCK : 0u;
    const bool go = L > 0u && L <= capacity && (unsigned long long)L * den <= (unsigned long long)E * num;

    Plan plan;
    std::vector<uint32_t> dest(n), prefix(n / PT_REPACK_BLOCK);
    if (!plan_host(flags.data(), n, capacity, num, den, plan, dest.data(), prefix.data())) return bad("plan_host refused a well-formed array");
    if (plan.live != L || plan.extent != E) return bad("live count or extent differ from the plain loop");
    if ((plan.go != 0u) != go) return bad("the decision differs from the plain loop");
    if (expectGo >= 0 && (int)plan.go != expectGo) return bad("an edge of the decision fell on the wrong side");
    for (uint32_t k = 0; k < L; ++k) if (dest[liveSlots[k]] != k) return bad("a live slot's destination is not its rank among the live slots");
    for (uint32_t s = 0; s < n; ++s) if ((flags[s] & 3u) == 2u && dest[s] != 0xFFFFFFFFu) return bad("a finished slot has a destination");

    // payloads of 4 and 32 bytes (the flag words and a ray record), each in an exactly sized array
    std::vector<uint32_t> f(flags);
    std::vector<uint32_t> rec((size_t)n * 8u);
    for (uint32_t s = 0; s < n; ++s) for (uint32_t k = 0; k < 8u; ++k) rec[(size_t)s * 8u + k] = s * 8u + k;
    move_host(plan, dest.data(), n, rec.data(), 32u, false);
    move_host(plan, dest.data(), n, f.data(), 4u, true);
    if (!plan.go) {
        if (std::memcmp(f.data(), flags.data(), (size_t)n * 4u) != 0) return bad("a refused plan changed the flags");
        return 0;
    }
    for (uint32_t s = 0; s < n; ++s) {
        if (s < L) {
            if (f[s] != flags[liveSlots[s]]) return bad("slot order is not stable");
            for (uint32_t k = 0; k < 8u; ++k) if (rec[(size_t)s * 8u + k] != liveSlots[s] * 8u + k) return bad("a record did not follow its slot");
        } else if (s < E) {
            if (f[s] != 2u) return bad("a slot between the live ones and the extent is not DONE");
        } else if (f[s] != flags[s]) return bad("a slot beyond the extent was touched");
    }
    return 0;
}

std::vector<uint32_t> make(uint32_t n, uint32_t livePerMille)
{
    std::vector<uint32_t> f(n);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t hi = rnd() & ~3u;                                     // the other bits of a flags word: anything
        f[s] = hi | ((rnd() % 1000u) < livePerMille ? (rnd() & 1u) : 2u);    // TRACE or ENDING, or DONE
    }
    return f;
}

} // namespace

int main()
{
    const uint32_t B = PT_REPACK_BLOCK;
    // random arrays of 1 ... 40 blocks at every density, the fill thresholds of the product and of the stress build
    for (uint32_t trial = 0; trial < 200u; ++trial) {
        const uint32_t n = (1u + rnd() % 40u) * B;
        const std::vector<uint32_t> f = make(n, rnd() % 1001u);
        if (run(f, n / 2u, 3u, 4u, -1) || run(f, n / 2u, 1u, 1u, -1)) return 1;
    }
    const uint32_t n = 8u * B, cap = n / 2u;
    std::vector<uint32_t> f(n, 2u);
    if (run(f, cap, 1u, 1u, 0)) return 1;                                   // no live slot
    std::fill(f.begin(), f.end(), 0u);
    if (run(f, cap, 1u, 1u, 0)) return 1;                                   // all live: L > capacity
    if (run(f, n, 1u, 1u, 1)) return 1;                                     // ... L == E with room for it: a (pointless) go at fill 1/1
    if (run(f, n, 3u, 4u, 0)) return 1;                                     // ... and refused at 3/4
    std::fill(f.begin(), f.end(), 2u);
    for (uint32_t k = 0; k < cap; ++k) f[2u * k + 1u] = 1u;
    if (run(f, cap, 1u, 1u, 1)) return 1;                                   // L == capacity
    f[0] = 0u;
    if (run(f, cap, 1u, 1u, 0)) return 1;                                   // L == capacity + 1: refused
    std::fill(f.begin(), f.end(), 2u);
    f[n - 1u] = 0u; f[n - B] = 1u; f[n - 7u] = 0u;
    if (run(f, cap, 3u, 4u, 1)) return 1;                                   // live slots only in the last block
    std::vector<uint32_t> one(B, 2u);
    one[5] = 0u; one[200] = 1u;
    if (run(one, B / 2u, 3u, 4u, 1)) return 1;                              // an extent of one block
    std::fill(one.begin(), one.end(), 0u);
    if (run(one, B, 1u, 1u, 1)) return 1;                                   // ... full
    // the refusals of the twin itself
    ptrepack::Plan plan;
    if (ptrepack::plan_host(f.data(), n - 1u, cap, 3u, 4u, plan, nullptr, nullptr)) return bad("a slot count that is no multiple of the block was accepted");
    if (ptrepack::plan_host(f.data(), n, cap, 3u, 0u, plan, nullptr, nullptr)) return bad("a fill of x / 0 was accepted");
    std::printf("repack ok\n");
    return 0;
}
