// adaptive_gather_sanitize_main.cpp — the host twins of the adaptive gather's steps (adaptive_gather_host.cpp) in a stand-alone
// program for `make adaptive-gather-sanitize` (AddressSanitizer + UBSan, host code only, no GPU): runs the whole loop of Part 19 over
// generated "gathers" in exactly sized heap arrays (lists of 1, 255, 256, 257 and 1,000 entries with non-finite ones among them),
// equalises the result in place and out of place, and makes the refusals.  Prints "adaptive gather ok" and returns 0, or says what
// went wrong.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "adaptive_gather_rule.h"

namespace {

uint32_t g_state = 1919u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("adaptive-gather-sanitize: %s\n", what); return 1; }

PTAdaptiveGather adaptive(uint32_t mn, uint32_t add, uint32_t mx, float threshold, float darkFloor)
{
    PTAdaptiveGather a = {};
    a.structSize = sizeof(a);
    a.minSamples = mn; a.addSamples = add; a.maxSamples = mx; a.threshold = threshold; a.darkFloor = darkFloor;
    return a;
}

// a stand-in for a gather of m samples of entry i: mean e, and an m2 whose spread grows with the entry's index
PTIrradiance fake_gather(uint32_t i, uint32_t m)
{
    const float e = 0.25f + rnd(), spread = 1.0f + 0.002f * (float)(i % 500u) * rnd();
    return PTIrradiance{{e, 0.5f * e, 0.25f * e}, (float)m * (e * 0.6215f) * (e * 0.6215f) * spread};
}

} // namespace

int main()
{
    using namespace ptag;
    std::string err;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static const uint64_t kSizes[5] = {1, 255, 256, 257, 1000};
    for (const uint64_t n : kSizes) {
        const PTAdaptiveGather a = adaptive(8, 8, 40, 0.05f, 0.01f);
        std::vector<PTReceiver> recv(n);
        for (uint64_t i = 0; i < n; ++i) recv[i] = PTReceiver{{(float)i, 0.0f, 1.0f}, (uint32_t)i * 7u, {0.0f, 1.0f, 0.0f}, 0u};
        std::vector<PTIrradiance> acc(n), fresh(n);
        std::vector<uint32_t> counts(n, 0u), listA(n), listB(n);
        std::vector<PTReceiver> compact(n);
        // round 0 writes
        for (uint64_t i = 0; i < n; ++i) {
            fresh[i] = fake_gather((uint32_t)i, a.minSamples);
            if (i % 37u == 5u) fresh[i].rgb[2] = nan;
            if (i % 37u == 11u) fresh[i].m2 = inf;
        }
        if (!fold_host(nullptr, n, fresh.data(), a.minSamples, 0u, n, acc.data(), counts.data(), err)) return bad(err.c_str());
        if (std::memcmp(acc.data(), fresh.data(), n * sizeof(PTIrradiance)) != 0) return bad("round 0 did not write the gather's bytes");
        uint32_t have = a.minSamples;
        uint64_t active = 0, stopped[3], stops[3] = {0, 0, 0};
        if (!select_host(&a, have, nullptr, n, acc.data(), recv.data(), n, listA.data(), compact.data(), &active, stopped, err)) return bad(err.c_str());
        uint32_t* cur = listA.data();
        uint32_t* nxt = listB.data();
        for (;;) {
            for (int k = 0; k < 3; ++k) stops[k] += stopped[k];
            if (!active) break;
            for (uint64_t k = 0; k < active; ++k) {
                if (k && cur[k] <= cur[k - 1]) return bad("the active list is not ascending");
                if (std::memcmp(&compact[k], &recv[cur[k]], sizeof(PTReceiver)) != 0) return bad("a receiver did not travel with its index");
                fresh[k] = fake_gather(cur[k], a.addSamples);
            }
            if (!fold_host(cur, active, fresh.data(), a.addSamples, have, n, acc.data(), counts.data(), err)) return bad(err.c_str());
            have += a.addSamples;
            const uint64_t before = active;
            if (!select_host(&a, have, cur, before, acc.data(), recv.data(), n, nxt, compact.data(), &active, stopped, err)) return bad(err.c_str());
            if (active > before) return bad("the active list grew");
            uint32_t* t = cur; cur = nxt; nxt = t;
        }
        if (stops[0] + stops[1] + stops[2] != n) return bad("the stop counts do not add up to the list");
        for (uint64_t i = 0; i < n; ++i) {
            if (counts[i] < a.minSamples || counts[i] > a.maxSamples || (counts[i] - a.minSamples) % a.addSamples) return bad("a count is off the rounds' grid");
            if ((i % 37u == 5u || i % 37u == 11u) && counts[i] != a.minSamples) return bad("a non-finite entry went on");
        }
        // equalise, out of place and in place
        std::vector<PTIrradiance> eq(n), inplace(acc);
        if (!equalise_host(acc.data(), counts.data(), n, a.maxSamples, eq.data(), err)) return bad(err.c_str());
        if (!equalise_host(inplace.data(), counts.data(), n, a.maxSamples, inplace.data(), err)) return bad(err.c_str());
        if (std::memcmp(eq.data(), inplace.data(), n * sizeof(PTIrradiance)) != 0) return bad("in place differs from out of place");
        for (uint64_t i = 0; i < n; ++i) {
            if (std::memcmp(eq[i].rgb, acc[i].rgb, 12) != 0) return bad("equalise moved an rgb");
            if ((i % 37u == 5u || i % 37u == 11u) && std::memcmp(&eq[i], &acc[i], 16) != 0) return bad("a non-finite entry's bytes moved");
        }
        // the refusals
        uint64_t s = 0;
        if (!select_host(&a, 8, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, &s, nullptr, err)) return bad("an empty list was refused");
        std::vector<uint32_t> list(n);
        for (uint64_t i = 0; i < n; ++i) list[i] = (uint32_t)i;
        list[n - 1] = (uint32_t)n;
        if (select_host(&a, 8, list.data(), n, acc.data(), recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("an index past the list was not refused");
        if (fold_host(list.data(), n, fresh.data(), 8, 8, n, acc.data(), nullptr, err)) return bad("fold: an index past the list was not refused");
        if (select_host(&a, 1, nullptr, n, acc.data(), recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("n = 1 was not refused");
        if (select_host(&a, 8, nullptr, n + 1, acc.data(), recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("activeCount > entryCount was not refused");
        if (select_host(&a, 8, nullptr, n, nullptr, recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("a NULL array was not refused");
        PTAdaptiveGather b = a; b.minSamples = 1;
        if (select_host(&b, 8, nullptr, n, acc.data(), recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("minSamples 1 was not refused");
        b = a; b.maxSamples = 7;
        if (select_host(&b, 8, nullptr, n, acc.data(), recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("maxSamples < minSamples was not refused");
        b = a; b.threshold = 0.0f;
        if (select_host(&b, 8, nullptr, n, acc.data(), recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("threshold 0 was not refused");
        b = a; b.darkFloor = nan;
        if (select_host(&b, 8, nullptr, n, acc.data(), recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("a NaN darkFloor was not refused");
        b = a; b.reserved[4] = 1;
        if (select_host(&b, 8, nullptr, n, acc.data(), recv.data(), n, listA.data(), compact.data(), &s, nullptr, err)) return bad("a reserved word was not refused");
        if (fold_host(nullptr, n, fresh.data(), 0, 8, n, acc.data(), nullptr, err)) return bad("m = 0 was not refused");
        if (fold_host(nullptr, n, fresh.data(), 8, kMaxCount, n, acc.data(), nullptr, err)) return bad("n + m > 2^24 was not refused");
        if (equalise_host(acc.data(), counts.data(), n, 1, eq.data(), err)) return bad("samplesEq 1 was not refused");
    }
    std::printf("adaptive gather ok\n");
    return 0;
}
