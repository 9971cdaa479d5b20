// adaptive_gather_rule.h — adaptive gathers (include/ptmi_plugin.h Part 19): the one definition of the rule, shared
// by the kernels (pt_adaptive_gather.hip) and the host twins (adaptive_gather_host.cpp).  Every fp32 operator is one IEEE binary32
// operation, left to right as written, and both sides are compiled with -ffp-contract=off, so both give the same bits.  The rule
// uses only + - * /, max (fmaxf) and comparisons.  tests/adaptive_gather_ref.py restates it in numpy from this text.
//
//  1. Rounds.  Round 0 gathers the samples [firstSample, firstSample + minSamples) of every entry; round r >= 1 gathers
//     [firstSample + minSamples + (r - 1) * addSamples, ... + addSamples) of the entries still active (uint32 arithmetic).  Each
//     round is PTGatherIrradiance over the active entries' receivers, their 32 bytes copied unchanged.  An entry that is dropped
//     stays dropped, so every active entry of a round holds the same count n.
//  2. Select, for an active entry with accumulated (rgb, m2) and count n:
//       S = (float)n;  l = (rgb.r * 0.299f + rgb.g * 0.587f) + rgb.b * 0.114f  (luminance3);
//       v = max(((m2 - (S * l) * l) / (S - 1.0f)), 0.0f) / S  (lmfilter_rule.h's step 1);
//       d = max(l, darkFloor);  noisy = v > (threshold * threshold) * (d * d).
//     In this order: rgb or m2 not finite -> stops, NON-FINITE; not noisy (a NaN v compares false) -> stops, BY THRESHOLD;
//     n + addSamples > maxSamples -> stops, BY MAXSAMPLES; otherwise the entry stays ACTIVE.
//     The next active list is the surviving indices in the order of the list they were selected from: a stable compaction.
//  3. Fold of (rgb_new, m2_new) of m samples into (rgb, m2) of n samples, n >= 1:
//       rgb'[c] = (rgb[c] * (float)n + rgb_new[c] * (float)m) / (float)(n + m);  m2' = m2 + m2_new;  n' = n + m.
//     n == 0 writes: (rgb', m2') = (rgb_new, m2_new), bit for bit.
//  4. Result: the accumulated entries and their counts.
//  5. Equalise to samplesEq, with l and v of step 2 from (rgb, m2, n_i) and S = (float)samplesEq:
//       out.rgb = rgb;  out.m2 = (S * l) * l + (v * S) * (S - 1.0f).
//     An entry with a non-finite rgb or m2, or with n_i outside 2 ... 2^24, passes through byte for byte.  This rewrites m2 so
//     that step 1 of lmfilter_rule.h at samples = samplesEq recovers v; it is not new statistics.
//
// The stop decision uses the samples it stops on, so the estimate is slightly biased towards stopping early: among equally noisy
// entries, those whose first samples happen to agree stop first.  minSamples is the guard.
#pragma once
#include <stdint.h>
#include <string>
#include "ptmi_math.h"
#include "ptmi_plugin.h"

#if defined(__HIPCC__)
#define PT_AG_HD __host__ __device__ __forceinline__
#else
#define PT_AG_HD inline
#endif

namespace ptag {

constexpr uint32_t kMinCount = 2u, kMaxCount = PT_ADAPTIVE_GATHER_MAX_TOTAL;
constexpr uint64_t kMaxEntries = PT_ADAPTIVE_GATHER_MAX_ENTRIES;
// what step 2 makes of an entry; kLeftOut: no entry (past the list, or an index the arrays do not hold)
constexpr uint32_t kActive = 0u, kByThreshold = 1u, kByMaxSamples = 2u, kNonFinite = 3u, kLeftOut = 4u;

// step 2's parameters as the rule uses them
struct Select {
    uint32_t n, addSamples, maxSamples;
    float threshold2, darkFloor;             // threshold2 = threshold * threshold
};

PT_AG_HD Select make_select(const PTAdaptiveGather& a, uint32_t n) { return Select{n, a.addSamples, a.maxSamples, a.threshold * a.threshold, a.darkFloor}; }

PT_AG_HD bool finite(float x) { return pt_abs(x) <= 3.402823466e38f; }

PT_AG_HD float luminance(const float e[3]) { return (e[0] * 0.299f + e[1] * 0.587f) + e[2] * 0.114f; }

// the variance of the mean luminance behind an entry of n samples
PT_AG_HD float variance_of_mean(float l, float m2, uint32_t n)
{
    const float S = (float)n;
    return pt_max((m2 - (S * l) * l) / (S - 1.0f), 0.0f) / S;
}

// step 2 for one entry (rgb, m2)
PT_AG_HD uint32_t select_entry(const Select& s, const float e[4])
{
    if (!(finite(e[0]) && finite(e[1]) && finite(e[2]) && finite(e[3]))) return kNonFinite;
    const float l = luminance(e);
    const float v = variance_of_mean(l, e[3], s.n);
    const float d = pt_max(l, s.darkFloor);
    const bool noisy = v > s.threshold2 * (d * d);
    if (!noisy) return kByThreshold;
    return s.n + s.addSamples > s.maxSamples ? kByMaxSamples : kActive;
}

// step 3, n >= 1
PT_AG_HD void fold_entry(float acc[4], uint32_t n, const float fresh[4], uint32_t m)
{
    const float fn = (float)n, fm = (float)m, ft = (float)(n + m);
    acc[0] = (acc[0] * fn + fresh[0] * fm) / ft;
    acc[1] = (acc[1] * fn + fresh[1] * fm) / ft;
    acc[2] = (acc[2] * fn + fresh[2] * fm) / ft;
    acc[3] = acc[3] + fresh[3];
}

// step 5.  false: the entry passes through byte for byte (m2 is not touched)
PT_AG_HD bool equalise_entry(const float e[4], uint32_t n, uint32_t samplesEq, float& m2)
{
    if (!(finite(e[0]) && finite(e[1]) && finite(e[2]) && finite(e[3])) || n < kMinCount || n > kMaxCount) return false;
    const float l = luminance(e);
    const float v = variance_of_mean(l, e[3], n);
    const float S = (float)samplesEq;
    m2 = (S * l) * l + (v * S) * (S - 1.0f);
    return true;
}

// ---- host side (adaptive_gather_host.cpp) ----
// The checks the context's entry points share with the twins.  false: err has the reason.
bool check_adaptive(const PTAdaptiveGather* a, std::string& err);
bool check_select(const PTAdaptiveGather* a, uint32_t n, uint64_t activeCount, uint64_t entryCount, std::string& err);
bool check_fold(uint32_t m, uint32_t n, uint64_t activeCount, uint64_t entryCount, std::string& err);
bool check_equalise(uint32_t samplesEq, uint64_t count, std::string& err);
// The steps on the host.  false: err has the reason (the checks above, a NULL array, an index >= entryCount).
bool select_host(const PTAdaptiveGather* a, uint32_t n, const uint32_t* active, uint64_t activeCount, const PTIrradiance* acc, const PTReceiver* recv,
                 uint64_t entryCount, uint32_t* outActive, PTReceiver* outRecv, uint64_t* survivors, uint64_t* stopped, std::string& err);
bool fold_host(const uint32_t* active, uint64_t activeCount, const PTIrradiance* fresh, uint32_t m, uint32_t n, uint64_t entryCount, PTIrradiance* acc,
               uint32_t* counts, std::string& err);
bool equalise_host(const PTIrradiance* irr, const uint32_t* counts, uint64_t count, uint32_t samplesEq, PTIrradiance* out, std::string& err);

} // namespace ptag
