// adaptive_gather_host.cpp — the host twins of the adaptive gather's steps (include/ptmi_plugin.h Part 19): the rule
// of adaptive_gather_rule.h in plain loops, entry by entry, and the argument checks the context's entry points share with them.
// No GPU involved.
#include "adaptive_gather_rule.h"

#include <cmath>
#include <cstring>

namespace ptag {

bool check_adaptive(const PTAdaptiveGather* a, std::string& err)
{
    if (!a) { err = "adaptive == NULL"; return false; }
    if (a->structSize < sizeof(PTAdaptiveGather) || a->structSize > 4096u) {
        err = "PTAdaptiveGather.structSize is not set (must be sizeof(PTAdaptiveGather) of the host's header)";
        return false;
    }
    if (a->minSamples < 2u || a->minSamples > PT_GATHER_MAX_SAMPLES) { err = "minSamples = " + std::to_string(a->minSamples) + " (2 ... 65536)"; return false; }
    if (a->addSamples < 1u || a->addSamples > PT_GATHER_MAX_SAMPLES) { err = "addSamples = " + std::to_string(a->addSamples) + " (1 ... 65536)"; return false; }
    if (a->maxSamples < a->minSamples || a->maxSamples > kMaxCount) {
        err = "maxSamples = " + std::to_string(a->maxSamples) + " (minSamples = " + std::to_string(a->minSamples) + " ... 16777216)";
        return false;
    }
    if (!(std::isfinite(a->threshold) && a->threshold > 0.0f)) { err = "threshold = " + std::to_string(a->threshold) + " is not finite and positive"; return false; }
    if (!(std::isfinite(a->darkFloor) && a->darkFloor >= 0.0f)) { err = "darkFloor = " + std::to_string(a->darkFloor) + " is not finite and non-negative"; return false; }
    for (uint32_t r : a->reserved)
        if (r) { err = "PTAdaptiveGather.reserved != 0"; return false; }
    return true;
}

static bool check_counts(uint64_t activeCount, uint64_t entryCount, std::string& err)
{
    if (entryCount > kMaxEntries) { err = "entryCount = " + std::to_string(entryCount) + " (at most 2^31)"; return false; }
    if (activeCount > entryCount) { err = "activeCount = " + std::to_string(activeCount) + " > entryCount = " + std::to_string(entryCount); return false; }
    return true;
}

bool check_select(const PTAdaptiveGather* a, uint32_t n, uint64_t activeCount, uint64_t entryCount, std::string& err)
{
    if (!check_adaptive(a, err)) return false;
    if (n < kMinCount || n > kMaxCount) { err = "n = " + std::to_string(n) + " (2 ... 16777216)"; return false; }
    return check_counts(activeCount, entryCount, err);
}

bool check_fold(uint32_t m, uint32_t n, uint64_t activeCount, uint64_t entryCount, std::string& err)
{
    if (m < 1u || m > PT_GATHER_MAX_SAMPLES) { err = "m = " + std::to_string(m) + " (1 ... 65536)"; return false; }
    if (n > kMaxCount || n + m > kMaxCount) { err = "n + m = " + std::to_string((uint64_t)n + m) + " (at most 16777216)"; return false; }
    return check_counts(activeCount, entryCount, err);
}

bool check_equalise(uint32_t samplesEq, uint64_t count, std::string& err)
{
    if (samplesEq < kMinCount || samplesEq > kMaxCount) { err = "samplesEq = " + std::to_string(samplesEq) + " (2 ... 16777216)"; return false; }
    if (count > kMaxEntries) { err = "count = " + std::to_string(count) + " (at most 2^31)"; return false; }
    return true;
}

static bool check_indices(const uint32_t* active, uint64_t activeCount, uint64_t entryCount, std::string& err)
{
    if (active)
        for (uint64_t k = 0; k < activeCount; ++k)
            if (active[k] >= entryCount) { err = "active[" + std::to_string(k) + "] = " + std::to_string(active[k]) + " >= entryCount"; return false; }
    return true;
}

bool select_host(const PTAdaptiveGather* a, uint32_t n, const uint32_t* active, uint64_t activeCount, const PTIrradiance* acc, const PTReceiver* recv,
                 uint64_t entryCount, uint32_t* outActive, PTReceiver* outRecv, uint64_t* survivors, uint64_t* stopped, std::string& err)
{
    if (!check_select(a, n, activeCount, entryCount, err)) return false;
    if (!survivors) { err = "survivors == NULL"; return false; }
    *survivors = 0;
    if (activeCount && (!acc || !recv || !outActive || !outRecv)) { err = "accumulated / receivers / outActive / outReceivers == NULL"; return false; }
    if (!check_indices(active, activeCount, entryCount, err)) return false;
    const Select s = make_select(*a, n);
    uint64_t kept = 0, why[4] = {0, 0, 0, 0};
    for (uint64_t k = 0; k < activeCount; ++k) {
        const uint32_t i = active ? active[k] : (uint32_t)k;
        const float e[4] = {acc[i].rgb[0], acc[i].rgb[1], acc[i].rgb[2], acc[i].m2};
        const uint32_t r = select_entry(s, e);
        ++why[r];
        if (r != kActive) continue;
        outActive[kept] = i;
        memmove(&outRecv[kept], &recv[i], sizeof(PTReceiver));
        ++kept;
    }
    *survivors = kept;
    if (stopped) { stopped[0] = why[kByThreshold]; stopped[1] = why[kByMaxSamples]; stopped[2] = why[kNonFinite]; }
    return true;
}

bool fold_host(const uint32_t* active, uint64_t activeCount, const PTIrradiance* fresh, uint32_t m, uint32_t n, uint64_t entryCount, PTIrradiance* acc,
               uint32_t* counts, std::string& err)
{
    if (!check_fold(m, n, activeCount, entryCount, err)) return false;
    if (activeCount && (!fresh || !acc)) { err = "new / accumulated == NULL"; return false; }
    if (!check_indices(active, activeCount, entryCount, err)) return false;
    for (uint64_t k = 0; k < activeCount; ++k) {
        const uint32_t i = active ? active[k] : (uint32_t)k;
        if (n == 0u) {
            memmove(&acc[i], &fresh[k], sizeof(PTIrradiance));
        } else {
            float e[4] = {acc[i].rgb[0], acc[i].rgb[1], acc[i].rgb[2], acc[i].m2};
            const float f[4] = {fresh[k].rgb[0], fresh[k].rgb[1], fresh[k].rgb[2], fresh[k].m2};
            fold_entry(e, n, f, m);
            acc[i] = PTIrradiance{{e[0], e[1], e[2]}, e[3]};
        }
        if (counts) counts[i] = n + m;
    }
    return true;
}

bool equalise_host(const PTIrradiance* irr, const uint32_t* counts, uint64_t count, uint32_t samplesEq, PTIrradiance* out, std::string& err)
{
    if (!check_equalise(samplesEq, count, err)) return false;
    if (count && (!irr || !counts || !out)) { err = "irradiance / counts / out == NULL"; return false; }
    for (uint64_t i = 0; i < count; ++i) {
        const float e[4] = {irr[i].rgb[0], irr[i].rgb[1], irr[i].rgb[2], irr[i].m2};
        float m2;
        const bool rewritten = equalise_entry(e, counts[i], samplesEq, m2);
        memmove(&out[i], &irr[i], sizeof(PTIrradiance));
        if (rewritten) out[i].m2 = m2;
    }
    return true;
}

} // namespace ptag
