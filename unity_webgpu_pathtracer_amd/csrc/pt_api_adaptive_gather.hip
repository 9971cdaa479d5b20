// pt_api_adaptive_gather.hip — adaptive gathers: more samples only for the receivers whose mean is still noisy (include/ptmi_plugin.h
// Part 19).  Every round is PTGatherIrradiance's own body over a compacted list (gather_irradiance,
// pt_api_gather.hip); the select, fold and equalise kernels are pt_adaptive_gather.hip's.  The host twins are in plugin_exports.cpp
// over adaptive_gather_host.cpp, which also holds the checks shared here.
#include "pt_context.h"
#include "adaptive_gather_rule.h"

namespace {

// Step 2 and the compaction on the context stream, then the four totals back to the host: synchronises.  activeCount == 0: zeros,
// nothing is launched.  totals: survivors, stopped by threshold, by maxSamples, as non-finite.
int run_select(PTContext* c, const ptag::Select& s, const uint32_t* dActive, uint32_t activeCount, const PTIrradiance* dAcc, const PTReceiver* dRecv,
               uint32_t entryCount, uint32_t* dOutActive, PTReceiver* dOutRecv, uint64_t totals[4])
{
    totals[0] = totals[1] = totals[2] = totals[3] = 0;
    if (activeCount == 0u) return PT_OK;
    PTContext::AdaptiveGather& G = c->adaptiveGather;
    const size_t blocks = pt_ag_blocks(activeCount);
    // grown only for a longer list; the kernels that used the old array ran on the context stream
    int rc;
    if ((rc = G.blockCounts.reserve(blocks * 16u + 32u, c->stream)) || (rc = G.totals.reserve(32))) return rc;
    PTAgSelectArgs A = {};
    A.active = dActive; A.acc = (const float4*)dAcc; A.recv = (const float4*)dRecv;
    A.activeCount = activeCount; A.entryCount = entryCount;
    A.n = s.n; A.addSamples = s.addSamples; A.maxSamples = s.maxSamples; A.threshold2 = s.threshold2; A.darkFloor = s.darkFloor;
    A.blockCounts = (uint32_t*)G.blockCounts.ptr;
    A.totals = (uint64_t*)((char*)G.blockCounts.ptr + blocks * 16u);
    A.outActive = dOutActive; A.outRecv = (float4*)dOutRecv;
    HIP_TRY(pt_launch_ag_select(A, c->stream));
    HIP_TRY(hipMemcpyAsync(G.totals.ptr, A.totals, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(totals, G.totals.ptr, 32);
    return PT_OK;
}

// The loop of Part 19 over device arrays; the arguments are checked.  Returns synchronised.
int adaptive_gather(PTContext* c, const PTFrameParams& p1, const PTAdaptiveGather& a, const PTReceiver* dRecv, uint64_t count, PTIrradiance* dOut, uint32_t* dCounts,
                    PTAdaptiveGatherStats* outStats, const char* who)
{
    PTAdaptiveGatherStats st = {};
    if (int rc = check_list_schedule(c, who, "receiver")) return rc;
    if (count == 0) {
        if (outStats) *outStats = st;
        return PT_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    PTContext::AdaptiveGather& G = c->adaptiveGather;
    // grown only for a longer list; a gather that read or wrote the old arrays was joined by the context stream
    int rc;
    if ((rc = G.active[0].reserve(count * 4u, c->stream)) || (rc = G.active[1].reserve(count * 4u, c->stream)) ||
        (rc = G.recv.reserve(count * sizeof(PTReceiver), c->stream)) || (rc = G.result.reserve(count * sizeof(PTIrradiance), c->stream)))
        return rc;
    RoctxRange range("PT adaptive gather");
    const uint32_t entries = (uint32_t)count;
    PTIrradiance* result = (PTIrradiance*)G.result.ptr;
    PTReceiver* compact = (PTReceiver*)G.recv.ptr;
    // round 0: every entry, the caller's list as it is
    uint32_t n = a.minSamples, firstSample = a.firstSample + a.minSamples, cur = 0;
    uint64_t totals[4];
    if ((rc = gather_irradiance(c, p1, dRecv, count, a.firstSample, a.minSamples, result, who))) return rc;
    HIP_TRY(pt_launch_ag_fold(nullptr, entries, entries, result, a.minSamples, 0u, dOut, dCounts, c->stream));
    if ((rc = run_select(c, ptag::make_select(a, n), nullptr, entries, dOut, dRecv, entries, (uint32_t*)G.active[0].ptr, compact, totals))) return rc;
    st.rounds = 1;
    st.samples = count * a.minSamples;
    for (;;) {
        st.stoppedThreshold += totals[1]; st.stoppedMaxSamples += totals[2]; st.stoppedNonFinite += totals[3];
        const uint32_t active = (uint32_t)totals[0];
        if (active == 0u) break;
        const uint32_t* list = (const uint32_t*)G.active[cur].ptr;
        if ((rc = gather_irradiance(c, p1, compact, active, firstSample, a.addSamples, result, who))) return rc;
        HIP_TRY(pt_launch_ag_fold(list, active, entries, result, a.addSamples, n, dOut, dCounts, c->stream));
        n += a.addSamples;
        firstSample += a.addSamples;
        ++st.rounds;
        st.samples += (uint64_t)active * a.addSamples;
        // the emit reads the receivers from the caller's list through the index: the compacted list the gather just read is free
        if ((rc = run_select(c, ptag::make_select(a, n), list, active, dOut, dRecv, entries, (uint32_t*)G.active[cur ^ 1u].ptr, compact, totals))) return rc;
        cur ^= 1u;
    }
    st.maxCount = n;
    if (outStats) *outStats = st;
    return PT_OK;
}

// what opens both variants of the loop, before the context is used
int import_adaptive(const PTFrameParams* hostParams, const PTAdaptiveGather* hostAdaptive, uint64_t count, const char* who, PTFrameParams& p1, PTAdaptiveGather& a)
{
    std::string err;
    if (!ptag::check_adaptive(hostAdaptive, err)) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": " + err);
    if (int rc = import_struct(hostAdaptive, a, sizeof(PTAdaptiveGather), "PTAdaptiveGather", "adaptive == NULL")) return rc;
    if (int rc = import_sampled_params(hostParams, a.minSamples, who, p1)) return rc;
    if (count > ptag::kMaxEntries) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": count = " + std::to_string(count) + " (at most 2^31)");
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTGatherIrradianceAdaptive(PTContext* c, const PTFrameParams* hostParams, const PTAdaptiveGather* hostAdaptive, const PTReceiver* dRecv, uint64_t count,
                                      PTIrradiance* dOut, uint32_t* dCounts, PTAdaptiveGatherStats* outStats)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceAdaptive: ctx == NULL");
    PTFrameParams p1;
    PTAdaptiveGather a;
    if (int rc = import_adaptive(hostParams, hostAdaptive, count, "PTGatherIrradianceAdaptive", p1, a)) return rc;
    if (!dRecv || !dOut) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceAdaptive: receivers/out == NULL");
    if (misaligned(dRecv) || misaligned(dOut) || misaligned(dCounts, 4))
        return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceAdaptive: receivers or out (16 bytes) or counts (4 bytes) misaligned");
    return adaptive_gather(c, p1, a, dRecv, count, dOut, dCounts, outStats, "PTGatherIrradianceAdaptive");
}

PT_API int PTGatherIrradianceAdaptiveHost(PTContext* c, const PTFrameParams* hostParams, const PTAdaptiveGather* hostAdaptive, const PTReceiver* recv, uint64_t count,
                                          PTIrradiance* out, uint32_t* counts, PTAdaptiveGatherStats* outStats)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceAdaptiveHost: ctx == NULL");
    PTFrameParams p1;
    PTAdaptiveGather a;
    if (int rc = import_adaptive(hostParams, hostAdaptive, count, "PTGatherIrradianceAdaptiveHost", p1, a)) return rc;
    if (!recv || !out) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceAdaptiveHost: receivers/out == NULL");
    for (uint64_t i = 0; i < count; ++i)
        if (recv[i].reserved != 0u) return fail(PT_ERR_INVALID_ARG, "PTGatherIrradianceAdaptiveHost: receivers[" + std::to_string(i) + "].reserved != 0");
    PTContext::AdaptiveGather& G = c->adaptiveGather;
    return host_round_trip(c, G.host, recv, count, out, [&](const PTReceiver* dRecv, PTIrradiance* dOut) {
        uint32_t* dCounts = nullptr;
        if (counts && count) {
            if (int rc = G.hostCounts.reserve(count * 4u)) return rc;
            dCounts = (uint32_t*)G.hostCounts.ptr;
        }
        if (int rc = adaptive_gather(c, p1, a, dRecv, count, dOut, dCounts, outStats, "PTGatherIrradianceAdaptiveHost")) return rc;
        if (dCounts) HIP_TRY(hipMemcpyAsync(counts, dCounts, count * 4u, hipMemcpyDeviceToHost, c->stream));      // the round trip's synchronise covers it
        return (int)PT_OK;
    });
}

PT_API int PTSelectReceivers(PTContext* c, const PTAdaptiveGather* hostAdaptive, uint32_t n, const uint32_t* dActive, uint64_t activeCount, const PTIrradiance* dAcc,
                             const PTReceiver* dRecv, uint64_t entryCount, uint32_t* dOutActive, PTReceiver* dOutRecv, uint64_t* survivors, uint64_t* stopped)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTSelectReceivers: ctx == NULL");
    std::string err;
    if (!ptag::check_select(hostAdaptive, n, activeCount, entryCount, err)) return fail(PT_ERR_INVALID_ARG, "PTSelectReceivers: " + err);
    if (!survivors) return fail(PT_ERR_INVALID_ARG, "PTSelectReceivers: survivors == NULL");
    *survivors = 0;
    if (activeCount && (!dAcc || !dRecv || !dOutActive || !dOutRecv)) return fail(PT_ERR_INVALID_ARG, "PTSelectReceivers: accumulated / receivers / outActive / outReceivers == NULL");
    if (misaligned(dActive, 4) || misaligned(dOutActive, 4) || misaligned(dAcc) || misaligned(dRecv) || misaligned(dOutRecv))
        return fail(PT_ERR_INVALID_ARG, "PTSelectReceivers: an index list (4 bytes), accumulated or receivers (16 bytes) misaligned");
    PTAdaptiveGather a;
    if (int rc = import_struct(hostAdaptive, a, sizeof(PTAdaptiveGather), "PTAdaptiveGather", "PTSelectReceivers: adaptive == NULL")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    uint64_t totals[4];
    if (int rc = run_select(c, ptag::make_select(a, n), dActive, (uint32_t)activeCount, dAcc, dRecv, (uint32_t)entryCount, dOutActive, dOutRecv, totals)) return rc;
    *survivors = totals[0];
    if (stopped) { stopped[0] = totals[1]; stopped[1] = totals[2]; stopped[2] = totals[3]; }
    return PT_OK;
}

PT_API int PTFoldIrradiance(PTContext* c, const uint32_t* dActive, uint64_t activeCount, const PTIrradiance* dNew, uint32_t m, uint32_t n, uint64_t entryCount,
                            PTIrradiance* dAcc, uint32_t* dCounts)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTFoldIrradiance: ctx == NULL");
    std::string err;
    if (!ptag::check_fold(m, n, activeCount, entryCount, err)) return fail(PT_ERR_INVALID_ARG, "PTFoldIrradiance: " + err);
    if (activeCount && (!dNew || !dAcc)) return fail(PT_ERR_INVALID_ARG, "PTFoldIrradiance: new / accumulated == NULL");
    if (misaligned(dActive, 4) || misaligned(dCounts, 4) || misaligned(dNew) || misaligned(dAcc))
        return fail(PT_ERR_INVALID_ARG, "PTFoldIrradiance: the index list or counts (4 bytes), new or accumulated (16 bytes) misaligned");
    if (activeCount == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(pt_launch_ag_fold(dActive, (uint32_t)activeCount, (uint32_t)entryCount, dNew, m, n, dAcc, dCounts, c->stream));
    return PT_OK;
}

PT_API int PTEqualiseIrradiance(PTContext* c, const PTIrradiance* dIrr, const uint32_t* dCounts, uint64_t count, uint32_t samplesEq, PTIrradiance* dOut)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTEqualiseIrradiance: ctx == NULL");
    std::string err;
    if (!ptag::check_equalise(samplesEq, count, err)) return fail(PT_ERR_INVALID_ARG, "PTEqualiseIrradiance: " + err);
    if (count && (!dIrr || !dCounts || !dOut)) return fail(PT_ERR_INVALID_ARG, "PTEqualiseIrradiance: irradiance / counts / out == NULL");
    if (misaligned(dCounts, 4) || misaligned(dIrr) || misaligned(dOut))
        return fail(PT_ERR_INVALID_ARG, "PTEqualiseIrradiance: counts (4 bytes), irradiance or out (16 bytes) misaligned");
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(pt_launch_ag_equalise(dIrr, dCounts, (uint32_t)count, samplesEq, dOut, c->stream));
    return PT_OK;
}

} // extern "C"
