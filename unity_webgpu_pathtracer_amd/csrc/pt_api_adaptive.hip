// pt_api_adaptive.hip — adaptive sampling: passes over the active 16x16 blocks only, each block with its own sample count
// (include/ptmi_plugin.h Part 7).
#include "pt_context.h"

#include <algorithm>

namespace {

std::string dims(uint32_t w, uint32_t h) { return std::to_string(w) + "x" + std::to_string(h); }

int need_state(const PTContext* c, const PTFrameParams* p, const char* who)
{
    const PTContext::Adaptive& A = c->adaptive;
    if (!A.live) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": no adaptive state (call PTAdaptiveBegin first)");
    if (p && (p->OutputWidth != A.w || p->OutputHeight != A.h))
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": the adaptive state is " + dims(A.w, A.h) + ", the params say " + dims(p->OutputWidth, p->OutputHeight));
    return PT_OK;
}

// a block this context renders: its own by tile ownership (pt_slot_to_pixel's rule) and with at least one covered pixel
bool renders(const PTContext* c, const PTTileMap& cover, uint32_t bx, uint32_t by)
{
    const uint32_t world = (uint32_t)(c->world > 1 ? c->world : 1);
    return (bx + by) % world == (uint32_t)c->rank && bx * 16u < cover.coverW && by * 16u < cover.coverH;
}

// the ids the next adaptive call renders: the active list, without foreign and uncovered blocks
void rendered_blocks(const PTContext* c, const PTTileMap& cover, std::vector<uint32_t>& out)
{
    const PTContext::Adaptive& A = c->adaptive;
    out.clear();
    auto take = [&](uint32_t id) { if (renders(c, cover, id % A.blocksX, id / A.blocksX)) out.push_back(id); };
    if (A.allActive) for (uint32_t id = 0; id < A.blocksX * A.blocksY; ++id) take(id);
    else for (uint32_t id : A.active) take(id);
}

// the list is stored as given, minus what this context does not render with the coverage of PTAdaptiveBegin's params
int set_active(PTContext* c, const uint32_t* blocks, uint32_t count, uint32_t* kept, const char* who)
{
    PTContext::Adaptive& A = c->adaptive;
    const uint32_t total = A.blocksX * A.blocksY;
    for (uint32_t i = 0; i < count; ++i) {
        if (blocks[i] >= total)
            return fail(PT_ERR_INVALID_ARG, std::string(who) + ": block id " + std::to_string(blocks[i]) + " at index " + std::to_string(i) + " is outside the " + std::to_string(total) + " blocks of the frame");
        if (i > 0u && blocks[i] <= blocks[i - 1u])
            return fail(PT_ERR_INVALID_ARG, std::string(who) + ": block ids must be strictly ascending (" + std::to_string(blocks[i - 1u]) + " then " + std::to_string(blocks[i]) + " at index " + std::to_string(i) + ")");
    }
    PTTileMap cover = {};
    cover.coverW = A.coverW; cover.coverH = A.coverH;
    A.allActive = blocks == nullptr && count == 0u;
    A.active.clear();
    uint32_t n = 0;
    if (A.allActive) {
        for (uint32_t id = 0; id < total; ++id) if (renders(c, cover, id % A.blocksX, id / A.blocksX)) ++n;
    } else {
        for (uint32_t i = 0; i < count; ++i)
            if (renders(c, cover, blocks[i] % A.blocksX, blocks[i] / A.blocksX)) A.active.push_back(blocks[i]);
        n = (uint32_t)A.active.size();
    }
    if (kept) *kept = n;
    return PT_OK;
}

int render_active(PTContext* c, const PTFrameParams* hostParams, int count, float4* dOut, const float4* dAcc, const char* who)
{
    RoctxRange range("PT adaptive pass (enqueue)");
    PTContext::Adaptive& A = c->adaptive;
    PTFrameParams p;
    PTBatch batch = {};
    int rc;
    if (count < 1 || count > PT_MAX_BATCH)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": count " + std::to_string(count) + " outside 1.." + std::to_string(PT_MAX_BATCH));
    if ((rc = import_batch(hostParams, count, p, batch))) return rc;
    if ((rc = need_state(c, &p, who))) return rc;
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    const int schedule = effective_schedule(c);
    if (schedule < 1 || schedule > 3)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": schedule " + std::to_string(schedule) + " has no pass over a block list (schedules 1, 2 and 3 do: PTSetSchedule)");
    if (!dOut) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": output buffer == NULL");
    if ((const float4*)dOut == dAcc) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": dOutput == dAccumulated (inactive pixels are copied from one to the other)");
    uint32_t maxIterations;
    if ((rc = wavefront_limits(p, maxIterations))) return rc;
    const uint64_t m = (uint64_t)(p.SamplesPerPass > 1 ? p.SamplesPerPass : 1) * (uint64_t)count;

    const PTTileMap cover = pt_make_tile_map(p, c->rank, c->world);
    std::vector<uint32_t> ids;
    rendered_blocks(c, cover, ids);
    std::vector<uint2>& table = A.lastTable;
    table.clear();
    A.lastM = 0u;
    bool allZero = true;
    for (uint32_t id : ids) {
        const uint32_t n = A.samples[id];
        if ((uint64_t)n + m > 0xFFFFFFFFull)
            return fail(PT_ERR_INVALID_ARG, std::string(who) + ": block " + std::to_string(id) + " holds " + std::to_string(n) + " samples, " + std::to_string(m) + " more pass 2^32");
        allZero = allZero && n == 0u;
        table.push_back(make_uint2(id, n));
    }
    if (!dAcc && !(A.allActive && allZero)) {
        table.clear();
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": dAccumulated == NULL needs every block active and every sample count 0");
    }
    if ((uint64_t)table.size() * 256u * (uint64_t)count > 0x3FFFFFFFull) {
        table.clear();
        return fail(PT_ERR_UNSUPPORTED, "batch too large: passes x active pixels exceeds 2^30 slots");
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t frameBytes = (size_t)p.OutputWidth * p.OutputHeight * sizeof(float4);
    if (table.empty()) {
        // nothing to render: the frame moves on unchanged (the context stream is ordered after every earlier pass)
        if (dAcc) HIP_TRY(hipMemcpyAsync(dOut, dAcc, frameBytes, hipMemcpyDeviceToDevice, c->stream));
        A.lastM = (uint32_t)m;
        return PT_OK;
    }

    EventPair ep;
    if (c->profiling && (rc = take_event_pair(c, ep))) return rc;
    PTContext::WfSet& set = next_wavefront_set(c);
    const uint32_t slotsPerPass = (uint32_t)table.size() * 256u;
    // the arena only ever grows; a list of another length is a new carving of the same memory (ensure_wavefront)
    if ((rc = ensure_wavefront(c, set, slotsPerPass * (uint32_t)count, maxIterations))) return rc;
    set.wf.slotsPerPass = slotsPerPass;
    // the call's snapshot of {block, sample count}: on the set's stream, before the init kernel.  The kernels never read a counter
    // the host shares between calls -- this call's init may run while the previous call's resolve is still pending.
    if ((rc = set.blockTable.send(table.data(), table.size() * sizeof(uint2), set.stream))) return rc;
    PTWfLaunch L = {};
    L.params = &p;
    L.batch = batch;
    L.mapKind = PT_WF_MAP_LIST;
    L.list.frameBlocksX = A.blocksX;
    L.list.coverW = cover.coverW;
    L.list.coverH = cover.coverH;
    L.list.table = (const uint2*)set.blockTable.dev.ptr;
    L.accumulated = dAcc;
    L.output = dOut;
    HIP_TRY(hipEventRecord(set.callEv, c->stream));
    L.orderAfter = set.callEv;              // as a pass (render_to): only the frame copy and the resolve wait for the caller's stream
    uint32_t launches = 0;
    if ((rc = enqueue_wavefront(c, set, L, c->profiling ? ep.start.h : nullptr, c->profiling ? ep.stop.h : nullptr, launches))) return rc;
    HIP_TRY(hipStreamWaitEvent(c->stream, set.done, 0));
    if (c->profiling) {
        ep.launches = launches;
        c->pending.push_back(std::move(ep));
    }
    for (const uint2& e : table) A.samples[e.x] = e.y + (uint32_t)m;
    A.lastM = (uint32_t)m;
    return PT_OK;
}

int accumulate_active(PTContext* c, const PTFrameParams* hostParams, int count, const void* dOut, const void* dAcc, int ownIndex, const char* who)
{
    PTContext::Adaptive& A = c->adaptive;
    PTContext::Moments& M = c->moments;
    PTFrameParams p;
    if (int rc = import_frame_params(hostParams, p)) return rc;
    if (count < 1 || count > PT_MAX_BATCH)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": count " + std::to_string(count) + " outside 1.." + std::to_string(PT_MAX_BATCH));
    if (int rc = need_state(c, &p, who)) return rc;
    if (!A.moments)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": PTAdaptiveBegin found no moments of " + dims(A.w, A.h) + " with its sample count, so none are tracked");
    if (M.planes.w != A.w || M.planes.h != A.h)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": the moments are " + dims(M.planes.w, M.planes.h) + ", the adaptive state is " + dims(A.w, A.h));
    const uint64_t m = (uint64_t)count * (uint64_t)(p.SamplesPerPass > 1 ? p.SamplesPerPass : 1);
    if (A.lastM == 0u || m != A.lastM)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": describes " + std::to_string(m) + " samples per block, the adaptive call last enqueued added " + std::to_string(A.lastM));
    if (!dOut || !dAcc) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": output / accumulated frame == NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (!A.lastTable.empty()) {
        std::vector<uint2> t(A.lastTable.size());
        for (size_t i = 0; i < t.size(); ++i) {
            const uint64_t n = A.lastTable[i].y;
            const float f = (float)((double)n * (double)(n + m) / (double)m);
            uint32_t bits;
            memcpy(&bits, &f, sizeof(bits));
            t[i] = make_uint2(A.lastTable[i].x, bits);
        }
        if (int rc = A.momentsTable.send(t.data(), t.size() * sizeof(uint2), c->stream)) return rc;
        HIP_TRY(pt_launch_moments_accumulate_blocks((uint32_t)t.size(), (const uint2*)A.momentsTable.dev.ptr, A.w, A.h, (const float4*)dOut, (const float4*)dAcc,
                                                    M.planes.f4(0), M.planes.f4(1), c->stream));
        for (const uint2& e : A.lastTable) { A.obs[e.x] += 1u; A.wsum[e.x] += m; }
    }
    A.lastM = 0u;                   // one observation per call
    M.lastOwn = ownIndex;
    M.lastPtr = ownIndex < 0 ? dOut : nullptr;
    // what the global getters and the k >= 2 checks see: the least converged block this context owns
    uint32_t minObs; uint64_t minSamples;
    if (int rc = adaptive_inv_dof(c, nullptr, &minObs, &minSamples)) return rc;
    M.observations = minObs;
    M.samples = minSamples;
    return PT_OK;
}

} // namespace

int adaptive_inv_dof(PTContext* c, const float** table, uint32_t* minObs, uint64_t* minSamples)
{
    PTContext::Adaptive& A = c->adaptive;
    if (table) *table = nullptr;
    *minObs = c->moments.observations;
    *minSamples = c->moments.samples;
    if (!A.live || !A.moments || A.w != c->moments.planes.w || A.h != c->moments.planes.h) return PT_OK;
    const uint32_t world = (uint32_t)(c->world > 1 ? c->world : 1);
    std::vector<float> inv(A.obs.size());
    bool any = false;
    for (uint32_t id = 0; id < (uint32_t)inv.size(); ++id) {
        const uint32_t k = A.obs[id];
        inv[id] = k > 1u ? (float)(1.0 / ((double)(k - 1u) * (double)A.wsum[id])) : 0.0f;
        if ((id % A.blocksX + id / A.blocksX) % world != (uint32_t)c->rank) continue;
        if (!any || k < *minObs) *minObs = k;
        if (!any || A.wsum[id] < *minSamples) *minSamples = A.wsum[id];
        any = true;
    }
    if (!table) return PT_OK;
    if (int rc = A.invDof.send(inv.data(), inv.size() * sizeof(float), c->stream)) return rc;
    *table = (const float*)A.invDof.dev.ptr;
    return PT_OK;
}

extern "C" {

PT_API int PTAdaptiveBegin(PTContext* c, const PTFrameParams* hostParams, uint32_t currentSample)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTAdaptiveBegin: ctx == NULL");
    PTFrameParams p;
    if (int rc = import_frame_params(hostParams, p)) return rc;
    PTContext::Adaptive& A = c->adaptive;
    const PTTileMap cover = pt_make_tile_map(p, c->rank, c->world);
    A.live = true;
    A.w = p.OutputWidth; A.h = p.OutputHeight;
    A.coverW = cover.coverW; A.coverH = cover.coverH;
    A.blocksX = (A.w + 15u) / 16u; A.blocksY = (A.h + 15u) / 16u;
    const size_t blocks = (size_t)A.blocksX * A.blocksY;
    A.samples.assign(blocks, currentSample);
    A.allActive = true;
    A.active.clear();
    A.lastTable.clear();
    A.lastM = 0u;
    const PTContext::Moments& M = c->moments;
    A.moments = M.planes.w == A.w && M.planes.h == A.h && M.observations >= 1u && M.samples == (uint64_t)currentSample;
    A.obs.assign(A.moments ? blocks : 0u, M.observations);
    A.wsum.assign(A.moments ? blocks : 0u, M.samples);
    return PT_OK;
}

PT_API int PTAdaptiveEnd(PTContext* c)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTAdaptiveEnd: ctx == NULL");
    PTContext::Adaptive& A = c->adaptive;
    A.live = A.moments = false;
    A.w = A.h = A.blocksX = A.blocksY = 0u;
    A.samples.clear(); A.active.clear(); A.obs.clear(); A.wsum.clear(); A.lastTable.clear();
    A.allActive = true;
    A.lastM = 0u;
    return PT_OK;
}

PT_API int PTSetActiveBlocks(PTContext* c, const uint32_t* blocks, uint32_t count, uint32_t* kept)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTSetActiveBlocks: ctx == NULL");
    if (int rc = need_state(c, nullptr, "PTSetActiveBlocks")) return rc;
    if (!blocks && count) return fail(PT_ERR_INVALID_ARG, "PTSetActiveBlocks: blocks == NULL with count " + std::to_string(count));
    if (blocks && count == 0u) {            // an empty list, as opposed to NULL / 0 = every block
        c->adaptive.allActive = false;
        c->adaptive.active.clear();
        if (kept) *kept = 0u;
        return PT_OK;
    }
    return set_active(c, blocks, count, kept, "PTSetActiveBlocks");
}

PT_API int PTSelectActiveBlocks(PTContext* c, const PTAdaptiveSelect* sel, uint32_t* kept)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTSelectActiveBlocks: ctx == NULL");
    if (!sel) return fail(PT_ERR_INVALID_ARG, "PTSelectActiveBlocks: select == NULL");
    if (sel->structSize < sizeof(PTAdaptiveSelect) || sel->structSize > 4096u)
        return fail(PT_ERR_INVALID_ARG, "PTAdaptiveSelect.structSize is " + std::to_string(sel->structSize) + ", must be sizeof(PTAdaptiveSelect) = " + std::to_string(sizeof(PTAdaptiveSelect)) + " of the host's header");
    if (int rc = need_state(c, nullptr, "PTSelectActiveBlocks")) return rc;
    if (sel->dilate > 1u) return fail(PT_ERR_INVALID_ARG, "PTSelectActiveBlocks: dilate " + std::to_string(sel->dilate) + " is neither 0 nor 1");
    if (!(sel->threshold >= 0.0f)) return fail(PT_ERR_INVALID_ARG, "PTSelectActiveBlocks: threshold must be >= 0 (and not NaN)");
    PTContext::Adaptive& A = c->adaptive;
    const PTContext::Moments& M = c->moments;
    const size_t blocks = (size_t)A.blocksX * A.blocksY;
    if (!M.tiles.ptr || M.planes.w != A.w || M.planes.h != A.h || M.tiles.used != blocks * sizeof(float))
        return fail(PT_ERR_INVALID_ARG, "PTSelectActiveBlocks: no noise tile map of " + dims(A.w, A.h) + " (call PTMeasureNoise first)");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float> tiles(blocks);
    HIP_TRY(hipMemcpyAsync(tiles.data(), M.tiles.ptr, blocks * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    auto within = [&](uint32_t id) { return (uint64_t)A.samples[id] + sel->addSamples <= (uint64_t)sel->maxSamples; };
    std::vector<uint8_t> core(blocks, 0), pick(blocks, 0);
    for (uint32_t id = 0; id < blocks; ++id) core[id] = pick[id] = tiles[id] > sel->threshold && within(id);
    if (sel->dilate)
        for (uint32_t id = 0; id < blocks; ++id) {
            if (!core[id]) continue;
            const int bx = (int)(id % A.blocksX), by = (int)(id / A.blocksX);
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = bx + dx, y = by + dy;
                    if (x < 0 || y < 0 || x >= (int)A.blocksX || y >= (int)A.blocksY) continue;
                    const uint32_t q = (uint32_t)y * A.blocksX + (uint32_t)x;
                    if (within(q)) pick[q] = 1;
                }
        }
    std::vector<uint32_t> ids;
    for (uint32_t id = 0; id < blocks; ++id) if (pick[id]) ids.push_back(id);
    if (ids.empty()) {
        A.allActive = false;
        A.active.clear();
        if (kept) *kept = 0u;
        return PT_OK;
    }
    return set_active(c, ids.data(), (uint32_t)ids.size(), kept, "PTSelectActiveBlocks");
}

PT_API int PTGetActiveBlocks(PTContext* c, uint32_t* dst, uint32_t capacity, uint32_t* count)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTGetActiveBlocks: ctx == NULL");
    if (int rc = need_state(c, nullptr, "PTGetActiveBlocks")) return rc;
    PTTileMap cover = {};
    cover.coverW = c->adaptive.coverW; cover.coverH = c->adaptive.coverH;
    std::vector<uint32_t> ids;
    rendered_blocks(c, cover, ids);
    if (count) *count = (uint32_t)ids.size();
    if (dst) {
        if (capacity < ids.size())
            return fail(PT_ERR_INVALID_ARG, "PTGetActiveBlocks: capacity " + std::to_string(capacity) + " is less than the " + std::to_string(ids.size()) + " active blocks");
        std::copy(ids.begin(), ids.end(), dst);
    }
    return PT_OK;
}

PT_API int PTGetBlockSamples(PTContext* c, uint32_t* dst, uint64_t capacity)
{
    if (!c || !dst) return fail(PT_ERR_INVALID_ARG, "PTGetBlockSamples: ctx/dst == NULL");
    if (int rc = need_state(c, nullptr, "PTGetBlockSamples")) return rc;
    const std::vector<uint32_t>& s = c->adaptive.samples;
    if (capacity < s.size())
        return fail(PT_ERR_INVALID_ARG, "PTGetBlockSamples: capacity " + std::to_string(capacity) + " is less than the " + std::to_string(s.size()) + " blocks of the frame");
    std::copy(s.begin(), s.end(), dst);
    return PT_OK;
}

PT_API int PTRenderPassActiveTo(PTContext* c, const PTFrameParams* hostParams, int count, void* dOutput, const void* dAccumulated)
{
    if (!c || !hostParams) return fail(PT_ERR_INVALID_ARG, "PTRenderPassActiveTo: ctx/params == NULL");
    return render_active(c, hostParams, count, (float4*)dOutput, (const float4*)dAccumulated, "PTRenderPassActiveTo");
}

PT_API int PTRenderPassActive(PTContext* c, const PTFrameParams* hostParams, int count)
{
    if (!c || !hostParams) return fail(PT_ERR_INVALID_ARG, "PTRenderPassActive: ctx/params == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    if ((rc = need_state(c, &p, "PTRenderPassActive"))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_frames(c, p.OutputWidth, p.OutputHeight))) return rc;
    return render_active(c, hostParams, count, c->frames.f4(c->cur), c->frames.f4(1 - c->cur), "PTRenderPassActive");
}

PT_API int PTAccumulateMomentsActive(PTContext* c, const PTFrameParams* hostParams, int count)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTAccumulateMomentsActive: ctx == NULL");
    PTFrameParams p;
    if (int rc = import_frame_params(hostParams, p)) return rc;
    if (int rc = need_state(c, &p, "PTAccumulateMomentsActive")) return rc;
    if (c->frames.w != p.OutputWidth || c->frames.h != p.OutputHeight)
        return fail(PT_ERR_INVALID_ARG, "PTAccumulateMomentsActive: the context's frames are " + dims(c->frames.w, c->frames.h) + ", the params say " +
                                            dims(p.OutputWidth, p.OutputHeight) + " (call it after the pass)");
    return accumulate_active(c, hostParams, count, c->frames.f4(c->cur), c->frames.f4(1 - c->cur), c->cur, "PTAccumulateMomentsActive");
}

PT_API int PTAccumulateMomentsActiveTo(PTContext* c, const PTFrameParams* hostParams, int count, const void* dOutput, const void* dAccumulated)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTAccumulateMomentsActiveTo: ctx == NULL");
    return accumulate_active(c, hostParams, count, dOutput, dAccumulated, -1, "PTAccumulateMomentsActiveTo");
}

} // extern "C"
