// pt_api_render.hip — passes, batches, the ping-pong frames, presentation and readback (include/ptmi_plugin.h Part 2).
#include "pt_context.h"

int ensure_frames(PTContext* c, uint32_t w, uint32_t h)
{
    if (c->frames.w == w && c->frames.h == h) return PT_OK;
    int rc = c->frames.resize(w, h, {sizeof(float4), sizeof(float4)}, nullptr);    // no drain of ours: freeing device memory waits for the device
    if (rc) return rc;
    for (int i = 0; i < 2; i++) HIP_TRY(hipMemsetAsync(c->frames.f4(i), 0, c->frames.buf[i].used, c->stream));
    c->cur = 0;                         // PrepareRenderTexture re-created the targets -> Reset() (PathTracer.cs:211-215)
    return PT_OK;
}

// one arena for all slot-indexed arrays of a wavefront state set (pt_wf_arena_bytes / pt_wf_arena_carve, pt_wavefront.hip);
// re-carved when the slot count changes
int ensure_wavefront(PTContext* c, PTContext::WfSet& set, uint32_t numSlots, uint32_t maxIterations)
{
    int rc;
    if ((rc = create_set_stream((uint32_t)(&set - c->sets), set.stream)) || (rc = create(set.callEv)) || (rc = create(set.done))) return rc;
    const bool needTlas = c->scene.hasTlas != 0u;
    if (set.wf.flags && set.wf.numSlots == numSlots && set.wf.maxIterations >= maxIterations && (!needTlas || set.wf.tlasSpill)) return PT_OK;
    if (c->residentWaves == 0u) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, c->device));
        c->residentWaves = (uint32_t)prop.multiProcessorCount * 4u * 8u;
    }
    // The arena only ever grows: a different slot count (another batch size, another frame size) that fits is a new carving of
    // the same memory -- launches already enqueued on the set's stream keep the pointers they were given and finish first
    // (stream order), so neither a synchronisation nor an allocation lands in a caller's timed region.
    if ((rc = set.arena.reserve(pt_wf_arena_bytes(numSlots, c->residentWaves, needTlas, maxIterations), set.stream))) {
        set.wf = PTWfBuffers{};
        return rc;
    }
    set.wf = pt_wf_arena_carve(set.arena.ptr, numSlots, c->residentWaves, needTlas, maxIterations);
    HIP_TRY(hipMemsetAsync(set.wf.statRows, 0, (size_t)set.wf.numStatRows * 16 * 8, set.stream));
    return PT_OK;
}

int wavefront_limits(const PTFrameParams& p, uint32_t& maxIterations)
{
    const uint32_t spp = p.SamplesPerPass > 1 ? (uint32_t)p.SamplesPerPass : 1u;
    const uint32_t bounces = p.MaxRayBounces > 1u ? p.MaxRayBounces : 1u;
    if (spp > 4095u || bounces > 8191u) return fail(PT_ERR_UNSUPPORTED, "wavefront schedules pack SamplesPerPass <= 4095 and MaxRayBounces <= 8191");
    const uint64_t maxIt = (uint64_t)spp * (bounces + 2u) + 4u;
    maxIterations = (uint32_t)(maxIt > 65536u ? 65536u : maxIt);
    return PT_OK;
}

PTContext::WfSet& next_wavefront_set(PTContext* c, uint32_t* index)
{
    if (c->nextSet >= c->numSets) c->nextSet = 0u;
    const uint32_t k = c->nextSet;
    c->nextSet = (k + 1u) % c->numSets;
    if (index) *index = k;
    return c->sets[k];
}

int enqueue_wavefront(PTContext* c, PTContext::WfSet& set, PTWfLaunch& L, hipEvent_t profStart, hipEvent_t profStop, uint32_t& launches)
{
    L.scene = &c->scene;
    L.buffers = &set.wf;
    L.counters = (unsigned long long*)c->dStats.ptr;
    L.repackStats = L.counters + 16;
    L.fullStats = c->statsLevel > 0;
    L.stream = set.stream;
    L.schedule = effective_schedule(c);
    L.iterationsOverride = c->wfIterations;
    if (c->update.pending) HIP_TRY(hipStreamWaitEvent(set.stream, c->update.done, 0));     // the trace reads the scene before the resolve's wait
    if (profStart) HIP_TRY(hipEventRecord(profStart, set.stream));
    uint32_t n = 0;
    HIP_TRY(pt_launch_wavefront(L, &n));
    launches += n;
    if (profStop) HIP_TRY(hipEventRecord(profStop, set.stream));
    HIP_TRY(hipEventRecord(set.done, set.stream));
    return PT_OK;
}

// The one place where the stream ordering of a list call is written down (the contract is at the declaration, pt_context.h).
// Each chunk is a launch sequence on the next state set and its stream, as a pass is (render_to), ordered after what the caller has
// enqueued on the context stream so far -- its list; for SH probes also the delta lights' records -- and before what it enqueues
// next.  The context stream joins the sets only after the last chunk is enqueued, so the chunks of one call overlap as passes in
// flight do.  Two CALLS do not: the second one's list is ordered after the stream's tail, and that is the first one's join.
// render_to and render_active do NOT go through here, and should not: a pass orders only its resolve behind the context stream
// (orderAfter), joins per sequence and carves every set on the first pass, for measured reasons.
int enqueue_list_chunks(PTContext* c, const PTFrameParams& p, uint64_t count, uint64_t perChunk, uint32_t slotsPerEntry, const char* rangeName,
                        ListChunkFill fill, void* fillArg)
{
    RoctxRange range(rangeName);
    int rc;
    uint32_t maxIterations;
    if ((rc = wavefront_limits(p, maxIterations))) return rc;
    if (count == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t used = 0u;                 // bit k: set k carries a chunk of this call
    static_assert(PT_WF_SETS <= 32, "one bit per state set");
    for (uint64_t first = 0; first < count; first += perChunk) {
        const uint32_t n = (uint32_t)(count - first < perChunk ? count - first : perChunk);
        EventPair ep;
        if (c->profiling && (rc = take_event_pair(c, ep))) return rc;
        uint32_t k;
        PTContext::WfSet& set = next_wavefront_set(c, &k);
        used |= 1u << k;
        const uint32_t numSlots = (n * slotsPerEntry + 255u) & ~255u;
        // the arena only ever grows; a list of another length is a new carving of the same memory (ensure_wavefront)
        if ((rc = ensure_wavefront(c, set, numSlots, maxIterations))) return rc;
        set.wf.slotsPerPass = numSlots;
        PTWfLaunch L = {};
        L.params = &p;
        fill(fillArg, first, n, L);
        // unlike a pass, the WHOLE chain waits for what the context stream holds so far: its init kernel reads the caller's list
        HIP_TRY(hipEventRecord(set.callEv, c->stream));
        HIP_TRY(hipStreamWaitEvent(set.stream, set.callEv, 0));
        uint32_t launches = 0;
        if ((rc = enqueue_wavefront(c, set, L, c->profiling ? ep.start.h : nullptr, c->profiling ? ep.stop.h : nullptr, launches))) return rc;
        if (c->profiling) {
            ep.launches = launches;
            c->pending.push_back(std::move(ep));
        }
    }
    // joined after the last chunk, not per sequence: the chunks of a call overlap.  Consumers of the context stream then see every
    // entry's result (a set that carried several chunks: its last record covers them)
    for (uint32_t k = 0; k < c->numSets; ++k)
        if (used & (1u << k)) HIP_TRY(hipStreamWaitEvent(c->stream, c->sets[k].done, 0));
    return PT_OK;
}

namespace {

// p: imported and validated (import_frame_params).
// `batch`: the passes a launch sequence renders together (count >= 1; batch.seedRoot[0] / currentSample[0] = those of p)
int render_to(PTContext* c, const PTFrameParams& params, float4* dOut, const float4* dAcc, const PTBatch* hostBatch = nullptr)
{
    RoctxRange range("PT pass (enqueue)");
    const PTFrameParams* p = &params;
    int rc;
    PTBatch batch = {};
    if (hostBatch) batch = *hostBatch;
    else { batch.count = 1u; batch.seedRoot[0] = p->RngSeedRoot; batch.currentSample[0] = p->CurrentSample; }
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (!dOut) return fail(PT_ERR_INVALID_ARG, "output buffer == NULL");
    if (p->CurrentSample > 0 && !dAcc) return fail(PT_ERR_INVALID_ARG, "CurrentSample > 0 needs an accumulated frame");
    HIP_TRY(hipSetDevice(c->device));

    const PTTileMap tm = pt_make_tile_map(*p, c->rank, c->world);

    EventPair ep;
    if (c->profiling && (rc = take_event_pair(c, ep))) return rc;
    uint32_t launches = 0;
    const int schedule = effective_schedule(c);
    switch (schedule) {
    case 1:
    case 2:
    case 3:
    case 4: {
        uint32_t maxIterations;
        if ((rc = wavefront_limits(*p, maxIterations))) return rc;
        // A pass may be cut into SUB-FRAMES (PTSetSubFrames): interleaved subsets of the context's 16x16 blocks, each with its own
        // launch sequence on its own state set and stream, all writing the same output frame.  To the kernels a sub-frame is
        // tile ownership (rank + world * j of world * S); to the machine it is what a second pass in flight is -- other kernels to
        // fill the ramp-up and drain of every launch -- without the host having to run ahead of the frame it shows.
        uint32_t S = c->subFrames < 1u ? 1u : c->subFrames;
        if (S > c->numSets) S = c->numSets;
        const bool zeroOnce = c->world > 1 && S > 1u;
        if (zeroOnce) HIP_TRY(hipMemsetAsync(dOut, 0, (size_t)p->OutputWidth * p->OutputHeight * sizeof(float4), c->stream));
        for (uint32_t j = 0; j < S; ++j) {
            const PTTileMap tmj = S == 1u ? tm : pt_make_tile_map(*p, c->rank + c->world * (int)j, c->world * (int)S);
            PTContext::WfSet& set = next_wavefront_set(c);
            // every set IN USE is carved on the FIRST pass of a frame size (a no-op afterwards): a caller that times passes after a
            // short warm-up must not find the allocation of sets it has not reached yet inside its timed region.  Sets beyond
            // PTSetPassesInFlight are never allocated (0.6 GB each at 1080p).
            const uint32_t slotsPerPass = pt_num_slots(tmj);
            if ((uint64_t)slotsPerPass * batch.count > 0x3FFFFFFFull) return fail(PT_ERR_UNSUPPORTED, "batch too large: passes x owned pixels exceeds 2^30 slots");
            if (j == 0u)
                for (uint32_t k = 0; k < c->numSets; ++k) {
                    if ((rc = ensure_wavefront(c, c->sets[k], slotsPerPass * batch.count, maxIterations))) return rc;
                    c->sets[k].wf.slotsPerPass = slotsPerPass;
                }
            // the launch chain runs on the set's own stream; only its resolve (which reads `accumulated` and writes `output`)
            // is ordered after what the caller has enqueued on the context stream so far, the previous pass included
            HIP_TRY(hipEventRecord(set.callEv, c->stream));
            PTWfLaunch L = {};
            L.params = p;
            L.batch = batch;
            L.mapKind = PT_WF_MAP_TILES;
            L.tiles = tmj;
            L.accumulated = dAcc;
            L.output = dOut;
            L.orderAfter = set.callEv;             // only the resolve waits for the caller's stream: the chain before it overlaps the previous pass
            L.zeroOutputFirst = c->world > 1 && !zeroOnce;
            // one EventPair spans the sub-frames: it starts on the first one's stream and stops on the last one's
            if ((rc = enqueue_wavefront(c, set, L, c->profiling && j == 0u ? ep.start.h : nullptr, c->profiling && j + 1u == S ? ep.stop.h : nullptr, launches))) return rc;
            HIP_TRY(hipStreamWaitEvent(c->stream, set.done, 0));          // joined per sequence: consumers of the context stream see the finished frame
        }
        break;
    }
    case 0:
    default:
        if (batch.count != 1u) return fail(PT_ERR_UNSUPPORTED, "internal: the megakernel renders one pass per launch");
        // pixels this context does not own must read as exact zeros (sum over ranks == single-GPU frame)
        if (c->world > 1)
            HIP_TRY(hipMemsetAsync(dOut, 0, (size_t)p->OutputWidth * p->OutputHeight * sizeof(float4), c->stream));
        if (c->profiling) HIP_TRY(hipEventRecord(ep.start, c->stream));
        HIP_TRY(pt_launch_megakernel(c->scene, *p, dAcc, dOut, tm, (unsigned long long*)c->dStats.ptr, c->statsLevel > 0, c->stream));
        if (c->profiling) HIP_TRY(hipEventRecord(ep.stop, c->stream));
        launches = 1;
        break;
    }
    if (c->profiling) {
        ep.launches = launches;
        c->pending.push_back(std::move(ep));
    }
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTRenderPass(PTContext* c, const PTFrameParams* hostParams)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_frames(c, p.OutputWidth, p.OutputHeight))) return rc;
    return render_to(c, p, c->frames.f4(c->cur), c->frames.f4(1 - c->cur));
}

PT_API int PTFlipFrames(PTContext* c) { if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL"); c->cur = 1 - c->cur; return PT_OK; }
PT_API int PTResetFrames(PTContext* c) { if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL"); c->cur = 0; return PT_OK; }

PT_API int PTRenderPassTo(PTContext* c, const PTFrameParams* hostParams, void* dOutput, const void* dAccumulated)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    return render_to(c, p, (float4*)dOutput, (const float4*)dAccumulated);
}

} // extern "C"

// The params array of a batch (PTRenderPassBatchTo, PTRenderPassActiveTo): `first` = pass 0 imported and validated, batch = every
// pass's RngSeedRoot and CurrentSample; the passes may differ in nothing else.
int import_batch(const PTFrameParams* hostParams, int count, PTFrameParams& first, PTBatch& batch)
{
    if (count < 1 || count > PT_MAX_BATCH) return fail(PT_ERR_INVALID_ARG, "count outside 1.." + std::to_string(PT_MAX_BATCH));
    // the host's array has the stride of ITS header (structSize of the first element)
    const uint32_t stride = hostParams->structSize;
    if (stride < PT_FRAME_PARAMS_MIN_SIZE || stride > 4096u) return fail(PT_ERR_INVALID_ARG, "PTFrameParams.structSize is not set");
    PTFrameParams other;
    int rc = import_struct(hostParams, first, PT_FRAME_PARAMS_MIN_SIZE, "PTFrameParams", "params == NULL");
    if (rc) return rc;
    batch = PTBatch{};
    batch.count = (uint32_t)count;
    for (int j = 0; j < count; ++j) {
        const PTFrameParams* hp = (const PTFrameParams*)((const char*)hostParams + (size_t)j * stride);
        if (hp->structSize != stride) return fail(PT_ERR_INVALID_ARG, "every PTFrameParams of a batch must carry the same structSize");
        if ((rc = import_struct(hp, other, PT_FRAME_PARAMS_MIN_SIZE, "PTFrameParams", "params == NULL"))) return rc;
        batch.seedRoot[j] = other.RngSeedRoot;
        batch.currentSample[j] = other.CurrentSample;
        other.RngSeedRoot = first.RngSeedRoot;
        other.CurrentSample = first.CurrentSample;
        if (memcmp(&other, &first, sizeof(first)) != 0)
            return fail(PT_ERR_INVALID_ARG, "the passes of a batch may differ in RngSeedRoot and CurrentSample only (pass " + std::to_string(j) + " differs elsewhere)");
    }
    return validate_params(first);
}

int take_event_pair(PTContext* c, EventPair& ep)
{
    int rc;
    if (c->pending.size() >= 4096) { rc = drain_events(c); if (rc) return rc; }
    if (!c->freeEvents.empty()) { ep = std::move(c->freeEvents.back()); c->freeEvents.pop_back(); }
    else if ((rc = create(ep.start, hipEventDefault)) || (rc = create(ep.stop, hipEventDefault))) return rc;
    return PT_OK;
}

extern "C" {

PT_API int PTRenderPassBatchTo(PTContext* c, const PTFrameParams* hostParams, int count, void* dOutput, const void* dAccumulated)
{
    if (!c || !hostParams) return fail(PT_ERR_INVALID_ARG, "ctx/params == NULL");
    PTFrameParams first;
    PTBatch batch = {};
    int rc = import_batch(hostParams, count, first, batch);
    if (rc) return rc;
    if (count == 1) return render_to(c, first, (float4*)dOutput, (const float4*)dAccumulated);
    if (effective_schedule(c) == 0) {
        // the megakernel writes pixels itself: run the passes one by one, ping-ponging between dOutput and a scratch frame so that the
        // last pass lands in dOutput
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = c->batchScratch.reserve((size_t)first.OutputWidth * first.OutputHeight * sizeof(float4), c->stream))) return rc;
        const float4* acc = (const float4*)dAccumulated;
        for (int j = 0; j < count; ++j) {
            PTFrameParams pj = first;
            pj.RngSeedRoot = batch.seedRoot[j];
            pj.CurrentSample = batch.currentSample[j];
            float4* out = ((count - 1 - j) & 1) ? (float4*)c->batchScratch.ptr : (float4*)dOutput;
            if ((rc = render_to(c, pj, out, acc))) return rc;
            acc = out;
        }
        return PT_OK;
    }
    return render_to(c, first, (float4*)dOutput, (const float4*)dAccumulated, &batch);
}

PT_API int PTRenderPassBatch(PTContext* c, const PTFrameParams* hostParams, int count)
{
    if (!c || !hostParams) return fail(PT_ERR_INVALID_ARG, "ctx/params == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_frames(c, p.OutputWidth, p.OutputHeight))) return rc;
    return PTRenderPassBatchTo(c, hostParams, count, c->frames.f4(c->cur), c->frames.f4(1 - c->cur));
}

PT_API int PTReadback(PTContext* c, float* dst, uint64_t dstFloats)
{
    if (!c || !dst) return fail(PT_ERR_INVALID_ARG, "ctx/dst == NULL");
    if (!c->frames.w) return fail(PT_ERR_INVALID_ARG, "no frame rendered yet");
    uint64_t need = (uint64_t)c->frames.w * c->frames.h * 4;
    if (dstFloats < need) return fail(PT_ERR_INVALID_ARG, "destination too small");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst, c->frames.f4(c->cur), need * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

PT_API int PTPresent(PTContext* c, const PTPresentParams* q, const void* dSrc, void* dDst)
{
    if (!c || !q || !dDst) return fail(PT_ERR_INVALID_ARG, "ctx/params/dst == NULL");
    if (q->OutputWidth == 0 || q->OutputHeight == 0 || (uint64_t)q->OutputWidth * q->OutputHeight > 0x7FFFFFFFull / 4)
        return fail(PT_ERR_INVALID_ARG, "bad presentation size");
    if (!dSrc) {
        if (!c->frames.w) return fail(PT_ERR_INVALID_ARG, "no frame rendered yet");
        if (q->OutputWidth != c->frames.w || q->OutputHeight != c->frames.h) return fail(PT_ERR_INVALID_ARG, "presentation size differs from the rendered frame");
        dSrc = c->frames.f4(c->cur);
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(pt_launch_present(*q, (const float4*)dSrc, (float4*)dDst, c->stream));
    return PT_OK;
}

PT_API int PTPresentToHost(PTContext* c, const PTPresentParams* q, float* dst, uint64_t dstFloats)
{
    if (!c || !q || !dst) return fail(PT_ERR_INVALID_ARG, "ctx/params/dst == NULL");
    const uint64_t need = (uint64_t)q->OutputWidth * q->OutputHeight * 4;
    if (dstFloats < need) return fail(PT_ERR_INVALID_ARG, "destination too small");
    HIP_TRY(hipSetDevice(c->device));
    int rc = c->present.reserve(need * sizeof(float));      // every use of it ends in the synchronise below
    if (rc) return rc;
    if ((rc = PTPresent(c, q, nullptr, c->present.ptr))) return rc;
    HIP_TRY(hipMemcpyAsync(dst, c->present.ptr, need * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

PT_API void* PTGetFramePointer(PTContext* c, int which)
{
    if (!c) return nullptr;
    if (which < 0) return c->frames.f4(c->cur);
    return which < 2 ? c->frames.f4(which) : nullptr;
}

} // extern "C"
