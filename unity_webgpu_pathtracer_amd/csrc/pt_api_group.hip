// pt_api_group.hip — tile pack / unpack and the one-process multi-device group (no reference counterpart).
#include "pt_context.h"

#include <thread>

namespace {

// runs fn(i) for every device of the group, device 0 on the calling thread and the others on one thread each (a pass is
// ~160 launches per device: enqueued serially, eight devices would be host-bound); the first error is re-raised here
template <class F>
int for_each_device(PTGroup* g, F fn)
{
    const size_t n = g->dev.size();
    std::vector<int> rcs(n, PT_OK);
    std::vector<std::string> msgs(n);
    std::vector<std::thread> workers;
    for (size_t i = 1; i < n; ++i)
        workers.emplace_back([&, i] { rcs[i] = fn((int)i); if (rcs[i]) msgs[i] = g_lastError; });
    rcs[0] = fn(0);
    if (rcs[0]) msgs[0] = g_lastError;
    for (auto& w : workers) w.join();
    for (size_t i = 0; i < n; ++i)
        if (rcs[i]) return fail(rcs[i], "device " + std::to_string(g->dev[i].ctx->device) + " (rank " + std::to_string(i) + "): " + msgs[i]);
    return PT_OK;
}

int group_ensure_buffers(PTGroup* g, const PTFrameParams& p)
{
    PTContext* root = g->dev[0].ctx;
    int rc;
    if (g->assembled.w != p.OutputWidth || g->assembled.h != p.OutputHeight) {
        HIP_TRY(hipSetDevice(root->device));
        if ((rc = g->assembled.resize(p.OutputWidth, p.OutputHeight, {sizeof(float4)}, root->stream))) return rc;
        HIP_TRY(hipMemsetAsync(g->assembled.f4(0), 0, g->assembled.buf[0].used, root->stream));
    }
    for (size_t i = 0; i < g->dev.size(); ++i) {
        PTGroup::Dev& d = g->dev[i];
        const size_t need = (size_t)pt_num_slots(pt_make_tile_map(p, (int)i, (int)g->dev.size())) * sizeof(float4);
        if (d.packed.bytes >= need) continue;
        HIP_TRY(hipSetDevice(d.ctx->device));
        if ((rc = d.packed.reserve(need, d.ctx->stream))) return rc;
        if (i > 0) {
            HIP_TRY(hipSetDevice(root->device));
            if ((rc = d.staged.reserve(need, root->stream))) return rc;
        }
    }
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTGetOwnedTileSlots(PTContext* c, const PTFrameParams* hostParams, uint64_t* out)
{
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "ctx/out == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    *out = pt_num_slots(pt_make_tile_map(p, c->rank, c->world));
    return PT_OK;
}

PT_API int PTPackOwnedTiles(PTContext* c, const PTFrameParams* hostParams, const void* dFrame, void* dPacked)
{
    if (!c || !dFrame || !dPacked) return fail(PT_ERR_INVALID_ARG, "ctx/frame/packed == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(pt_launch_pack_tiles(pt_make_tile_map(p, c->rank, c->world), p.OutputWidth, (const float4*)dFrame, (float4*)dPacked, c->stream));
    return PT_OK;
}

PT_API int PTUnpackTiles(PTContext* c, const PTFrameParams* hostParams, int rank, int world, const void* dPacked, void* dFrame)
{
    if (!c || !dFrame || !dPacked) return fail(PT_ERR_INVALID_ARG, "ctx/frame/packed == NULL");
    if (world < 1 || rank < 0 || rank >= world) return fail(PT_ERR_INVALID_ARG, "bad rank/worldSize");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(pt_launch_unpack_tiles(pt_make_tile_map(p, rank, world), p.OutputWidth, (const float4*)dPacked, (float4*)dFrame, c->stream));
    return PT_OK;
}

PT_API int PTGroupDestroy(PTGroup* g)
{
    if (!g) return PT_OK;
    for (PTGroup::Dev& d : g->dev) {
        hipSetDevice(d.ctx->device);
        hipStreamSynchronize(d.ctx->stream);
    }
    std::vector<PTContext*> ctx;
    for (PTGroup::Dev& d : g->dev) ctx.push_back(d.ctx);
    if (!ctx.empty()) { hipSetDevice(ctx[0]->device); hipStreamSynchronize(ctx[0]->stream); }
    delete g;                                       // the group's buffers and events go before the contexts they were used with
    for (PTContext* c : ctx) PTDestroy(c);
    return PT_OK;
}

PT_API int PTCreateMulti(const int* devices, int n, PTGroup** out)
{
    if (!out) return fail(PT_ERR_INVALID_ARG, "outGroup == NULL");
    *out = nullptr;
    if (!devices || n < 1 || n > 64) return fail(PT_ERR_INVALID_ARG, "deviceIndices == NULL or deviceCount outside 1..64");
    PTGroup* g = new PTGroup();
    for (int i = 0; i < n; ++i) {
        PTContext* c = nullptr;
        int rc = PTCreate(devices[i], &c);
        if (rc == PT_OK) rc = PTSetTileOwnership(c, i, n);
        if (rc != PT_OK) {
            const std::string msg = g_lastError;
            if (c) PTDestroy(c);
            PTGroupDestroy(g);
            return fail(rc, msg);
        }
        g->dev.emplace_back();
        g->dev.back().ctx = c;
    }
    for (PTGroup::Dev& d : g->dev) {
        hipSetDevice(g->dev[0].ctx->device);
        if (hipEventCreateWithFlags(&d.unpacked.h, hipEventDisableTiming) != hipSuccess) { PTGroupDestroy(g); return fail(PT_ERR_HIP, "hipEventCreate failed"); }
        hipSetDevice(d.ctx->device);
        if (hipEventCreateWithFlags(&d.arrived.h, hipEventDisableTiming) != hipSuccess) { PTGroupDestroy(g); return fail(PT_ERR_HIP, "hipEventCreate failed"); }
        // direct xGMI copies into the root's staging buffers; "already enabled" / "not supported" leave the staged path
        if (d.ctx->device != g->dev[0].ctx->device) { (void)hipDeviceEnablePeerAccess(g->dev[0].ctx->device, 0); (void)hipGetLastError(); }
    }
    *out = g;
    return PT_OK;
}

PT_API int PTGroupSize(PTGroup* g) { return g ? (int)g->dev.size() : fail(PT_ERR_INVALID_ARG, "group == NULL"); }
PT_API PTContext* PTGroupGetContext(PTGroup* g, int i) { return (g && i >= 0 && i < (int)g->dev.size()) ? g->dev[i].ctx : nullptr; }

PT_API int PTGroupSetScene(PTGroup* g, const PTSceneDesc* scene)
{
    if (!g) return fail(PT_ERR_INVALID_ARG, "group == NULL");
    // the index validation walks the whole scene on the host: once for the group, not once per device
    int rc = set_scene(g->dev[0].ctx, scene, true);
    if (rc) return rc;
    return for_each_device(g, [&](int i) { return i == 0 ? PT_OK : set_scene(g->dev[i].ctx, scene, false); });
}

PT_API int PTGroupRenderPassBatch(PTGroup* g, const PTFrameParams* hostParams, int count)
{
    if (!g) return fail(PT_ERR_INVALID_ARG, "group == NULL");
    PTFrameParams p;
    int rc = import_frame_params(hostParams, p);
    if (rc) return rc;
    if ((rc = group_ensure_buffers(g, p))) return rc;
    PTContext* root = g->dev[0].ctx;
    const int world = (int)g->dev.size();
    rc = for_each_device(g, [&](int i) -> int {
        PTGroup::Dev& d = g->dev[i];
        PTContext* c = d.ctx;
        int r = count == 1 ? PTRenderPass(c, hostParams) : PTRenderPassBatch(c, hostParams, count);   // owned tiles into the device's own ping-pong frames
        if (r) return r;
        // staged (and the root's packed, which the root unpacks in place) may only be overwritten once the root has scattered the
        // previous pass's tiles out of it: a straggling root must not see tiles of pass k+1 in the assembled frame of pass k
        if (d.unpackedValid) HIP_TRY(hipStreamWaitEvent(c->stream, d.unpacked, 0));
        HIP_TRY(pt_launch_pack_tiles(pt_make_tile_map(p, i, world), p.OutputWidth, c->frames.f4(c->cur), (float4*)d.packed.ptr, c->stream));
        if (i > 0) HIP_TRY(hipMemcpyPeerAsync(d.staged.ptr, root->device, d.packed.ptr, c->device, d.packed.bytes, c->stream));
        HIP_TRY(hipEventRecord(d.arrived, c->stream));
        return PT_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipSetDevice(root->device));
    for (int i = 0; i < world; ++i) {
        PTGroup::Dev& d = g->dev[i];
        if (i > 0) HIP_TRY(hipStreamWaitEvent(root->stream, d.arrived, 0));
        HIP_TRY(pt_launch_unpack_tiles(pt_make_tile_map(p, i, world), p.OutputWidth, d.tiles(), g->assembled.f4(0), root->stream));
        HIP_TRY(hipEventRecord(d.unpacked, root->stream));
        d.unpackedValid = true;
    }
    return PT_OK;
}

PT_API int PTGroupRenderPass(PTGroup* g, const PTFrameParams* hostParams) { return PTGroupRenderPassBatch(g, hostParams, 1); }

PT_API int PTGroupFlipFrames(PTGroup* g)
{
    if (!g) return fail(PT_ERR_INVALID_ARG, "group == NULL");
    for (PTGroup::Dev& d : g->dev) PTFlipFrames(d.ctx);
    return PT_OK;
}

PT_API int PTGroupResetFrames(PTGroup* g)
{
    if (!g) return fail(PT_ERR_INVALID_ARG, "group == NULL");
    for (PTGroup::Dev& d : g->dev) PTResetFrames(d.ctx);
    return PT_OK;
}

PT_API int PTGroupSynchronize(PTGroup* g)
{
    if (!g) return fail(PT_ERR_INVALID_ARG, "group == NULL");
    for (size_t i = g->dev.size(); i-- > 0;) { int rc = PTSynchronize(g->dev[i].ctx); if (rc) return rc; }   // the root last: it waits for the others
    return PT_OK;
}

PT_API int PTGroupReadback(PTGroup* g, float* dst, uint64_t dstFloats)
{
    if (!g || !dst) return fail(PT_ERR_INVALID_ARG, "group/dst == NULL");
    if (!g->assembled.w) return fail(PT_ERR_INVALID_ARG, "no frame rendered yet");
    const uint64_t need = (uint64_t)g->assembled.w * g->assembled.h * 4;
    if (dstFloats < need) return fail(PT_ERR_INVALID_ARG, "destination too small");
    PTContext* root = g->dev[0].ctx;
    HIP_TRY(hipSetDevice(root->device));
    HIP_TRY(hipMemcpyAsync(dst, g->assembled.f4(0), need * sizeof(float), hipMemcpyDeviceToHost, root->stream));
    HIP_TRY(hipStreamSynchronize(root->stream));
    return PT_OK;
}

PT_API void* PTGroupGetAssembledFrame(PTGroup* g) { return g ? (void*)g->assembled.f4(0) : nullptr; }

PT_API int PTGroupGetStats(PTGroup* g, PTStats* out)
{
    if (!g || !out) return fail(PT_ERR_INVALID_ARG, "group/out == NULL");
    uint64_t acc[16] = {};
    for (PTGroup::Dev& d : g->dev) {
        PTStats st;
        int rc = PTGetStats(d.ctx, &st);
        if (rc) return rc;
        const uint64_t* v = (const uint64_t*)&st;
        for (int k = 0; k < 16; ++k) { if (k == 12) acc[k] = v[k] > acc[k] ? v[k] : acc[k]; else acc[k] += v[k]; }
    }
    memcpy(out, acc, sizeof(PTStats));
    return PT_OK;
}

PT_API int PTGroupResetStats(PTGroup* g)
{
    if (!g) return fail(PT_ERR_INVALID_ARG, "group == NULL");
    for (PTGroup::Dev& d : g->dev) { int rc = PTResetStats(d.ctx); if (rc) return rc; }
    return PT_OK;
}

} // extern "C"
