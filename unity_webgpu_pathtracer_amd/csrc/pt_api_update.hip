// pt_api_update.hip — scene updates and PTReadTLAS (include/ptmi_plugin.h Part 5).
#include "pt_context.h"

#include <algorithm>
#include <cmath>

namespace {

size_t al256(size_t b) { return (b + 255) / 256 * 256; }
// one instance generation: raw TLAS ((2n - 1) nodes, then n indices), breadth-first copy, PTGpuInstance records, instByLeaf
size_t inst_raw_bytes(uint32_t n) { return al256(((size_t)2 * n - 1) * 64 + (size_t)n * 4); }
size_t inst_gen_bytes(uint32_t n) { return inst_raw_bytes(n) + al256(((size_t)2 * n - 1) * 64) + al256((size_t)n * 144) + al256((size_t)n * 96); }
struct InstGen { float* raw; float* bfs; float* inst; float* byLeaf; };
InstGen inst_gen(void* base, uint32_t n)
{
    char* p = (char*)base;
    InstGen g;
    g.raw = (float*)p; p += inst_raw_bytes(n);
    g.bfs = (float*)p; p += al256(((size_t)2 * n - 1) * 64);
    g.inst = (float*)p; p += al256((size_t)n * 144);
    g.byLeaf = (float*)p;
    return g;
}

} // namespace

// Opens an update of group g.  The update stream and both generations exist afterwards: their sizes depend on the scene alone and
// PTSetScene discards the groups, so after a group's first update nothing is reallocated.  The generation an update writes is
// not the current one; the update stream first waits until every piece of work that read it (enqueued before it stopped
// being current) has finished.
int begin_update(PTContext* c, PTContext::UpdGroup& g, size_t genBytes, size_t stagingBytes, int& target)
{
    PTContext::Update& u = c->update;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = create(u.stream)) || (rc = create(u.done)) || (rc = create(u.input))) return rc;
    for (int k = 0; k < 2; ++k) {
        if ((rc = g.gen[k].reserve(genBytes)) || (rc = create(g.freeEv[k])) || (rc = create(g.stagedEv[k]))) return rc;
        if (stagingBytes && (rc = g.staging[k].reserve(stagingBytes))) return rc;
    }
    target = g.cur == 0 ? 1 : 0;
    if (g.freeRecorded[target]) HIP_TRY(hipStreamWaitEvent(u.stream, g.freeEv[target], 0));
    return PT_OK;
}

// host array -> pinned staging of `target` -> device, on the update stream; waits only for that staging buffer's last copy
int stage_host(PTContext* c, PTContext::UpdGroup& g, int target, const void* src, size_t bytes, void* dst)
{
    if (g.stagedRecorded[target]) HIP_TRY(hipEventSynchronize(g.stagedEv[target]));
    memcpy(g.staging[target].ptr, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, g.staging[target].ptr, bytes, hipMemcpyHostToDevice, c->update.stream));
    HIP_TRY(hipEventRecord(g.stagedEv[target], c->update.stream));
    g.stagedRecorded[target] = true;
    return PT_OK;
}

// the written generation becomes current: work enqueued from now on (passes on their set streams, the context stream's
// queries, guides and resolves) waits for the update; the previous generation is free once the context stream reaches here
int end_update(PTContext* c, PTContext::UpdGroup& g, int target)
{
    if (g.cur >= 0) {
        HIP_TRY(hipEventRecord(g.freeEv[g.cur], c->stream));
        g.freeRecorded[g.cur] = true;
    }
    g.cur = target;
    HIP_TRY(hipEventRecord(c->update.done, c->update.stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->update.done, 0));
    c->update.pending = true;
    return PT_OK;
}

namespace {

bool finite_record(const PTBlasInstance& r)
{
    for (float v : r.localToWorld) if (!std::isfinite(v)) return false;
    for (float v : r.worldToLocal) if (!std::isfinite(v)) return false;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(r.aabbMin[k]) || !std::isfinite(r.aabbMax[k])) return false;
    return true;
}

int update_instances(PTContext* c, const PTBlasInstance* src, uint32_t count, bool onDevice)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!src) return fail(PT_ERR_INVALID_ARG, "instances == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (!c->scene.hasTlas) return fail(PT_ERR_UNSUPPORTED, "instance updates need a HAS_TLAS scene");
    PTContext::Update& u = c->update;
    const uint32_t n = u.instanceCount;
    if (count != n) return fail(PT_ERR_INVALID_ARG, "count (" + std::to_string(count) + ") != the scene's instanceCount (" + std::to_string(n) + ")");
    if (!onDevice)
        for (uint32_t i = 0; i < n; ++i)
            if (!finite_record(src[i])) return fail(PT_ERR_INVALID_ARG, "instance " + std::to_string(i) + ": non-finite matrix or AABB");
    PTContext::UpdGroup& g = u.inst;
    const bool fresh = g.gen[0].ptr == nullptr;
    int rc, target;
    if ((rc = begin_update(c, g, inst_gen_bytes(n), onDevice ? 0 : (size_t)n * sizeof(PTBlasInstance), target))) return rc;
    if (!u.tlasWork.ptr) {
        if ((rc = u.tlasWork.reserve(pt_tlas_work_bytes(n)))) return rc;
        u.tlasW = pt_tlas_carve(u.tlasWork.ptr, n);
    }
    if (fresh)                                      // the offsets rows of both generations: PTSetScene's records
        for (int k = 0; k < 2; ++k)
            HIP_TRY(hipMemcpyAsync(inst_gen(g.gen[k].ptr, n).inst, c->instances.ptr, (size_t)n * 144, hipMemcpyDeviceToDevice, u.stream));
    const size_t inBytes = (size_t)n * sizeof(PTBlasInstance);
    if (onDevice) {
        HIP_TRY(hipEventRecord(u.input, c->stream));
        HIP_TRY(hipStreamWaitEvent(u.stream, u.input, 0));
        HIP_TRY(hipMemcpyAsync(u.tlasW.input, src, inBytes, hipMemcpyDeviceToDevice, u.stream));
    } else if ((rc = stage_host(c, g, target, src, inBytes, u.tlasW.input))) {
        return rc;
    }
    const InstGen G = inst_gen(g.gen[target].ptr, n);
    HIP_TRY(pt_launch_tlas_update(u.tlasW, u.tlasW.input, G.raw, G.bfs, G.byLeaf, G.inst, u.stream));
    if ((rc = end_update(c, g, target))) return rc;
    c->scene.tlas = G.raw;
    c->scene.tlasBfs = G.bfs;
    c->scene.instances = (const float4*)G.inst;
    c->scene.instByLeaf = (const float4*)G.byLeaf;
    c->scene.tlasNodeCount = 2u * n - 1u;           // unreachable padding past the tree: the kernels only read reachable nodes
    c->scene.tlasIndexOffset = (2u * n - 1u) * 16u;
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTUpdateInstances(PTContext* c, const PTBlasInstance* instances, uint32_t count)
{
    return update_instances(c, instances, count, false);
}

PT_API int PTUpdateInstancesDevice(PTContext* c, const PTBlasInstance* dInstances, uint32_t count)
{
    return update_instances(c, dInstances, count, true);
}

PT_API int PTUpdateLights(PTContext* c, const void* lights, uint32_t count)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!lights) return fail(PT_ERR_INVALID_ARG, "lights == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (!c->scene.hasLights) return fail(PT_ERR_UNSUPPORTED, "light updates need a scene set with HAS_LIGHTS");
    const uint32_t sceneLightCount = c->update.sceneLightCount;
    if (count == 0 || count > sceneLightCount)
        return fail(PT_ERR_INVALID_ARG, "count must be 1.." + std::to_string(sceneLightCount) + " (the lightCount given to PTSetScene)");
    PTContext::UpdGroup& g = c->update.lights;
    const size_t cap = (size_t)sceneLightCount * 64;
    int rc, target;
    if ((rc = begin_update(c, g, 2 * cap, cap, target))) return rc;
    float4* dl = (float4*)g.gen[target].ptr;
    float4* dc = (float4*)((char*)g.gen[target].ptr + cap);
    if ((rc = stage_host(c, g, target, lights, (size_t)count * 64, dl))) return rc;
    DScene S = c->scene;
    S.lights = dl;
    S.lightCount = (int32_t)count;
    HIP_TRY(pt_launch_derive_lights(S, dc, c->update.stream));
    if ((rc = end_update(c, g, target))) return rc;
    c->scene.lights = dl;
    c->scene.lightConst = dc;
    c->scene.lightCount = (int32_t)count;
    ++c->update.lightGeneration;
    c->update.lightTypes.clear();
    for (uint32_t l = 0; l < count; ++l) c->update.lightTypes.push_back(((const PTLight*)lights)[l].type);
    return PT_OK;
}

PT_API int PTUpdateMaterials(PTContext* c, const void* materials, uint32_t count)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!materials) return fail(PT_ERR_INVALID_ARG, "materials == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (count != c->scene.materialCount)
        return fail(PT_ERR_INVALID_ARG, "count (" + std::to_string(count) + ") != the scene's materialCount (" + std::to_string(c->scene.materialCount) + ")");
    // the texture slots validate_scene checks: negative = none, otherwise a texture PTSetScene validated (the texture data
    // itself was only borrowed for that call)
    const float* mats = (const float*)materials;
    const std::vector<uint32_t>& valid = c->update.validTextures;
    if (c->scene.hasTextures)
        for (uint32_t m = 0; m < count; ++m)
            for (int k : kTextureSlots) {
                const float f = mats[(size_t)m * 32 + k];
                if (f < 0.0f) continue;
                const bool ok = f < 1.0e9f && std::binary_search(valid.begin(), valid.end(), (uint32_t)(uint64_t)f);
                if (!ok) return fail(PT_ERR_INVALID_ARG, "material " + std::to_string(m) + ": texture index is not a texture PTSetScene validated");
            }
    PTContext::UpdGroup& g = c->update.mats;
    const size_t bytes = (size_t)count * 128;
    int rc, target;
    if ((rc = begin_update(c, g, bytes, bytes, target))) return rc;
    if ((rc = stage_host(c, g, target, materials, bytes, g.gen[target].ptr))) return rc;
    if ((rc = end_update(c, g, target))) return rc;
    c->scene.materials = (const float4*)g.gen[target].ptr;
    return PT_OK;
}

PT_API int PTReadTLAS(PTContext* c, void* dstNodes, uint64_t dstNodeBytes, uint32_t* dstIndices, uint64_t dstIndexCount, uint32_t* outNodeCount)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!dstNodes || !dstIndices || !outNodeCount) return fail(PT_ERR_INVALID_ARG, "dstNodes / dstIndices / outNodeCount == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (!c->scene.hasTlas) return fail(PT_ERR_UNSUPPORTED, "the scene has no TLAS");
    HIP_TRY(hipSetDevice(c->device));
    const PTContext::Update& u = c->update;
    if (u.stream) HIP_TRY(hipStreamSynchronize(u.stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t n = u.instanceCount;
    uint32_t nodes = u.origTlasNodes;
    const char* base = (const char*)c->tlas.ptr;
    if (u.inst.cur >= 0) {
        // the copies of this call run on the context stream, not the null stream: passes in flight are not waited for
        HIP_TRY(hipMemcpyAsync(&nodes, u.tlasW.ctrl, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (nodes > 2u * n - 1u) return fail(PT_ERR_HIP, "internal: TLAS node count out of range");
        base = (const char*)inst_gen(u.inst.gen[u.inst.cur].ptr, n).raw;
    }
    const size_t idxOff = u.inst.cur >= 0 ? ((size_t)2 * n - 1) * 64 : (size_t)u.origTlasNodes * 64;
    if (dstNodeBytes < (uint64_t)nodes * 64 || dstIndexCount < n)
        return fail(PT_ERR_INVALID_ARG, "destination too small: " + std::to_string(nodes) + " nodes and " + std::to_string(n) + " indices");
    HIP_TRY(hipMemcpyAsync(dstNodes, base, (size_t)nodes * 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dstIndices, base + idxOff, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *outNodeCount = nodes;
    return PT_OK;
}

} // extern "C"
