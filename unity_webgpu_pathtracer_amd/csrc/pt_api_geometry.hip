// pt_api_geometry.hip — geometry updates and PTReadGeometry (include/ptmi_plugin.h Part 9).
#include "pt_context.h"

#include <cmath>

namespace {

size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// What the first geometry update of a scene reads back, once (synchronising): the node buffer, the .w words of the triangle
// rows and, with HAS_TLAS, the instances' offsets.  PTSetScene's own buffers serve in every generation: a refit never
// rewrites row n1, imask or a primIdx, and instance updates keep the offsets rows.
int ensure_host_copy(PTContext* c)
{
    PTContext::Geometry& G = c->update.geometry;
    if (!G.hostNodes.empty()) return PT_OK;
    std::vector<PTFloat4> nodes(c->nodes.used / 16), tris(c->tris.used / 16);
    HIP_TRY(hipMemcpy(nodes.data(), c->nodes.ptr, c->nodes.used, hipMemcpyDeviceToHost));
    if (!tris.empty()) HIP_TRY(hipMemcpy(tris.data(), c->tris.ptr, c->tris.used, hipMemcpyDeviceToHost));
    G.hostTriW.resize(tris.size());
    for (size_t i = 0; i < tris.size(); ++i) memcpy(&G.hostTriW[i], &tris[i].w, 4);
    G.blasKeys.clear();
    if (c->scene.hasTlas) {
        const uint32_t n = c->update.instanceCount;
        std::vector<int32_t> inst((size_t)n * 36);
        HIP_TRY(hipMemcpy(inst.data(), c->instances.ptr, (size_t)n * 144, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) G.blasKeys.insert(G.blasKeys.end(), &inst[(size_t)i * 36 + 32], &inst[(size_t)i * 36 + 35]);
    }
    int rc;
    if ((rc = G.nodeBox.reserve(nodes.size() / 5 * 24))) return rc;
    G.hostNodes.swap(nodes);
    return PT_OK;
}

// The plan of the BLAS the three offsets name; made (and the BLAS walked) on its first update
int find_plan(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t attrOffset, uint32_t triCount, PTContext::GeomPlan*& out)
{
    PTContext::Geometry& G = c->update.geometry;
    for (PTContext::GeomPlan& p : G.plans)
        if (p.key[0] == bvhOffset && p.key[1] == triOffset && p.key[2] == attrOffset) {
            if (p.triCount != triCount)
                return fail(PT_ERR_INVALID_ARG, "triangleCount (" + std::to_string(triCount) + ") != the BLAS's (" + std::to_string(p.triCount) + ")");
            out = &p;
            return PT_OK;
        }
    bool named = !c->scene.hasTlas && bvhOffset == 0 && triOffset == 0 && attrOffset == 0;
    for (size_t i = 0; i + 2 < G.blasKeys.size() && !named; i += 3)
        named = G.blasKeys[i] == bvhOffset && G.blasKeys[i + 1] == triOffset && G.blasKeys[i + 2] == attrOffset;
    if (!named) return fail(PT_ERR_INVALID_ARG, "bvhOffset / triOffset / triAttributeOffset name no BLAS of the scene");
    if ((uint64_t)attrOffset + triCount > c->attrs.used / 128u) return fail(PT_ERR_INVALID_ARG, "triangleCount reaches past the attribute records");
    ptbvh::RefitPlan plan;
    std::string why;
    if (!ptbvh::plan_refit(G.hostNodes.data(), G.hostNodes.size() / 5, G.hostTriW.data(), 1, G.hostTriW.size(), (uint64_t)bvhOffset,
                           (uint64_t)triOffset, triCount, plan, why))
        return fail(PT_ERR_INVALID_ARG, "geometry update refused: " + why);
    // Instances may share a BLAS only whole (the same three offsets).  A different BLAS that starts inside this one's nodes or
    // records would be changed by this one's refit behind its back: refused where it can be seen from the roots.
    uint32_t nodeLo = 0xFFFFFFFFu, nodeHi = 0;
    for (uint32_t n : plan.order) { nodeLo = n < nodeLo ? n : nodeLo; nodeHi = n > nodeHi ? n : nodeHi; }
    for (size_t i = 0; i + 2 < G.blasKeys.size(); i += 3) {
        const int32_t* k = &G.blasKeys[i];
        if (k[0] == bvhOffset && k[1] == triOffset && k[2] == attrOffset) continue;
        const bool nodesShared = (uint32_t)k[0] >= nodeLo && (uint32_t)k[0] <= nodeHi;
        const bool trisShared = (uint64_t)k[1] >= (uint64_t)triOffset && (uint64_t)k[1] < (uint64_t)triOffset + (uint64_t)triCount * 3u;
        if (nodesShared || trisShared) return fail(PT_ERR_INVALID_ARG, "another BLAS of the scene shares nodes or triangle records with this one");
    }
    PTContext::GeomPlan p;
    p.key[0] = bvhOffset; p.key[1] = triOffset; p.key[2] = attrOffset;
    p.triCount = triCount;
    if (int rc = p.order.reserve(plan.order.size() * 4)) return rc;
    HIP_TRY(hipMemcpy(p.order.ptr, plan.order.data(), plan.order.size() * 4, hipMemcpyHostToDevice));
    p.levelStart.swap(plan.levelStart);
    G.plans.push_back(std::move(p));
    out = &G.plans.back();
    return PT_OK;
}

int update_geometry(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t attrOffset, const PTFloat4* verts, int triangleCount,
                    const PTTriangleAttributes* attrs, bool onDevice)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!verts) return fail(PT_ERR_INVALID_ARG, "vertices == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (triangleCount <= 0 || bvhOffset < 0 || triOffset < 0 || attrOffset < 0) return fail(PT_ERR_INVALID_ARG, "triangleCount <= 0 or a negative offset");
    const uint32_t triCount = (uint32_t)triangleCount;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_host_copy(c))) return rc;
    PTContext::GeomPlan* plan = nullptr;
    if ((rc = find_plan(c, bvhOffset, triOffset, attrOffset, triCount, plan))) return rc;
    const bool flat = !c->scene.hasTlas;                             // a flat scene's kernels index the materials with the records' materialIndex
    if (!onDevice) {
        for (size_t i = 0; i < (size_t)triCount * 3; ++i)
            if (!std::isfinite(verts[i].x) || !std::isfinite(verts[i].y) || !std::isfinite(verts[i].z))
                return fail(PT_ERR_INVALID_ARG, "vertex " + std::to_string(i) + " is not finite");
        for (uint32_t i = 0; attrs && flat && i < triCount; ++i)
            if (attrs[i].materialIndex >= c->scene.materialCount)
                return fail(PT_ERR_INVALID_ARG, "triangle " + std::to_string(i) + ": materialIndex " + std::to_string(attrs[i].materialIndex) + " >= materialCount");
    }
    PTContext::Update& u = c->update;
    PTContext::Geometry& G = u.geometry;
    const size_t nodeBytes = c->nodes.used, triBytes = c->tris.used, attrBytes = c->attrs.used;
    // staging is sized for the scene, not for the call: the groups never reallocate between updates (begin_update)
    int tg = 0, ta = 0;
    if ((rc = begin_update(c, u.geom, al256(nodeBytes) + triBytes, onDevice ? 0 : triBytes, tg))) return rc;
    if (attrs && (rc = begin_update(c, u.attrs, attrBytes, onDevice ? 0 : attrBytes, ta))) return rc;
    // carry-over: the target generation is two updates old; everything this update does not rewrite comes from the current one
    char* dNodes = (char*)u.geom.gen[tg].ptr;
    char* dTris = dNodes + al256(nodeBytes);
    HIP_TRY(hipMemcpyAsync(dNodes, c->scene.nodes, nodeBytes, hipMemcpyDeviceToDevice, u.stream));
    HIP_TRY(hipMemcpyAsync(dTris, c->scene.tris, triBytes, hipMemcpyDeviceToDevice, u.stream));
    const float4* dVerts = (const float4*)verts;
    if (onDevice) {
        HIP_TRY(hipEventRecord(u.input, c->stream));
        HIP_TRY(hipStreamWaitEvent(u.stream, u.input, 0));
    } else {
        // 48 B per triangle, as the records: room for the largest BLAS, so that it is allocated once (first host update)
        if (!G.verts.ptr && (rc = G.verts.reserve(triBytes))) return rc;
        if ((rc = stage_host(c, u.geom, tg, verts, (size_t)triCount * 48, G.verts.ptr))) return rc;
        dVerts = (const float4*)G.verts.ptr;
    }
    PTRefitArgs A;
    A.nodes = (uint4*)dNodes;
    A.tris = (float4*)dTris;
    A.verts = dVerts;
    A.nodeBox = (float*)G.nodeBox.ptr;
    A.order = (const uint32_t*)plan->order.ptr;
    A.nodeOff = (uint32_t)bvhOffset; A.triOff = (uint32_t)triOffset; A.triCount = triCount;
    HIP_TRY(pt_launch_refit(A, plan->levelStart.data(), (uint32_t)plan->levelStart.size() - 1u, u.stream, nullptr));
    char* dAttrs = nullptr;
    if (attrs) {
        dAttrs = (char*)u.attrs.gen[ta].ptr;
        char* dst = dAttrs + (size_t)attrOffset * 128;
        HIP_TRY(hipMemcpyAsync(dAttrs, c->scene.attrs, attrBytes, hipMemcpyDeviceToDevice, u.stream));
        if (onDevice) HIP_TRY(pt_launch_refit_attrs((float4*)dst, (const float4*)attrs, triCount, flat ? c->scene.materialCount : 0xFFFFFFFFu, u.stream));
        else if ((rc = stage_host(c, u.attrs, ta, attrs, (size_t)triCount * 128, dst))) return rc;
    }
    if ((rc = end_update(c, u.geom, tg))) return rc;
    c->scene.nodes = (const uint4*)dNodes;
    c->scene.tris = (const float4*)dTris;
    if (attrs) {
        if ((rc = end_update(c, u.attrs, ta))) return rc;
        c->scene.attrs = (const float4*)dAttrs;
    }
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTUpdateGeometry(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* vertices,
                            int triangleCount, const PTTriangleAttributes* attrsOrNull)
{
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, vertices, triangleCount, attrsOrNull, false);
}

PT_API int PTUpdateGeometryDevice(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* dVertices,
                                  int triangleCount, const PTTriangleAttributes* dAttrsOrNull)
{
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, dVertices, triangleCount, dAttrsOrNull, true);
}

PT_API int PTReadGeometry(PTContext* c, void* dstNodes, uint64_t nodeBytes, void* dstTris, uint64_t triBytes, void* dstAttrs, uint64_t attrBytes)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!dstNodes || !dstTris) return fail(PT_ERR_INVALID_ARG, "dstNodes / dstTris == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (nodeBytes < c->nodes.used || triBytes < c->tris.used || (dstAttrs && attrBytes < c->attrs.used))
        return fail(PT_ERR_INVALID_ARG, "destination too small: " + std::to_string(c->nodes.used) + " node bytes, " + std::to_string(c->tris.used) +
                                            " triangle bytes, " + std::to_string(c->attrs.used) + " attribute bytes");
    HIP_TRY(hipSetDevice(c->device));
    if (c->update.stream) HIP_TRY(hipStreamSynchronize(c->update.stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(dstNodes, c->scene.nodes, c->nodes.used, hipMemcpyDeviceToHost));
    if (c->tris.used) HIP_TRY(hipMemcpy(dstTris, c->scene.tris, c->tris.used, hipMemcpyDeviceToHost));
    if (dstAttrs && c->attrs.used) HIP_TRY(hipMemcpy(dstAttrs, c->scene.attrs, c->attrs.used, hipMemcpyDeviceToHost));
    return PT_OK;
}

} // extern "C"
