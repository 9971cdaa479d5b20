// pt_api_geometry.hip — geometry updates and PTReadGeometry (include/ptmi_plugin.h Part 9); geometry rebuilds and
// the tree-quality measure (Part 10); skinned geometry (Part 11); morph targets (Part 12).
#include "pt_context.h"
#include "morph_rule.h"

#include <cmath>

namespace {

size_t al256(size_t b) { return (b + 255) / 256 * 256; }

} // namespace

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

namespace {

// end of the span that starts at `off`: the next larger distinct offset among the instances' (field 0 nodes, 1 rows), or `total`
uint64_t span_end(const PTContext::Geometry& G, int field, int32_t off, uint64_t total)
{
    uint64_t end = total;
    for (size_t i = 0; i + 2 < G.blasKeys.size(); i += 3) {
        const int32_t k = G.blasKeys[i + field];
        if (k > off && (uint64_t)k < end) end = (uint64_t)k;
    }
    return end;
}

} // namespace

// The plan of the BLAS the three offsets name; made (and the BLAS walked) on its first update.  triCount == 0 (PTMeasureGeometry):
// the BLAS's own count -- the plan's, or for a BLAS without one the count its row span holds.
int find_plan(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t attrOffset, uint32_t triCount, PTContext::GeomPlan*& out)
{
    PTContext::Geometry& G = c->update.geometry;
    for (PTContext::GeomPlan& p : G.plans)
        if (p.key[0] == bvhOffset && p.key[1] == triOffset && p.key[2] == attrOffset) {
            if (triCount && p.triCount != triCount)
                return fail(PT_ERR_INVALID_ARG, "triangleCount (" + std::to_string(triCount) + ") != the BLAS's (" + std::to_string(p.triCount) + ")");
            out = &p;
            return PT_OK;
        }
    bool named = !c->scene.hasTlas && bvhOffset == 0 && triOffset == 0 && attrOffset == 0;
    for (size_t i = 0; i + 2 < G.blasKeys.size() && !named; i += 3)
        named = G.blasKeys[i] == bvhOffset && G.blasKeys[i + 1] == triOffset && G.blasKeys[i + 2] == attrOffset;
    if (!named) return fail(PT_ERR_INVALID_ARG, "bvhOffset / triOffset / triAttributeOffset name no BLAS of the scene");
    if (!triCount) triCount = (uint32_t)((span_end(G, 1, triOffset, G.hostTriW.size()) - (uint64_t)triOffset) / 3u);
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
    p.nodeCapacity = (uint32_t)(span_end(G, 0, bvhOffset, G.hostNodes.size() / 5) - (uint64_t)bvhOffset);
    if (int rc = p.order.reserve(plan.order.size() * 4)) return rc;
    HIP_TRY(hipMemcpy(p.order.ptr, plan.order.data(), plan.order.size() * 4, hipMemcpyHostToDevice));
    p.levelStart.swap(plan.levelStart);
    G.plans.push_back(std::move(p));
    out = &G.plans.back();
    return PT_OK;
}

namespace {

// The tree of the builder's rule for dVerts, built on the update stream at the BLAS's offsets of the generation being written
// (after the carry-over copy).  Refusals return before anything of the context changes; on success the BLAS's plan is the new tree's.
int rebuild_blas(PTContext* c, PTContext::GeomPlan& plan, char* dNodes, char* dTris, const float4* dVerts, bool checkFinite)
{
    PTContext::Update& u = c->update;
    PTContext::Geometry& G = u.geometry;
    const uint32_t n = plan.triCount, cap = plan.nodeCapacity;
    const size_t workBytes = ptbvh::device_build_work_bytes(n);
    if (!workBytes) return fail(PT_ERR_HIP, "rocprim::radix_sort_pairs: size query failed");
    int rc;
    // grown only for a larger BLAS; the builds that used the old arrays ran on the update stream
    if (workBytes > G.buildWork.bytes && (rc = G.buildWork.reserve(workBytes, u.stream))) return rc;
    ptbvh::DeviceBuildResult res;
    std::string err;
    uint4* nodes = (uint4*)(dNodes + (size_t)plan.key[0] * 80);
    const ptbvh::DeviceBuildStatus st = ptbvh::device_build_cwbvh(u.stream, dVerts, n, nodes, (float4*)(dTris + (size_t)plan.key[1] * 16), cap,
                                                                   G.buildWork.ptr, checkFinite, res, err);
    if (st == ptbvh::kBuildNonFinite) return fail(PT_ERR_INVALID_ARG, "vertex " + std::to_string(res.badVertex) + " is not finite");
    if (st == ptbvh::kBuildOverCapacity)
        return fail(PT_ERR_INVALID_ARG, "the rebuilt tree has " + std::to_string(res.nodeCount) + " nodes, the BLAS's node span (its capacity) holds " + std::to_string(cap));
    if (st != ptbvh::kBuildOk) return fail(PT_ERR_HIP, "geometry rebuild: " + err);
    const uint32_t K = res.nodeCount;
    if (K < cap) HIP_TRY(hipMemsetAsync(nodes + (size_t)K * 5u, 0, (size_t)(cap - K) * 80, u.stream));
    // The builder allocates nodes level by level: index order is depth order, the new plan is the identity over 0 ... K - 1 with the
    // level boundaries the build loop held.  The update stream is idle here (the build's last read-back), so nothing reads the old order.
    std::vector<uint32_t> order(K);
    for (uint32_t k = 0; k < K; ++k) order[k] = (uint32_t)plan.key[0] + k;
    if (plan.order.bytes < (size_t)K * 4 && (rc = plan.order.reserve((size_t)cap * 4))) return rc;
    // on the update stream, not the null stream: a synchronous copy there waits for every set stream that blocks against it
    HIP_TRY(hipMemcpyAsync(plan.order.ptr, order.data(), (size_t)K * 4, hipMemcpyHostToDevice, u.stream));
    HIP_TRY(hipStreamSynchronize(u.stream));        // `order` is this function's
    plan.levelStart.swap(res.levelStart);
    return PT_OK;
}

// PTSkinGeometry's vertex source: the BLAS's skin (PTSetSkin) and a joint palette instead of the caller's vertices.  With
// morphWeights it is PTMorphGeometry's: the BLAS's morph (PTSetMorph) and one weight per target, and the palette may be NULL.
struct SkinSource {
    const float* palette;
    uint32_t jointCount;
    bool onDevice;
    float* outBounds;
    const float* morphWeights = nullptr;
    uint32_t targetCount = 0;
};

// Every geometry update: the vertices are the caller's (host arrays staged, or device arrays), or with `skin` those the skin kernel
// or the morph kernel makes from the BLAS's skin or morph and the palette or weights (verts, triangleCount and attrs then are
// unused: the skin or the morph has them).
int update_geometry(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t attrOffset, const PTFloat4* verts, int triangleCount,
                    const PTTriangleAttributes* attrs, bool onDevice, bool rebuild, const SkinSource* skin = nullptr)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!skin && !verts) return fail(PT_ERR_INVALID_ARG, "vertices == NULL");
    if (skin && !skin->morphWeights && !skin->palette) return fail(PT_ERR_INVALID_ARG, "jointMatrices == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if ((!skin && triangleCount <= 0) || bvhOffset < 0 || triOffset < 0 || attrOffset < 0) return fail(PT_ERR_INVALID_ARG, "triangleCount <= 0 or a negative offset");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_host_copy(c))) return rc;
    PTContext::GeomPlan* plan = nullptr;
    if ((rc = find_plan(c, bvhOffset, triOffset, attrOffset, skin ? 0u : (uint32_t)triangleCount, plan))) return rc;
    const uint32_t triCount = plan->triCount;
    const bool flat = !c->scene.hasTlas;                             // a flat scene's kernels index the materials with the records' materialIndex
    const bool staged = !skin && !onDevice;                          // host arrays go through the groups' pinned staging
    const bool morph = skin && skin->morphWeights;
    if (morph) {
        const PTContext::GeomPlan::Morph& M = plan->morph;
        if (!M.targetCount) return fail(PT_ERR_INVALID_ARG, "the BLAS has no morph (PTSetMorph)");
        if (skin->targetCount != M.targetCount)
            return fail(PT_ERR_INVALID_ARG, "targetCount (" + std::to_string(skin->targetCount) + ") != the morph's (" + std::to_string(M.targetCount) + ")");
        std::string why;
        if (!skin->onDevice && !ptmorph::morph_check_weights(skin->morphWeights, M.targetCount, why)) return fail(PT_ERR_INVALID_ARG, why);
        if (skin->onDevice && ((uintptr_t)skin->morphWeights & 15u)) return fail(PT_ERR_INVALID_ARG, "dWeights is not 16-byte aligned");
    }
    if (skin && skin->palette) {
        const PTContext::GeomPlan::Skin& K = plan->skin;
        if (!K.jointCount) return fail(PT_ERR_INVALID_ARG, morph ? "a palette needs a skin: the BLAS has no skin (PTSetSkin)" : "the BLAS has no skin (PTSetSkin)");
        if (skin->jointCount != K.jointCount)
            return fail(PT_ERR_INVALID_ARG, "jointCount (" + std::to_string(skin->jointCount) + ") != the skin's (" + std::to_string(K.jointCount) + ")");
        std::string why;
        if (!skin->onDevice && !ptskin::skin_check_palette(skin->palette, K.jointCount, why)) return fail(PT_ERR_INVALID_ARG, why);
        if (skin->onDevice && ((uintptr_t)skin->palette & 15u)) return fail(PT_ERR_INVALID_ARG, "dJointMatrices is not 16-byte aligned");
    } else if (!skin && !onDevice) {
        for (size_t i = 0; i < (size_t)triCount * 3; ++i)
            if (!std::isfinite(verts[i].x) || !std::isfinite(verts[i].y) || !std::isfinite(verts[i].z))
                return fail(PT_ERR_INVALID_ARG, "vertex " + std::to_string(i) + " is not finite");
        for (uint32_t i = 0; attrs && flat && i < triCount; ++i)
            if (attrs[i].materialIndex >= c->scene.materialCount)
                return fail(PT_ERR_INVALID_ARG, "triangle " + std::to_string(i) + ": materialIndex " + std::to_string(attrs[i].materialIndex) + " >= materialCount");
    }
    const bool writeAttrs = morph ? plan->morph.restAttrs.ptr != nullptr : skin ? plan->skin.restAttrs.ptr != nullptr : attrs != nullptr;
    PTContext::Update& u = c->update;
    PTContext::Geometry& G = u.geometry;
    const size_t nodeBytes = c->nodes.used, triBytes = c->tris.used, attrBytes = c->attrs.used;
    // staging is sized for the scene, not for the call: the groups never reallocate between updates (begin_update)
    int tg = 0, ta = 0;
    if ((rc = begin_update(c, u.geom, al256(nodeBytes) + triBytes, staged ? triBytes : 0, tg))) return rc;
    if (writeAttrs && (rc = begin_update(c, u.attrs, attrBytes, staged ? attrBytes : 0, ta))) return rc;
    // carry-over: the target generation is two updates old; everything this update does not rewrite comes from the current one
    char* dNodes = (char*)u.geom.gen[tg].ptr;
    char* dTris = dNodes + al256(nodeBytes);
    HIP_TRY(hipMemcpyAsync(dNodes, c->scene.nodes, nodeBytes, hipMemcpyDeviceToDevice, u.stream));
    HIP_TRY(hipMemcpyAsync(dTris, c->scene.tris, triBytes, hipMemcpyDeviceToDevice, u.stream));
    PTSkinArgs S = {};
    PTMorphArgs MA = {};
    char* dAttrs = nullptr;
    // the BLAS's attribute records of the target generation: the carry-over copy, then the new records
    auto write_attrs = [&]() -> int {
        dAttrs = (char*)u.attrs.gen[ta].ptr;
        char* dst = dAttrs + (size_t)attrOffset * 128;
        HIP_TRY(hipMemcpyAsync(dAttrs, c->scene.attrs, attrBytes, hipMemcpyDeviceToDevice, u.stream));
        if (morph) HIP_TRY(pt_launch_morph_attrs(MA, skin->palette ? &S : nullptr, (float4*)dst, u.stream));
        else if (skin) HIP_TRY(pt_launch_skin_attrs(S, (float4*)dst, u.stream));     // each record once, no staging copy
        else if (onDevice) HIP_TRY(pt_launch_refit_attrs((float4*)dst, (const float4*)attrs, triCount, flat ? c->scene.materialCount : 0xFFFFFFFFu, u.stream));
        else if (int e = stage_host(c, u.attrs, ta, attrs, (size_t)triCount * 128, dst)) return e;
        return PT_OK;
    };
    const float4* dVerts = (const float4*)verts;
    if (onDevice || (skin && skin->onDevice)) {
        HIP_TRY(hipEventRecord(u.input, c->stream));
        HIP_TRY(hipStreamWaitEvent(u.stream, u.input, 0));
    }
    // 48 B per triangle, as the records: room for the largest BLAS, so that it is allocated once (first host update or skin)
    if ((staged || skin) && !G.verts.ptr && (rc = G.verts.reserve(triBytes))) return rc;
    if (skin) {
        const PTContext::GeomPlan::Skin& K = plan->skin;
        S.rest = (const float4*)K.rest.ptr; S.joints = (const uint2*)K.joints.ptr; S.weights = (const float4*)K.weights.ptr;
        S.restAttrs = (const float4*)K.restAttrs.ptr;
        S.triCount = triCount;
        S.palette = (const float4*)skin->palette;
        if (skin->palette && !skin->onDevice) {
            if ((rc = G.palette.send(skin->palette, (size_t)K.jointCount * 48, u.stream))) return rc;
            S.palette = (const float4*)G.palette.dev.ptr;
        }
        if (morph) {
            const PTContext::GeomPlan::Morph& M = plan->morph;
            MA.rest = (const float4*)M.rest.ptr; MA.restAttrs = (const float4*)M.restAttrs.ptr;
            MA.position = M.position.args(); MA.normal = M.normal.args(); MA.tangent = M.tangent.args();
            MA.triCount = triCount;
            MA.weights = skin->morphWeights;
            if (!skin->onDevice) {
                if ((rc = G.morphWeights.send(skin->morphWeights, (size_t)M.targetCount * 4, u.stream))) return rc;
                MA.weights = (const float*)G.morphWeights.dev.ptr;
            }
        }
        // grown only for a larger BLAS; the folds that used the old array ran on the update stream (the morph's work space is the skin's)
        if ((rc = G.skinWork.reserve(pt_skin_work_floats(triCount) * sizeof(float), u.stream))) return rc;
        if (morph) HIP_TRY(pt_launch_morph_vertices(MA, skin->palette ? &S : nullptr, (float4*)G.verts.ptr, (float*)G.skinWork.ptr, u.stream));
        else HIP_TRY(pt_launch_skin_vertices(S, (float4*)G.verts.ptr, (float*)G.skinWork.ptr, u.stream));
        if (skin->outBounds) {
            if ((rc = G.skinBounds.reserve(6 * sizeof(float)))) return rc;
            HIP_TRY(hipMemcpyAsync(G.skinBounds.ptr, G.skinWork.ptr, 6 * sizeof(float), hipMemcpyDeviceToHost, u.stream));
        }
        dVerts = (const float4*)G.verts.ptr;
        if (writeAttrs && (rc = write_attrs())) return rc;
    } else if (staged) {
        if ((rc = stage_host(c, u.geom, tg, verts, (size_t)triCount * 48, G.verts.ptr))) return rc;
        dVerts = (const float4*)G.verts.ptr;
    }
    if (rebuild) {
        // a refusal leaves the scene as it was: the generation being written is not current, and nothing below has run
        if ((rc = rebuild_blas(c, *plan, dNodes, dTris, dVerts, onDevice || skin != nullptr))) return rc;
    } else {
    PTRefitArgs A;
    A.nodes = (uint4*)dNodes;
    A.tris = (float4*)dTris;
    A.verts = dVerts;
    A.nodeBox = (float*)G.nodeBox.ptr;
    A.order = (const uint32_t*)plan->order.ptr;
    A.nodeOff = (uint32_t)bvhOffset; A.triOff = (uint32_t)triOffset; A.triCount = triCount;
    HIP_TRY(pt_launch_refit(A, plan->levelStart.data(), (uint32_t)plan->levelStart.size() - 1u, u.stream, nullptr));
    }
    if (skin && skin->outBounds) {
        // 24 bytes: synchronises with the update stream only, not with the passes in flight
        HIP_TRY(hipStreamSynchronize(u.stream));
        memcpy(skin->outBounds, G.skinBounds.ptr, 6 * sizeof(float));
    }
    if (!skin && writeAttrs && (rc = write_attrs())) return rc;
    if ((rc = end_update(c, u.geom, tg))) return rc;
    c->scene.nodes = (const uint4*)dNodes;
    c->scene.tris = (const float4*)dTris;
    if (writeAttrs) {
        if ((rc = end_update(c, u.attrs, ta))) return rc;
        c->scene.attrs = (const float4*)dAttrs;
    }
    return PT_OK;
}

// PTSetSkin: the desc's arrays onto the device, replacing the BLAS's skin; desc == NULL removes it
int set_skin(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t attrOffset, int triangleCount, const PTSkinDesc* hostDesc)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (triangleCount <= 0 || bvhOffset < 0 || triOffset < 0 || attrOffset < 0) return fail(PT_ERR_INVALID_ARG, "triangleCount <= 0 or a negative offset");
    PTSkinDesc d;
    if (hostDesc)
        if (int rc = import_struct(hostDesc, d, sizeof(PTSkinDesc), "PTSkinDesc", "desc == NULL")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_host_copy(c))) return rc;
    PTContext::GeomPlan* plan = nullptr;
    if ((rc = find_plan(c, bvhOffset, triOffset, attrOffset, (uint32_t)triangleCount, plan))) return rc;
    const uint32_t triCount = plan->triCount;
    std::string why;
    if (hostDesc && !ptskin::skin_check(d, triCount, c->scene.hasTlas ? 0xFFFFFFFFu : c->scene.materialCount, why)) return fail(PT_ERR_INVALID_ARG, why);
    // skin kernels enqueued so far read the arrays replaced or freed below
    if (c->update.stream) HIP_TRY(hipStreamSynchronize(c->update.stream));
    PTContext::GeomPlan::Skin K;
    if (hostDesc) {
        const size_t n = (size_t)triCount * 3u;
        if ((rc = K.rest.reserve(n * 16)) || (rc = K.joints.reserve(n * 8)) || (rc = K.weights.reserve(n * 16))) return rc;
        HIP_TRY(hipMemcpy(K.rest.ptr, d.restVertices, n * 16, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(K.joints.ptr, d.joints, n * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(K.weights.ptr, d.weights, n * 16, hipMemcpyHostToDevice));
        if (d.restAttrs) {
            if ((rc = K.restAttrs.reserve((size_t)triCount * 128))) return rc;
            HIP_TRY(hipMemcpy(K.restAttrs.ptr, d.restAttrs, (size_t)triCount * 128, hipMemcpyHostToDevice));
        }
        K.jointCount = d.jointCount;
    }
    plan->skin = std::move(K);                                      // the old arrays are released with K
    return PT_OK;
}

// PTSetMorph: the desc's arrays onto the device (each stream in the kernels' layout), replacing the BLAS's morph; desc == NULL removes it
int set_morph(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t attrOffset, int triangleCount, const PTMorphDesc* hostDesc)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (triangleCount <= 0 || bvhOffset < 0 || triOffset < 0 || attrOffset < 0) return fail(PT_ERR_INVALID_ARG, "triangleCount <= 0 or a negative offset");
    PTMorphDesc d;
    if (hostDesc)
        if (int rc = import_struct(hostDesc, d, sizeof(PTMorphDesc), "PTMorphDesc", "desc == NULL")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_host_copy(c))) return rc;
    PTContext::GeomPlan* plan = nullptr;
    if ((rc = find_plan(c, bvhOffset, triOffset, attrOffset, (uint32_t)triangleCount, plan))) return rc;
    const uint32_t triCount = plan->triCount, corners = triCount * 3u;
    std::string why;
    if (hostDesc && !ptmorph::morph_check(d, triCount, c->scene.hasTlas ? 0xFFFFFFFFu : c->scene.materialCount, why)) return fail(PT_ERR_INVALID_ARG, why);
    PTContext::GeomPlan::Morph M;
    // one stream: laid out on the host, then copied; an empty stream keeps 16 bytes so that its pointer says "present"
    auto upload = [&](const uint32_t* off, const PTMorphEntry* ent, PTContext::GeomPlan::Morph::Stream& S) -> int {
        ptmorph::MorphLayout L;
        if (!ptmorph::morph_layout(off, ent, corners, L)) return fail(PT_ERR_INVALID_ARG, "the stream's stored entries (padding included) do not fit 32 bits");
        const size_t bytes = L.entries.size() * sizeof(PTMorphEntry);
        if (int e = S.count.reserve(L.count.size() * 4)) return e;
        if (int e = S.sliceBase.reserve(L.sliceBase.size() * 4)) return e;
        if (int e = S.entries.reserve(bytes ? bytes : 16)) return e;
        HIP_TRY(hipMemcpy(S.count.ptr, L.count.data(), L.count.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(S.sliceBase.ptr, L.sliceBase.data(), L.sliceBase.size() * 4, hipMemcpyHostToDevice));
        if (bytes) HIP_TRY(hipMemcpy(S.entries.ptr, L.entries.data(), bytes, hipMemcpyHostToDevice));
        return PT_OK;
    };
    if (hostDesc) {
        if ((rc = M.rest.reserve((size_t)corners * 16))) return rc;
        HIP_TRY(hipMemcpy(M.rest.ptr, d.restVertices, (size_t)corners * 16, hipMemcpyHostToDevice));
        if ((rc = upload(d.positionOffsets, d.positionEntries, M.position))) return rc;
        if (d.normalOffsets && (rc = upload(d.normalOffsets, d.normalEntries, M.normal))) return rc;
        if (d.tangentOffsets && (rc = upload(d.tangentOffsets, d.tangentEntries, M.tangent))) return rc;
        if (d.restAttrs) {
            if ((rc = M.restAttrs.reserve((size_t)triCount * 128))) return rc;
            HIP_TRY(hipMemcpy(M.restAttrs.ptr, d.restAttrs, (size_t)triCount * 128, hipMemcpyHostToDevice));
        }
        M.targetCount = d.targetCount;
    }
    // morph kernels enqueued so far read the arrays replaced or freed below
    if (c->update.stream) HIP_TRY(hipStreamSynchronize(c->update.stream));
    plan->morph = std::move(M);                                     // the old arrays are released with M
    return PT_OK;
}

} // namespace

extern "C" {

PT_API int PTUpdateGeometry(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* vertices,
                            int triangleCount, const PTTriangleAttributes* attrsOrNull)
{
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, vertices, triangleCount, attrsOrNull, false, false);
}

PT_API int PTUpdateGeometryDevice(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* dVertices,
                                  int triangleCount, const PTTriangleAttributes* dAttrsOrNull)
{
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, dVertices, triangleCount, dAttrsOrNull, true, false);
}

PT_API int PTRebuildGeometry(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* vertices,
                             int triangleCount, const PTTriangleAttributes* attrsOrNull)
{
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, vertices, triangleCount, attrsOrNull, false, true);
}

PT_API int PTRebuildGeometryDevice(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* dVertices,
                                   int triangleCount, const PTTriangleAttributes* dAttrsOrNull)
{
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, dVertices, triangleCount, dAttrsOrNull, true, true);
}

PT_API int PTSetSkin(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, int triangleCount, const PTSkinDesc* descOrNull)
{
    return set_skin(c, bvhOffset, triOffset, triAttributeOffset, triangleCount, descOrNull);
}

PT_API int PTSkinGeometry(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const float* jointMatrices,
                          uint32_t jointCount, uint32_t flags, float* outBounds)
{
    if (flags & ~PT_SKIN_REBUILD) return fail(PT_ERR_INVALID_ARG, "unknown flags");
    const SkinSource src = {jointMatrices, jointCount, false, outBounds};
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, nullptr, 0, nullptr, false, (flags & PT_SKIN_REBUILD) != 0, &src);
}

PT_API int PTSkinGeometryDevice(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const float* dJointMatrices,
                                uint32_t jointCount, uint32_t flags, float* outBounds)
{
    if (flags & ~PT_SKIN_REBUILD) return fail(PT_ERR_INVALID_ARG, "unknown flags");
    const SkinSource src = {dJointMatrices, jointCount, true, outBounds};
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, nullptr, 0, nullptr, false, (flags & PT_SKIN_REBUILD) != 0, &src);
}

PT_API int PTSetMorph(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, int triangleCount, const PTMorphDesc* descOrNull)
{
    return set_morph(c, bvhOffset, triOffset, triAttributeOffset, triangleCount, descOrNull);
}

PT_API int PTMorphGeometry(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const float* weights, uint32_t targetCount,
                           const float* jointMatricesOrNull, uint32_t jointCount, uint32_t flags, float* outBounds)
{
    if (flags & ~PT_SKIN_REBUILD) return fail(PT_ERR_INVALID_ARG, "unknown flags");
    if (c && !weights) return fail(PT_ERR_INVALID_ARG, "weights == NULL");
    SkinSource src = {jointMatricesOrNull, jointCount, false, outBounds};
    src.morphWeights = weights; src.targetCount = targetCount;
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, nullptr, 0, nullptr, false, (flags & PT_SKIN_REBUILD) != 0, &src);
}

PT_API int PTMorphGeometryDevice(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const float* dWeights, uint32_t targetCount,
                                 const float* dJointMatricesOrNull, uint32_t jointCount, uint32_t flags, float* outBounds)
{
    if (flags & ~PT_SKIN_REBUILD) return fail(PT_ERR_INVALID_ARG, "unknown flags");
    if (c && !dWeights) return fail(PT_ERR_INVALID_ARG, "dWeights == NULL");
    SkinSource src = {dJointMatricesOrNull, jointCount, true, outBounds};
    src.morphWeights = dWeights; src.targetCount = targetCount;
    return update_geometry(c, bvhOffset, triOffset, triAttributeOffset, nullptr, 0, nullptr, false, (flags & PT_SKIN_REBUILD) != 0, &src);
}

PT_API int PTMeasureGeometry(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, PTGeometryQuality* out)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (!out) return fail(PT_ERR_INVALID_ARG, "out == NULL");
    if (out->structSize < sizeof(PTGeometryQuality) || out->structSize > 4096u)
        return fail(PT_ERR_INVALID_ARG, "PTGeometryQuality.structSize is not set (must be sizeof(PTGeometryQuality) of the host's header)");
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    if (bvhOffset < 0 || triOffset < 0 || triAttributeOffset < 0) return fail(PT_ERR_INVALID_ARG, "a negative offset");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_host_copy(c))) return rc;
    PTContext::GeomPlan* plan = nullptr;
    if ((rc = find_plan(c, bvhOffset, triOffset, triAttributeOffset, 0, plan))) return rc;
    PTContext::Geometry& G = c->update.geometry;
    const uint32_t K = plan->levelStart.back();
    if ((rc = G.qualityWork.reserve(pt_quality_work_bytes(K), c->stream))) return rc;
    // on the context stream: behind every update enqueued so far (end_update), as a query is
    HIP_TRY(pt_launch_geometry_quality(c->scene.nodes, (const uint32_t*)plan->order.ptr, K, (double*)G.qualityWork.ptr, c->stream));
    double r[2] = {0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(r, G.qualityWork.ptr, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->nodeCapacity = plan->nodeCapacity;
    out->nodeCount = K;
    out->triangleCount = plan->triCount;
    out->levels = (uint32_t)plan->levelStart.size() - 1u;
    out->reserved = 0;
    out->rootHalfArea = r[1];
    out->sahCost = r[1] > 0.0 ? 1.0 + r[0] / r[1] : 0.0;
    return PT_OK;
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
    // on the context stream, not the null stream: passes in flight are not waited for (they do not write the scene)
    HIP_TRY(hipMemcpyAsync(dstNodes, c->scene.nodes, c->nodes.used, hipMemcpyDeviceToHost, c->stream));
    if (c->tris.used) HIP_TRY(hipMemcpyAsync(dstTris, c->scene.tris, c->tris.used, hipMemcpyDeviceToHost, c->stream));
    if (dstAttrs && c->attrs.used) HIP_TRY(hipMemcpyAsync(dstAttrs, c->scene.attrs, c->attrs.used, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

} // extern "C"
