// bvh_refit.cpp — CWBVH refit on the host, behind PTRefitBVH (include/ptmi_plugin.h Part 1), and the plan the device refit
// launches from (pt_api_geometry.hip).  The rule is in bvh_refit.h and DESIGN.md 5.14; pt_refit.hip restates it in two kernels.
#include "bvh_refit.h"

#include <cmath>
#include <cstring>

namespace ptbvh {

namespace {
struct Box { float mn[3], mx[3]; };
const float kInf = INFINITY;
uint32_t word(const PTFloat4& f, int k) { uint32_t u; memcpy(&u, (const char*)&f + 4 * k, 4); return u; }
} // namespace

bool plan_refit(const PTFloat4* nodes, uint64_t nodeCount, const uint32_t* triW, size_t triWStride, uint64_t triRows,
                uint64_t nodeOff, uint64_t triOff, uint32_t triCount, RefitPlan& plan, std::string& err)
{
    auto bad = [&](const std::string& m) { err = m; return false; };
    plan.order.clear();
    plan.levelStart.assign(1, 0u);
    if (triCount == 0 || triOff + (uint64_t)triCount * 3u > triRows) return bad("the triangle records of the BLAS reach past the triangle array");
    if (nodeOff >= nodeCount) return bad("the BLAS root is past the node array");
    std::vector<uint8_t> seenNode(nodeCount - nodeOff, 0), seenRec(triCount, 0);
    uint64_t records = 0;
    std::vector<uint64_t> level(1, 0u), next;                        // node indices relative to nodeOff
    while (!level.empty()) {
        next.clear();
        for (uint64_t rel : level) {
            if (nodeOff + rel >= nodeCount) return bad("child index past the node array");
            if (seenNode[rel]) return bad("node " + std::to_string(nodeOff + rel) + " is reachable twice");
            seenNode[rel] = 1;
            plan.order.push_back((uint32_t)(nodeOff + rel));
            const PTFloat4* n = nodes + (nodeOff + rel) * 5u;
            const uint32_t childBase = word(n[1], 0), triBase = word(n[1], 1), imask = word(n[0], 3) >> 24;
            const uint32_t metaWords[2] = {word(n[1], 2), word(n[1], 3)};
            uint32_t inner = 0;
            for (int s = 0; s < 8; ++s) {
                const uint32_t m = (metaWords[s >> 2] >> (8 * (s & 3))) & 255u;
                if (m == 0) continue;
                if (refit_slot_inner(m)) {
                    if ((m >> 5) != 1u) return bad("node " + std::to_string(nodeOff + rel) + ": inner child with a meta byte that is not (1 << 5) | (24 + slot)");
                    next.push_back((uint64_t)childBase + inner++);
                    continue;
                }
                const uint32_t first = m & 31u, bits = m >> 5;
                if (bits != 1u && bits != 3u && bits != 7u) return bad("node " + std::to_string(nodeOff + rel) + ": leaf triangle bits are not 1, 3 or 7");
                const uint32_t count = bits == 1u ? 1u : (bits == 3u ? 2u : 3u);
                if (triBase % 3u) return bad("node " + std::to_string(nodeOff + rel) + ": triBaseIndex is not a whole record");
                for (uint32_t j = 0; j < count; ++j) {
                    const uint64_t rec = (uint64_t)triBase / 3u + first + j;
                    if (rec >= triCount) return bad("a triangle record outside the BLAS's triangleCount records");
                    if (seenRec[rec]) return bad("triangle record " + std::to_string(rec) + " is reachable twice");
                    seenRec[rec] = 1;
                    ++records;
                    const uint32_t prim = triW[(triOff + rec * 3u + 2u) * triWStride];
                    if (prim >= triCount) return bad("primitive index " + std::to_string(prim) + " >= triangleCount");
                }
            }
            if (inner != (uint32_t)__builtin_popcount(imask)) return bad("node " + std::to_string(nodeOff + rel) + ": imask does not match its inner children");
        }
        plan.levelStart.push_back((uint32_t)plan.order.size());
        level.swap(next);
    }
    if (records != triCount) return bad("the BLAS reaches " + std::to_string(records) + " triangle records, not triangleCount = " + std::to_string(triCount));
    return true;
}

bool refit_cwbvh(PTFloat4* nodes, uint64_t nodeCount, PTFloat4* tris, uint64_t triRows, uint64_t nodeOff, uint64_t triOff,
                 const PTFloat4* verts, uint32_t triCount, std::string& err)
{
    if (!nodes || !tris || !verts) { err = "nodes / tris / vertices == NULL"; return false; }
    for (uint64_t i = 0; i < (uint64_t)triCount * 3u; ++i)
        if (!std::isfinite(verts[i].x) || !std::isfinite(verts[i].y) || !std::isfinite(verts[i].z)) { err = "vertex " + std::to_string(i) + " is not finite"; return false; }
    RefitPlan plan;
    if (!plan_refit(nodes, nodeCount, (const uint32_t*)tris + 3, 4, triRows, nodeOff, triOff, triCount, plan, err)) return false;
    // ---- triangle records: e2, e1, v0 | primIdx (the bytes BuildBVH writes)
    for (uint32_t r = 0; r < triCount; ++r) {
        PTFloat4* rec = tris + triOff + (uint64_t)r * 3u;
        const uint32_t prim = word(rec[2], 3);
        const PTFloat4 v0 = verts[3u * prim], v1 = verts[3u * prim + 1u], v2 = verts[3u * prim + 2u];
        rec[0] = PTFloat4{v2.x - v0.x, v2.y - v0.y, v2.z - v0.z, 0.0f};
        rec[1] = PTFloat4{v1.x - v0.x, v1.y - v0.y, v1.z - v0.z, 0.0f};
        rec[2].x = v0.x; rec[2].y = v0.y; rec[2].z = v0.z;
    }
    // ---- nodes, the deepest level first; nodeBox is indexed relative to the BLAS root, as childBaseIndex is
    std::vector<Box> nodeBox(nodeCount - nodeOff);
    for (size_t lv = plan.levelStart.size() - 1; lv-- > 0;) {
        for (uint32_t k = plan.levelStart[lv]; k < plan.levelStart[lv + 1]; ++k) {
            const uint64_t node = plan.order[k];
            PTFloat4* n = nodes + node * 5u;
            const uint32_t childBase = word(n[1], 0), triBase = word(n[1], 1), imask = word(n[0], 3) >> 24;
            const uint32_t metaWords[2] = {word(n[1], 2), word(n[1], 3)};
            Box cb[8], nb;
            bool used[8];
            for (int a = 0; a < 3; ++a) { nb.mn[a] = kInf; nb.mx[a] = -kInf; }
            uint32_t inner = 0;
            for (int s = 0; s < 8; ++s) {
                const uint32_t m = (metaWords[s >> 2] >> (8 * (s & 3))) & 255u;
                used[s] = m != 0;
                if (!used[s]) continue;
                Box b;
                if (refit_slot_inner(m)) {
                    b = nodeBox[(uint64_t)childBase + inner++];
                } else {
                    for (int a = 0; a < 3; ++a) { b.mn[a] = kInf; b.mx[a] = -kInf; }
                    const uint32_t count = (uint32_t)__builtin_popcount(m >> 5);
                    for (uint32_t j = 0; j < count; ++j) {
                        const uint32_t prim = word(tris[triOff + triBase + 3u * ((m & 31u) + j) + 2u], 3);
                        for (uint32_t v = 0; v < 3; ++v) {
                            const float* p = &verts[3u * prim + v].x;
                            for (int a = 0; a < 3; ++a) { b.mn[a] = refit_min(b.mn[a], p[a]); b.mx[a] = refit_max(b.mx[a], p[a]); }
                        }
                    }
                }
                cb[s] = b;
                for (int a = 0; a < 3; ++a) { nb.mn[a] = refit_min(nb.mn[a], b.mn[a]); nb.mx[a] = refit_max(nb.mx[a], b.mx[a]); }
            }
            nodeBox[node - nodeOff] = nb;
            int e[3];
            float p[3];
            for (int a = 0; a < 3; ++a) { e[a] = refit_exponent(nb.mx[a] - nb.mn[a]); p[a] = ldexpf(1.0f, e[a]); }
            uint8_t q[48];
            memset(q, 0, sizeof(q));
            for (int s = 0; s < 8; ++s) {
                if (!used[s]) continue;
                for (int a = 0; a < 3; ++a) {
                    q[8 * a + s] = (uint8_t)refit_quant_lo(cb[s].mn[a], nb.mn[a], p[a]);
                    q[24 + 8 * a + s] = (uint8_t)refit_quant_hi(cb[s].mx[a], nb.mn[a], p[a]);
                }
            }
            const uint32_t w = ((uint32_t)e[0] & 255u) | (((uint32_t)e[1] & 255u) << 8) | (((uint32_t)e[2] & 255u) << 16) | (imask << 24);
            n[0].x = nb.mn[0]; n[0].y = nb.mn[1]; n[0].z = nb.mn[2];
            memcpy(&n[0].w, &w, 4);
            memcpy(&n[2], q, 48);
        }
    }
    return true;
}

} // namespace ptbvh
