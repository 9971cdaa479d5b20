// bvh_quality.cpp — the tree-quality measure on the host, behind PTMeasureBVHArrays (include/ptmi_plugin.h Part 10).  The rule
// is in bvh_quality.h and DESIGN.md 5.15; pt_quality.hip restates it in a kernel.
#include "bvh_quality.h"
#include "bvh_refit.h"

#include <cstring>

namespace ptbvh {

bool measure_cwbvh(const PTFloat4* nodes, uint64_t nodeCount, const PTFloat4* tris, uint64_t triRows, uint32_t triCount, Quality& out, std::string& err)
{
    if (!nodes || !tris) { err = "nodes / tris == NULL"; return false; }
    RefitPlan plan;
    if (!plan_refit(nodes, nodeCount, (const uint32_t*)tris + 3, 4, triRows, 0, 0, triCount, plan, err)) return false;
    out = Quality();
    out.nodeCapacity = (uint32_t)nodeCount;
    out.nodeCount = (uint32_t)plan.order.size();
    out.triangleCount = triCount;
    out.levels = (uint32_t)plan.levelStart.size() - 1u;
    double sum = 0.0;
    for (size_t k = 0; k < plan.order.size(); ++k) {
        uint32_t w[20];
        memcpy(w, nodes + (size_t)plan.order[k] * 5u, 80);
        double fold;
        sum += quality_node_term(w, fold);
        if (k == 0) out.rootHalfArea = fold;
    }
    out.sahCost = out.rootHalfArea > 0.0 ? 1.0 + sum / out.rootHalfArea : 0.0;
    return true;
}

} // namespace ptbvh
