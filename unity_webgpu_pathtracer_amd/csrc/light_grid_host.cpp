// light_grid_host.cpp — the host twin of the light-grid build (include/ptmi_plugin.h Part 25): the rule of
// light_grid_rule.h in plain loops, and the parameter checks the context's entry point shares with it.  No GPU involved.
#include "light_grid_rule.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ptlgrid {

bool check_params(const PTLightGridParams* p, std::string& err)
{
    if (!p) { err = "params == NULL"; return false; }
    if (p->structSize == 0u) { err = "PTLightGridParams.structSize is not set (must be sizeof(PTLightGridParams) of the host's header)"; return false; }
    if (p->structSize < sizeof(PTLightGridParams) || p->structSize > 4096u) {
        err = "PTLightGridParams.structSize = " + std::to_string(p->structSize) + " is not a size of this struct";
        return false;
    }
    uint64_t cells = 1;
    for (uint32_t a = 0; a < 3u; ++a) {
        if (p->dims[a] < 1u || p->dims[a] > kMaxDim) {
            err = "dims[" + std::to_string(a) + "] = " + std::to_string(p->dims[a]) + " (1 ... " + std::to_string(kMaxDim) + ")";
            return false;
        }
        cells *= p->dims[a];
    }
    if (cells > kMaxCells) { err = "dims give " + std::to_string(cells) + " cells (at most " + std::to_string(kMaxCells) + ")"; return false; }
    if (!std::isfinite(p->cellSize) || !(p->cellSize > 0.0f)) { err = "cellSize = " + std::to_string(p->cellSize) + " is not finite and > 0"; return false; }
    if (p->reserved) { err = "PTLightGridParams.reserved != 0"; return false; }
    return true;
}

bool build_host(const PTLightGridParams* p, const void* lights, uint32_t lightCount, uint32_t* offsets, uint32_t* indices, uint64_t indexCapacity,
                uint32_t* rectBefore, uint64_t* outTotal, std::string& err)
{
    if (!check_params(p, err)) return false;
    if (lightCount && !lights) { err = "lights == NULL"; return false; }
    if (!offsets || !rectBefore) { err = "offsets / rectBefore == NULL"; return false; }
    if (indexCapacity && !indices) { err = "indices == NULL"; return false; }
    Grid g;
    for (uint32_t a = 0; a < 3u; ++a) { g.origin[a] = p->origin[a]; g.dims[a] = p->dims[a]; }
    g.cellSize = p->cellSize;
    std::vector<ptdirect::Light> L(lightCount);
    uint32_t rects = 0;
    for (uint32_t l = 0; l < lightCount; ++l) {
        PTLight r;
        memcpy(&r, (const char*)lights + (size_t)l * sizeof(PTLight), sizeof(r));
        ptdirect::Light& o = L[l];
        for (uint32_t a = 0; a < 3u; ++a) { o.position[a] = r.position[a]; o.emission[a] = r.emission[a]; o.u[a] = r.u[a]; o.v[a] = r.v[a]; }
        o.type = r.type; o.range = r.range; o.area = r.area;
        ptdirect::derive_rows(o);
        rectBefore[l] = rects;
        rects += r.type == PT_LIGHT_TYPE_RECTANGLE ? 1u : 0u;
    }
    rectBefore[lightCount] = rects;
    const uint32_t cells = cell_count(g);
    // two passes over the cells: the counts, then -- when they fit -- the lists
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t total = 0;
        for (uint32_t c = 0; c <= cells; ++c) {
            if (pass == 0) offsets[c] = (uint32_t)total;
            if (c == cells) {
                if (pass == 1) for (uint32_t l = 0; l < lightCount; ++l) indices[total + l] = l;
                total += lightCount;
                continue;
            }
            const uint32_t i[3] = {c % g.dims[0], (c / g.dims[0]) % g.dims[1], c / (g.dims[0] * g.dims[1])};
            float lo[3], hi[3];
            cell_box(g, i, lo, hi);
            for (uint32_t l = 0; l < lightCount; ++l) {
                if (!lists(L[l], lo, hi)) continue;
                if (pass == 1) indices[total] = l;
                ++total;
            }
        }
        if (total > 0xFFFFFFFFull) { err = "more than 2^32 - 1 list entries"; return false; }
        offsets[cells + 1u] = (uint32_t)total;
        if (outTotal) *outTotal = total;
        if (!indices || total > indexCapacity) break;
    }
    return true;
}

} // namespace ptlgrid
