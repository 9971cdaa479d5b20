// pt_api_light_grid.hip — the light grid of the culled direct-light calls: build, read-back, info and the check the culled calls
// make (include/ptmi_plugin.h Part 25).
#include "pt_context.h"
#include "light_grid_rule.h"

#include <vector>

int current_light_grid(PTContext* c, const char* who, PTLightGridDevice& out)
{
    const PTContext::LightGrid& lg = c->lightGrid;
    if (!lg.built) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": no light grid (PTBuildLightGrid has not been called)");
    if (lg.generation != c->update.lightGeneration)
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": the light grid is stale: the lights changed since PTBuildLightGrid (PTSetScene, PTUpdateLights)");
    out.g = lg.g;
    out.offsets = (const uint32_t*)lg.offsets.ptr;
    out.indices = (const uint32_t*)lg.indices.ptr;
    out.rectBefore = (const uint32_t*)lg.rectBefore.ptr;
    return PT_OK;
}

extern "C" {

PT_API int PTBuildLightGrid(PTContext* c, const PTLightGridParams* params)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTBuildLightGrid: ctx == NULL");
    std::string err;
    if (!ptlgrid::check_params(params, err)) return fail(PT_ERR_INVALID_ARG, "PTBuildLightGrid: " + err);
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    PTContext::LightGrid& lg = c->lightGrid;
    ptlgrid::Grid g;
    for (uint32_t a = 0; a < 3u; ++a) { g.origin[a] = params->origin[a]; g.dims[a] = params->dims[a]; }
    g.cellSize = params->cellSize;
    const uint32_t cells = ptlgrid::cell_count(g);
    const uint32_t L = c->scene.hasLights && c->scene.lightCount > 0 ? (uint32_t)c->scene.lightCount : 0u;
    if ((uint64_t)(cells + 1u) * L > 0xFFFFFFFFull) return fail(PT_ERR_INVALID_ARG, "PTBuildLightGrid: (cells + 1) * lightCount > 2^32 - 1");
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("PT light grid (build)");
    lg.built = false;                                                   // until the emit launch is enqueued
    const uint32_t blocks = pt_light_grid_blocks(cells);
    int rc;
    if ((rc = lg.offsets.reserve(((size_t)cells + 2u) * 4u, c->stream)) || (rc = lg.rectBefore.reserve(((size_t)L + 1u) * 4u, c->stream)) ||
        (rc = lg.blockCounts.reserve(((size_t)blocks + 1u) * 4u, c->stream)) || (rc = lg.total.reserve(4u)))
        return rc;
    uint32_t* blockCounts = (uint32_t*)lg.blockCounts.ptr;
    HIP_TRY(pt_launch_light_grid_count(c->scene, L, g, (uint32_t*)lg.offsets.ptr, blockCounts, (uint32_t*)lg.rectBefore.ptr, blockCounts + blocks, c->stream));
    // the one read-back: the index buffer is sized for the total
    HIP_TRY(hipMemcpyAsync(lg.total.ptr, blockCounts + blocks, 4u, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t total = *(const uint32_t*)lg.total.ptr;
    if ((rc = lg.indices.reserve(((size_t)total + 1u) * 4u))) return rc;      // the stream is drained; + 1: an empty grid still has a buffer
    HIP_TRY(pt_launch_light_grid_emit(c->scene, L, g, (uint32_t*)lg.offsets.ptr, blockCounts, (uint32_t*)lg.indices.ptr, total, c->stream));
    lg.g = g;
    lg.cells = cells;
    lg.lightCount = L;
    lg.entries = total;
    lg.longest = -1;
    lg.generation = c->update.lightGeneration;
    lg.built = true;
    return PT_OK;
}

PT_API int PTReadLightGrid(PTContext* c, uint32_t* offsets, uint32_t* indices, uint64_t indexCapacity, uint32_t* rectBefore)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTReadLightGrid: ctx == NULL");
    const PTContext::LightGrid& lg = c->lightGrid;
    if (!lg.built) return fail(PT_ERR_INVALID_ARG, "PTReadLightGrid: no light grid (PTBuildLightGrid has not been called)");
    if (indices && indexCapacity < lg.entries)
        return fail(PT_ERR_INVALID_ARG, "PTReadLightGrid: indexCapacity = " + std::to_string(indexCapacity) + " is below the " + std::to_string(lg.entries) + " entries");
    HIP_TRY(hipSetDevice(c->device));
    if (offsets) HIP_TRY(hipMemcpyAsync(offsets, lg.offsets.ptr, ((size_t)lg.cells + 2u) * 4u, hipMemcpyDeviceToHost, c->stream));
    if (indices && lg.entries) HIP_TRY(hipMemcpyAsync(indices, lg.indices.ptr, (size_t)lg.entries * 4u, hipMemcpyDeviceToHost, c->stream));
    if (rectBefore) HIP_TRY(hipMemcpyAsync(rectBefore, lg.rectBefore.ptr, ((size_t)lg.lightCount + 1u) * 4u, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

PT_API int PTLightGridInfo(PTContext* c, PTLightGridStats* out)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "PTLightGridInfo: ctx == NULL");
    if (!out) return fail(PT_ERR_INVALID_ARG, "PTLightGridInfo: out == NULL");
    if (out->structSize < sizeof(PTLightGridStats) || out->structSize > 4096u)
        return fail(PT_ERR_INVALID_ARG, "PTLightGridInfo: PTLightGridStats.structSize is not set (must be sizeof(PTLightGridStats) of the host's header)");
    PTContext::LightGrid& lg = c->lightGrid;
    PTLightGridStats s = {};
    s.structSize = (uint32_t)sizeof(s);
    if (lg.built) {
        if (lg.longest < 0) {                                            // the lengths, from the offsets; once per build
            HIP_TRY(hipSetDevice(c->device));
            std::vector<uint32_t> offsets((size_t)lg.cells + 2u);
            HIP_TRY(hipMemcpyAsync(offsets.data(), lg.offsets.ptr, offsets.size() * 4u, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            uint32_t longest = 0;
            for (uint32_t k = 0; k < lg.cells; ++k) longest = offsets[k + 1] - offsets[k] > longest ? offsets[k + 1] - offsets[k] : longest;
            lg.longest = longest;
        }
        s.built = 1u;
        s.cells = lg.cells;
        s.lightCount = lg.lightCount;
        s.longest = (uint32_t)lg.longest;
        s.stale = lg.generation != c->update.lightGeneration ? 1u : 0u;
        s.entries = lg.entries;
        s.generation = lg.generation;
    }
    *out = s;
    return PT_OK;
}

} // extern "C"
