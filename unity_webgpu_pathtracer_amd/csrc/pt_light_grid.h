// pt_light_grid.h — launchers of the light-grid build (pt_light_grid.hip; include/ptmi_plugin.h Part 25) and the
// grid as the culled direct-light kernels read it (pt_direct.hip).
#pragma once
#include "pt_device.h"
#include "light_grid_rule.h"

// a built grid on the device: offsets cells + 2 words, indices offsets[cells + 1] words, rectBefore L + 1 words
struct PTLightGridDevice {
    ptlgrid::Grid g;
    const uint32_t* offsets;
    const uint32_t* indices;
    const uint32_t* rectBefore;
};

// cells of a build block: one lane per cell, the overflow cell included
constexpr uint32_t kLightGridBlock = 1024u;
inline uint32_t pt_light_grid_blocks(uint32_t cells) { return (cells + 1u + kLightGridBlock - 1u) / kLightGridBlock; }

// count: offsets[c] = the length of cell c's list for c = 0 ... cells, blockCounts[b] = the sum over block b, rectBefore[l] = 1 for
// a rectangle light.  scan: blockCounts and rectBefore[0, L) become their exclusive prefixes; offsets[cells + 1] = *total = all
// entries, rectBefore[L] = all rectangles.  The lights are S.lights / S.lightConst, L = lightCount (0: a scene without lights)
hipError_t pt_launch_light_grid_count(const DScene& S, uint32_t lightCount, const ptlgrid::Grid& g, uint32_t* offsets, uint32_t* blockCounts,
                                      uint32_t* rectBefore, uint32_t* total, hipStream_t stream);
// emit: offsets[c] becomes the start of cell c's list, indices gets the lists (capacity words: nothing is written past them)
hipError_t pt_launch_light_grid_emit(const DScene& S, uint32_t lightCount, const ptlgrid::Grid& g, uint32_t* offsets, const uint32_t* blockCounts,
                                     uint32_t* indices, uint32_t capacity, hipStream_t stream);
