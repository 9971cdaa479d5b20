// pt_light_grid.hip — the light grid built on the device (include/ptmi_plugin.h Part 25).
//
//     pt_lgrid_count   one lane per cell (the overflow cell is the last lane), workgroups of 1024: the lights walked through
//                      wave-uniform scalar loads, light_grid_rule.h's tests against the lane's inflated box; the lane's count,
//                      the workgroup's total (pt_compact.h's scan), and a 0 / 1 word per light for the rectangles
//     pt_lgrid_scan    one workgroup of 1024: the block totals and the rectangle words become exclusive prefixes
//     pt_lgrid_emit    the same workgroups as count: the exclusive scan of the counts inside the block on top of the block's
//                      prefix is the list's start; the same walk writes the lights, in ascending index by construction
// No atomics: the same lights and the same grid give the same bytes, whatever the launch geometry.
#include "pt_device.h"
#include "pt_compact.h"
#include "pt_light_grid.h"

namespace {

// light l as the grid rule reads it; l is the same in every lane of the wave: five scalar loads
PT_DEV ptdirect::Light grid_light(const float4* lights, const float4* lightConst, uint32_t l)
{
    const float4 a = pt_uniform_load(lights, (size_t)l * 4), b = pt_uniform_load(lights, (size_t)l * 4 + 1), c = pt_uniform_load(lights, (size_t)l * 4 + 2),
                 d = pt_uniform_load(lights, (size_t)l * 4 + 3);
    const float4 n = pt_uniform_load(lightConst, (size_t)l * 4);
    ptdirect::Light L = {};
    L.position[0] = a.x; L.position[1] = a.y; L.position[2] = a.z; L.type = pt_asuint(a.w);
    L.emission[0] = b.x; L.emission[1] = b.y; L.emission[2] = b.z; L.range = b.w;
    L.u[0] = c.x; L.u[1] = c.y; L.u[2] = c.z; L.area = c.w;
    L.v[0] = d.x; L.v[1] = d.y; L.v[2] = d.z;
    L.N[0] = n.x; L.N[1] = n.y; L.N[2] = n.z;
    return L;
}

struct GridBuildArgs {
    const float4* lights;
    const float4* lightConst;
    uint32_t lightCount, cells;
    ptlgrid::Grid g;
};

// the list of `cell` in ascending light index: emit(k, l) for its k-th light; returns its length.  A lane past the overflow cell
// walks along (the loads are the wave's) and lists nothing
template <class Emit>
PT_DEV uint32_t walk_cell(const GridBuildArgs& A, uint32_t cell, Emit emit)
{
    const bool real = cell < A.cells, overflow = cell == A.cells;
    const uint32_t c = real ? cell : 0u;
    const uint32_t i[3] = {c % A.g.dims[0], (c / A.g.dims[0]) % A.g.dims[1], c / (A.g.dims[0] * A.g.dims[1])};
    float lo[3], hi[3];
    ptlgrid::cell_box(A.g, i, lo, hi);
    uint32_t n = 0;
    for (uint32_t l = 0; l < A.lightCount; ++l) {
        const ptdirect::Light Lt = grid_light(A.lights, A.lightConst, l);
        if (overflow || (real && ptlgrid::lists(Lt, lo, hi))) {
            emit(n, l);
            ++n;
        }
    }
    return n;
}

} // namespace

extern "C" __global__ __launch_bounds__(1024) void pt_lgrid_count(GridBuildArgs A, uint32_t* __restrict__ offsets, uint32_t* __restrict__ blockCounts,
                                                                  uint32_t* __restrict__ rectBefore)
{
    __shared__ uint32_t s_sum[16];
    const uint32_t cell = blockIdx.x * kLightGridBlock + threadIdx.x;
    const uint32_t n = walk_cell(A, cell, [](uint32_t, uint32_t) {});
    if (cell <= A.cells) offsets[cell] = n;
    uint32_t all;
    compact_scan_threads(n, s_sum, all);
    if (threadIdx.x == 0u) blockCounts[blockIdx.x] = all;
    for (uint32_t l = cell; l < A.lightCount; l += gridDim.x * kLightGridBlock)
        rectBefore[l] = pt_asuint(A.lights[(size_t)l * 4].w) == PT_LIGHT_TYPE_RECTANGLE ? 1u : 0u;
}

extern "C" __global__ __launch_bounds__(1024) void pt_lgrid_scan(uint32_t* __restrict__ blockCounts, uint32_t blocks, uint32_t* __restrict__ rectBefore,
                                                                 uint32_t lightCount, uint32_t* __restrict__ offsets, uint32_t cells,
                                                                 uint32_t* __restrict__ total)
{
    __shared__ uint32_t s_a[16], s_b[16];
    const uint32_t all = compact_scan_blocks(blockCounts, blocks, s_a, [](uint32_t, uint32_t) {});
    const uint32_t rects = compact_scan_blocks(rectBefore, lightCount, s_b, [](uint32_t, uint32_t) {});
    if (threadIdx.x == 0u) {
        offsets[cells + 1u] = all;
        *total = all;
        rectBefore[lightCount] = rects;
    }
}

extern "C" __global__ __launch_bounds__(1024) void pt_lgrid_emit(GridBuildArgs A, uint32_t* __restrict__ offsets, const uint32_t* __restrict__ blockCounts,
                                                                 uint32_t* __restrict__ indices, uint32_t capacity)
{
    __shared__ uint32_t s_sum[16];
    const uint32_t cell = blockIdx.x * kLightGridBlock + threadIdx.x;
    const uint32_t n = cell <= A.cells ? offsets[cell] : 0u;
    uint32_t all;
    const uint32_t base = blockCounts[blockIdx.x] + compact_scan_threads(n, s_sum, all);
    walk_cell(A, cell, [&](uint32_t k, uint32_t l) {
        if (k < n && base + k < capacity) indices[base + k] = l;                 // what was counted is what is written
    });
    if (cell <= A.cells) offsets[cell] = base;
}

namespace {

GridBuildArgs build_args(const DScene& S, uint32_t lightCount, const ptlgrid::Grid& g)
{
    GridBuildArgs A;
    A.lights = S.lights; A.lightConst = S.lightConst;
    A.lightCount = lightCount; A.cells = ptlgrid::cell_count(g);
    A.g = g;
    return A;
}

} // namespace

hipError_t pt_launch_light_grid_count(const DScene& S, uint32_t lightCount, const ptlgrid::Grid& g, uint32_t* offsets, uint32_t* blockCounts,
                                      uint32_t* rectBefore, uint32_t* total, hipStream_t stream)
{
    const GridBuildArgs A = build_args(S, lightCount, g);
    if (lightCount && (!S.lights || !S.lightConst)) return hipErrorInvalidValue;
    const uint32_t blocks = pt_light_grid_blocks(A.cells);
    hipLaunchKernelGGL(pt_lgrid_count, dim3(blocks), dim3(kLightGridBlock), 0, stream, A, offsets, blockCounts, rectBefore);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pt_lgrid_scan, dim3(1), dim3(1024), 0, stream, blockCounts, blocks, rectBefore, lightCount, offsets, A.cells, total);
    return hipGetLastError();
}

hipError_t pt_launch_light_grid_emit(const DScene& S, uint32_t lightCount, const ptlgrid::Grid& g, uint32_t* offsets, const uint32_t* blockCounts,
                                     uint32_t* indices, uint32_t capacity, hipStream_t stream)
{
    const GridBuildArgs A = build_args(S, lightCount, g);
    hipLaunchKernelGGL(pt_lgrid_emit, dim3(pt_light_grid_blocks(A.cells)), dim3(kLightGridBlock), 0, stream, A, offsets, blockCounts, indices, capacity);
    return hipGetLastError();
}
