// pt_quality.hip — the tree-quality measure on the MI355X behind PTMeasureGeometry (include/ptmi_plugin.h Part 10, DESIGN.md
// 5.15): the rule of bvh_quality.h in one kernel.  pt_geometry_quality runs one lane per node over the BLAS's node list (the
// refit plan's order), reads the node's 80 bytes, and reduces its term over the wave and the workgroup into one partial sum per
// workgroup; pt_geometry_quality_fold adds the partials in index order.  No atomics: the same tree gives the same bits.
#include "pt_quality.h"
#include "bvh_quality.h"

using namespace ptbvh;

namespace {

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// out[0]: filled by the fold; out[1]: the root's half area (the lane of order[0])
__global__ __launch_bounds__(256) void pt_geometry_quality(const uint4* __restrict__ nodes, const uint32_t* __restrict__ order, uint32_t count,
                                                           double* __restrict__ partial, double* __restrict__ out)
{
    __shared__ double waveSum[4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    double term = 0.0;
    if (k < count) {
        const uint4* n = nodes + (size_t)order[k] * 5u;
        const uint4 r0 = n[0], r1 = n[1], r2 = n[2], r3 = n[3], r4 = n[4];
        const uint32_t w[20] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w, r4.x, r4.y, r4.z, r4.w};
        double fold;
        term = quality_node_term(w, fold);
        if (k == 0u) out[1] = fold;
    }
    term = wave_sum(term);
    if ((threadIdx.x & 63u) == 0u) waveSum[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0u) partial[blockIdx.x] = ((waveSum[0] + waveSum[1]) + waveSum[2]) + waveSum[3];
}

__global__ __launch_bounds__(64) void pt_geometry_quality_fold(const double* __restrict__ partial, uint32_t count, double* __restrict__ out)
{
    // one wave: lane l adds partials l, l + 64, ... in order, then the lanes are reduced
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < count; i += 64u) s += partial[i];
    s = wave_sum(s);
    if (threadIdx.x == 0u) out[0] = s;
}

} // namespace

size_t pt_quality_work_bytes(uint32_t nodeCount) { return (size_t)(2u + (nodeCount + 255u) / 256u) * sizeof(double); }

hipError_t pt_launch_geometry_quality(const uint4* nodes, const uint32_t* order, uint32_t nodeCount, double* work, hipStream_t stream)
{
    const uint32_t blocks = (nodeCount + 255u) / 256u;
    hipLaunchKernelGGL(pt_geometry_quality, dim3(blocks), dim3(256), 0, stream, nodes, order, nodeCount, work + 2, work);
    hipLaunchKernelGGL(pt_geometry_quality_fold, dim3(1), dim3(64), 0, stream, work + 2, blocks, work);
    return hipGetLastError();
}
