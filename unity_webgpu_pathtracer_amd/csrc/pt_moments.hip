// pt_moments.hip — per-pixel second moments across progressive passes and the noise metric read from them
// (include/ptmi_plugin.h Part 6: PTAccumulateMoments / PTMeasureNoise).
//
// Accumulate: elementwise, one lane per pixel (a wave takes 64 consecutive pixels), 16-byte accesses: reads Out and Acc (32 B),
// reads and rewrites the two moment planes (64 B).  Every operation is one IEEE float32 operation (-ffp-contract=off).
//
// Noise: one 256-thread workgroup per 16x16 block -- the unit of the filter and of tile ownership.  A 256-bin histogram in
// LDS (integer atomics), non-empty bins added to the global histogram with integer atomics, the maximum as an integer atomic
// max on the bits (eps >= 0, so the bits order as the values do), the block's sum of eps reduced in a fixed order and written
// to a slab; pt_noise_finish (one workgroup) folds the slab in block order.  No float atomics: two calls on the same data give
// the same bytes.
#include "pt_launch.h"

namespace {

PT_DEV float mo_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }      // dn_lum's order

} // namespace

extern "C" __global__ __launch_bounds__(256) void pt_moments_accumulate(uint32_t pixels, float f, const float4* __restrict__ out,
                                                                        const float4* __restrict__ acc, float4* __restrict__ plane0,
                                                                        float4* __restrict__ plane1)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= pixels) return;
    const float4 o = out[p], a = acc[p];
    const float dr = o.x - a.x, dg = o.y - a.y, db = o.z - a.z;
    const float dl = mo_lum(dr, dg, db);
    float4 s0 = plane0[p], s1 = plane1[p];
    s0.x += (dr * dr) * f; s0.y += (dg * dg) * f; s0.z += (db * db) * f; s0.w += (dl * dl) * f;
    s1.x += (dr * dg) * f; s1.y += (dr * db) * f; s1.z += (dg * db) * f;
    plane0[p] = s0;
    plane1[p] = make_float4(s1.x, s1.y, s1.z, 0.0f);
}

// The same update over a list of 16x16 blocks (PTAccumulateMomentsActive): workgroup e takes table entry e = {block id, bits of the
// block's f}; a pixel outside the list has Out == Acc, so skipping it is exact and the traffic follows the listed area.
extern "C" __global__ __launch_bounds__(256) void pt_moments_accumulate_blocks(const uint2* __restrict__ table, uint32_t width, uint32_t height,
                                                                               const float4* __restrict__ out, const float4* __restrict__ acc,
                                                                               float4* __restrict__ plane0, float4* __restrict__ plane1)
{
    const uint2 entry = table[blockIdx.x];
    const uint32_t blocksX = (width + 15u) / 16u;
    const uint32_t by = entry.x / blocksX, bx = entry.x - by * blocksX;
    const uint32_t x = bx * 16u + (threadIdx.x & 15u), y = by * 16u + (threadIdx.x >> 4);
    if (x >= width || y >= height) return;
    const float f = __uint_as_float(entry.y);
    const size_t p = (size_t)y * width + x;
    const float4 o = out[p], a = acc[p];
    const float dr = o.x - a.x, dg = o.y - a.y, db = o.z - a.z;
    const float dl = mo_lum(dr, dg, db);
    float4 s0 = plane0[p], s1 = plane1[p];
    s0.x += (dr * dr) * f; s0.y += (dg * dg) * f; s0.z += (db * db) * f; s0.w += (dl * dl) * f;
    s1.x += (dr * dg) * f; s1.y += (dr * db) * f; s1.z += (dg * db) * f;
    plane0[p] = s0;
    plane1[p] = make_float4(s1.x, s1.y, s1.z, 0.0f);
}

extern "C" __global__ __launch_bounds__(256) void pt_noise_blocks(PTNoiseArgs A, const float4* __restrict__ frame,
                                                                  const float4* __restrict__ plane0, uint32_t* __restrict__ stats,
                                                                  float* __restrict__ blockSums, float* __restrict__ tiles,
                                                                  const float* __restrict__ blockInvDof)
{
    __shared__ uint32_t s_hist[256];
    __shared__ float s_part[4];
    __shared__ uint32_t s_max, s_below;
    const uint32_t t = threadIdx.x;
    const uint32_t block = blockIdx.y * gridDim.x + blockIdx.x;
    if ((blockIdx.x + blockIdx.y) % A.world != A.rank) {            // another rank's block (uniform over the workgroup)
        if (t == 0u) { blockSums[block] = 0.0f; tiles[block] = 0.0f; }
        return;
    }
    s_hist[t] = 0u;
    if (t == 0u) { s_max = 0u; s_below = 0u; }
    __syncthreads();
    const uint32_t x = blockIdx.x * 16u + (t & 15u), y = blockIdx.y * 16u + (t >> 4);
    const bool inside = x < A.width && y < A.height;
    const float invDof = blockInvDof ? blockInvDof[block] : A.invDof;      // one workgroup is one block: uniform
    float eps = 0.0f;
    if (inside) {
        const size_t p = (size_t)y * A.width + x;
        const float4 c = frame[p];
        const float sll = plane0[p].w;
        const float l = mo_lum(c.x, c.y, c.z);
        eps = __builtin_sqrtf(sll * invDof) / (l + A.relFloor);
        if (!(eps >= 0.0f)) eps = __builtin_inff();                 // NaN or negative
        const uint32_t bits = __float_as_uint(eps) & 0x7FFFFFFFu;   // -0 counts as 0
        eps = __uint_as_float(bits);
        int bin = (int)(bits >> 20) - ((127 - 24) << 3);
        bin = bin < 0 ? 0 : (bin > 255 ? 255 : bin);
        atomicAdd(&s_hist[bin], 1u);
        atomicMax(&s_max, bits);
        if (eps <= A.threshold) atomicAdd(&s_below, 1u);
    }
    // the block's sum in a fixed order: a butterfly inside each wave, then the four waves in wave order
    float sum = eps;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((t & 63u) == 0u) s_part[t >> 6] = sum;
    __syncthreads();
    if (s_hist[t] != 0u) atomicAdd(&stats[t], s_hist[t]);
    if (t == 0u) {
        const float total = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
        const uint32_t bw = A.width - blockIdx.x * 16u, bh = A.height - blockIdx.y * 16u;
        const uint32_t count = (bw < 16u ? bw : 16u) * (bh < 16u ? bh : 16u);
        blockSums[block] = total;
        tiles[block] = total / (float)count;
        atomicMax(&stats[PT_NOISE_MAX], s_max);
        if (s_below != 0u) atomicAdd(&stats[PT_NOISE_BELOW], s_below);
    }
}

// One workgroup: thread t folds the contiguous slice [t * per, (t + 1) * per) of the slab in block order, then the 256 partial
// sums are combined pairwise with the lower slice first.
extern "C" __global__ __launch_bounds__(256) void pt_noise_finish(uint32_t blocks, const float* __restrict__ blockSums,
                                                                  uint32_t* __restrict__ stats)
{
    __shared__ float s_sum[256];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (blocks + 255u) / 256u;
    const uint32_t lo = t * per;
    const uint32_t hi = lo + per < blocks ? lo + per : blocks;
    float sum = 0.0f;
    for (uint32_t b = lo; b < hi; ++b) sum += blockSums[b];
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t w = 1u; w < 256u; w <<= 1) {
        if ((t & (2u * w - 1u)) == 0u) s_sum[t] += s_sum[t + w];
        __syncthreads();
    }
    if (t == 0u) stats[PT_NOISE_SUM] = __float_as_uint(s_sum[0]);
}

hipError_t pt_launch_moments_accumulate(uint32_t pixels, float f, const float4* out, const float4* acc, float4* plane0,
                                        float4* plane1, hipStream_t stream)
{
    if (pixels == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_moments_accumulate, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, pixels, f, out, acc, plane0, plane1);
    return hipGetLastError();
}

hipError_t pt_launch_moments_accumulate_blocks(uint32_t entries, const uint2* table, uint32_t width, uint32_t height, const float4* out,
                                               const float4* acc, float4* plane0, float4* plane1, hipStream_t stream)
{
    if (entries == 0u) return hipSuccess;
    hipLaunchKernelGGL(pt_moments_accumulate_blocks, dim3(entries), dim3(256), 0, stream, table, width, height, out, acc, plane0, plane1);
    return hipGetLastError();
}

hipError_t pt_launch_noise(const PTNoiseArgs& A, const float4* frame, const float4* plane0, uint32_t* stats, float* blockSums,
                           float* tiles, hipStream_t stream, const float* blockInvDof)
{
    const dim3 grid((A.width + 15u) / 16u, (A.height + 15u) / 16u);
    hipLaunchKernelGGL(pt_noise_blocks, grid, dim3(256), 0, stream, A, frame, plane0, stats, blockSums, tiles, blockInvDof);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pt_noise_finish, dim3(1), dim3(256), 0, stream, grid.x * grid.y, blockSums, stats);
    return hipGetLastError();
}
