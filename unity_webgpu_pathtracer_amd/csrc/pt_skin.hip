// pt_skin.hip — linear-blend skinning on the MI355X (include/ptmi_plugin.h Part 11): the rule of skin_rule.h in
// three kernels.  pt_skin_vertices runs one lane per vertex: a 16-byte, an 8-byte and a 16-byte coalesced load (rest position,
// joints, weights), four divergent 48-byte reads of the palette (global memory: at most 48 KB, L2-resident, and neighbouring
// vertices share joints), one 16-byte store; the lanes' positions are reduced to one box per workgroup.  pt_skin_bounds_fold
// folds those boxes in index order.  pt_skin_attrs runs one lane per 16-byte row of the attribute records and writes every
// record once, straight where the scene reads it.  No atomics: the same input gives the same bits.
#include "pt_skin.h"
#include "skin_rule.h"

using namespace ptskin;

namespace {

// the blend matrix of vertex i
__device__ __forceinline__ void blend_matrix(const PTSkinArgs& A, uint32_t i, float B[12])
{
    const uint2 j = A.joints[i];
    const float4 w = A.weights[i];
    const float4* m0 = A.palette + 3u * (j.x & 0xFFFFu);
    const float4* m1 = A.palette + 3u * (j.x >> 16);
    const float4* m2 = A.palette + 3u * (j.y & 0xFFFFu);
    const float4* m3 = A.palette + 3u * (j.y >> 16);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float4 a = m0[r], b = m1[r], c = m2[r], d = m3[r];
        B[4 * r] = skin_blend(w.x, a.x, w.y, b.x, w.z, c.x, w.w, d.x);
        B[4 * r + 1] = skin_blend(w.x, a.y, w.y, b.y, w.z, c.y, w.w, d.y);
        B[4 * r + 2] = skin_blend(w.x, a.z, w.y, b.z, w.z, c.z, w.w, d.z);
        B[4 * r + 3] = skin_blend(w.x, a.w, w.y, b.w, w.z, c.w, w.w, d.w);
    }
}

__device__ __forceinline__ float wave_min(float v)
{
    for (int off = 32; off > 0; off >>= 1) v = skin_min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
    for (int off = 32; off > 0; off >>= 1) v = skin_max(v, __shfl_xor(v, off, 64));
    return v;
}

__global__ __launch_bounds__(256) void pt_skin_vertices(PTSkinArgs A, float4* __restrict__ outVerts, float* __restrict__ partial)
{
    __shared__ float waveBox[4][6];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < A.triCount * 3u) {
        float B[12], p[3];
        blend_matrix(A, i, B);
        const float4 v = A.rest[i];
        skin_point(B, v.x, v.y, v.z, p);
        outVerts[i] = make_float4(p[0], p[1], p[2], 0.0f);
        for (int a = 0; a < 3; ++a) mn[a] = mx[a] = p[a];
    }
    for (int a = 0; a < 3; ++a) { mn[a] = wave_min(mn[a]); mx[a] = wave_max(mx[a]); }
    if ((threadIdx.x & 63u) == 0u)
        for (int a = 0; a < 3; ++a) { waveBox[threadIdx.x >> 6][a] = mn[a]; waveBox[threadIdx.x >> 6][3 + a] = mx[a]; }
    __syncthreads();
    if (threadIdx.x < 6u) {
        const uint32_t a = threadIdx.x;
        float acc = waveBox[0][a];
        for (int w = 1; w < 4; ++w) acc = a < 3u ? skin_min(acc, waveBox[w][a]) : skin_max(acc, waveBox[w][a]);
        partial[(size_t)blockIdx.x * 6u + a] = acc;
    }
}

__global__ __launch_bounds__(64) void pt_skin_bounds_fold(const float* __restrict__ partial, uint32_t count, float* __restrict__ out)
{
    // one wave: lane l folds boxes l, l + 64, ... in order, then the lanes are reduced
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t b = threadIdx.x; b < count; b += 64u)
        for (int a = 0; a < 3; ++a) { mn[a] = skin_min(mn[a], partial[(size_t)b * 6u + a]); mx[a] = skin_max(mx[a], partial[(size_t)b * 6u + 3u + a]); }
    for (int a = 0; a < 3; ++a) { mn[a] = wave_min(mn[a]); mx[a] = wave_max(mx[a]); }
    if (threadIdx.x == 0u)
        for (int a = 0; a < 3; ++a) { out[a] = mn[a]; out[3 + a] = mx[a]; }
}

// row r of a record: 0 ... 2 the corners' normals, 3 ... 5 their tangents (xyz skinned, the pad copied), 6 and 7 copied
__global__ __launch_bounds__(256) void pt_skin_attrs(PTSkinArgs A, float4* __restrict__ dst)
{
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= A.triCount * 8u) return;
    float4 v = A.restAttrs[row];
    const uint32_t r = row & 7u;
    if (r < 6u) {
        float B[12], o[3];
        blend_matrix(A, (row >> 3) * 3u + (r < 3u ? r : r - 3u), B);
        skin_direction(B, v.x, v.y, v.z, o);
        v.x = o[0]; v.y = o[1]; v.z = o[2];
    }
    dst[row] = v;
}

} // namespace

size_t pt_skin_work_floats(uint32_t triCount) { return (size_t)6u * (1u + (triCount * 3u + 255u) / 256u); }

hipError_t pt_launch_skin_vertices(const PTSkinArgs& A, float4* outVerts, float* work, hipStream_t stream)
{
    const uint32_t blocks = (A.triCount * 3u + 255u) / 256u;
    hipLaunchKernelGGL(pt_skin_vertices, dim3(blocks), dim3(256), 0, stream, A, outVerts, work + 6);
    hipLaunchKernelGGL(pt_skin_bounds_fold, dim3(1), dim3(64), 0, stream, work + 6, blocks, work);
    return hipGetLastError();
}

hipError_t pt_launch_skin_bounds_fold(const float* partial, uint32_t count, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(pt_skin_bounds_fold, dim3(1), dim3(64), 0, stream, partial, count, out);
    return hipGetLastError();
}

hipError_t pt_launch_skin_attrs(const PTSkinArgs& A, float4* dstAttrs, hipStream_t stream)
{
    hipLaunchKernelGGL(pt_skin_attrs, dim3((A.triCount * 8u + 255u) / 256u), dim3(256), 0, stream, A, dstAttrs);
    return hipGetLastError();
}
