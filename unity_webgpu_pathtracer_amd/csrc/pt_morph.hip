// pt_morph.hip — morph targets, then the skin, on the MI355X (include/ptmi_plugin.h Part 12): the rule of
// morph_rule.h in two kernels, each in a plain and a skinned form.  pt_morph_vertices runs one lane per corner and one wave per
// slice of the position stream (64 corners): a 16-byte coalesced load of the rest position, then one fully coalesced 1 KB request
// per slot of the slice -- the trip count is the slice's slot count, the same for the whole wave; a lane applies slot s only if
// s < its own count, so padding is loaded and dropped, never applied.  Four slots are in flight at a time: an entry names the
// weight it needs, so one slot at a time is two dependent loads per slot (measured: 26 against 23 us for 8 dense targets on the
// Sponza-class scene, 46 against 32 us in pt_morph_attrs).  The weight of an entry comes from global memory (at most 4 KB,
// L2-resident).  Under SKIN the blend matrix and skin_point of Part 11 follow.  The positions are reduced to one box per
// workgroup as pt_skin_vertices does, and pt_skin.hip's fold finishes them.  pt_morph_attrs runs one lane per 16-byte row of the
// attribute records and writes every record once, straight where the scene reads it.  No atomics: the same input gives the same bits.
#include "pt_morph.h"
#include "morph_rule.h"

using namespace ptskin;
using namespace ptmorph;

namespace {

// the blend matrix of vertex i (as pt_skin.hip's)
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

// (x, y, z) folded with slots 0 ... slots - 1 of the corner's column; only slots below the corner's count are applied
__device__ __forceinline__ void fold(const float4* __restrict__ column, uint32_t slots, uint32_t count, const float* __restrict__ weights, float& x, float& y, float& z)
{
    uint32_t s = 0;
    // four slots at a time: the four entry loads go out together, then the four weight loads (every slot below `slots` is stored,
    // and padding names target 0, so all eight are in bounds), then the listed ones are applied in order
    for (; s + 4u <= slots; s += 4u) {
        float4 e[4];
        float w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = column[(size_t)(s + k) * 64u];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = weights[__float_as_uint(e[k].w)];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (s + k < count) {
                x = morph_step(x, w[k], e[k].x);
                y = morph_step(y, w[k], e[k].y);
                z = morph_step(z, w[k], e[k].z);
            }
    }
    for (; s < slots; ++s) {
        if (s < count) {
            const float4 e = column[(size_t)s * 64u];
            const float w = weights[__float_as_uint(e.w)];
            x = morph_step(x, w, e.x);
            y = morph_step(y, w, e.y);
            z = morph_step(z, w, e.z);
        }
    }
}

template <bool SKIN>
__global__ __launch_bounds__(256) void pt_morph_vertices(PTMorphArgs A, PTSkinArgs K, float4* __restrict__ outVerts, float* __restrict__ partial)
{
    __shared__ float waveBox[4][6];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < A.triCount * 3u) {
        const float4 v = A.rest[i];
        float p[3] = {v.x, v.y, v.z};
        // the wave's 64 corners are one slice: base and slot count are wave-uniform
        const uint32_t base = A.position.sliceBase[i >> 6], slots = (A.position.sliceBase[(i >> 6) + 1u] - base) >> 6;
        fold(A.position.entries + base + (i & 63u), slots, A.position.count[i], A.weights, p[0], p[1], p[2]);
        if (SKIN) {
            float B[12];
            blend_matrix(K, i, B);
            skin_point(B, p[0], p[1], p[2], p);
        }
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

// row r of a record: 0 ... 2 the corners' normals, 3 ... 5 their tangents (xyz morphed, the pad or the tangent's w copied), 6 and 7 copied
template <bool SKIN>
__global__ __launch_bounds__(256) void pt_morph_attrs(PTMorphArgs A, PTSkinArgs K, float4* __restrict__ dst)
{
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= A.triCount * 8u) return;
    float4 v = A.restAttrs[row];
    const uint32_t r = row & 7u;
    if (r < 6u) {
        const uint32_t corner = (row >> 3) * 3u + (r < 3u ? r : r - 3u);
        const float4* entries = r < 3u ? A.normal.entries : A.tangent.entries;
        const uint32_t* counts = r < 3u ? A.normal.count : A.tangent.count;
        const uint32_t* sliceBase = r < 3u ? A.normal.sliceBase : A.tangent.sliceBase;
        const float rest[3] = {v.x, v.y, v.z};
        float m[3] = {v.x, v.y, v.z}, o[3];
        uint32_t count = 0;
        if (entries) {
            count = counts[corner];
            fold(entries + sliceBase[corner >> 6] + (corner & 63u), count, count, A.weights, m[0], m[1], m[2]);
        }
        if (SKIN) {
            float B[12];
            blend_matrix(K, corner, B);
            morph_skin_direction(B, m, rest, o);
            v.x = o[0]; v.y = o[1]; v.z = o[2];
        } else if (count) {                                     // no entry and no palette: the rest row, bit for bit
            morph_direction(m, rest, o);
            v.x = o[0]; v.y = o[1]; v.z = o[2];
        }
    }
    dst[row] = v;
}

} // namespace

size_t pt_morph_work_floats(uint32_t triCount) { return (size_t)6u * (1u + (triCount * 3u + 255u) / 256u); }

hipError_t pt_launch_morph_vertices(const PTMorphArgs& A, const PTSkinArgs* skin, float4* outVerts, float* work, hipStream_t stream)
{
    const uint32_t blocks = (A.triCount * 3u + 255u) / 256u;
    if (skin) hipLaunchKernelGGL(pt_morph_vertices<true>, dim3(blocks), dim3(256), 0, stream, A, *skin, outVerts, work + 6);
    else hipLaunchKernelGGL(pt_morph_vertices<false>, dim3(blocks), dim3(256), 0, stream, A, PTSkinArgs{}, outVerts, work + 6);
    return pt_launch_skin_bounds_fold(work + 6, blocks, work, stream);
}

hipError_t pt_launch_morph_attrs(const PTMorphArgs& A, const PTSkinArgs* skin, float4* dstAttrs, hipStream_t stream)
{
    const dim3 grid((A.triCount * 8u + 255u) / 256u);
    if (skin) hipLaunchKernelGGL(pt_morph_attrs<true>, grid, dim3(256), 0, stream, A, *skin, dstAttrs);
    else hipLaunchKernelGGL(pt_morph_attrs<false>, grid, dim3(256), 0, stream, A, PTSkinArgs{}, dstAttrs);
    return hipGetLastError();
}
