// pt_refit.hip — CWBVH refit on the MI355X (include/ptmi_plugin.h Part 9): the rule of bvh_refit.h in two
// kernels.  pt_refit_tris rewrites the triangle records; pt_refit_level rewrites the nodes of ONE tree level, one thread per
// node, and is launched once per level from the deepest to the root.  A launch reads what deeper launches wrote (nodeBox) and
// what never changes (row n1, imask, primIdx); stream order is the only synchronisation -- no atomics, counters or fences.
#include "pt_refit.h"
#include "bvh_refit.h"

using namespace ptbvh;

namespace {

__global__ __launch_bounds__(256) void pt_refit_tris(PTRefitArgs A)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= A.triCount) return;
    float4* rec = A.tris + (size_t)A.triOff + (size_t)r * 3u;
    const float4 r2 = rec[2];
    const uint32_t prim = __float_as_uint(r2.w);
    const float4 v0 = A.verts[3u * prim], v1 = A.verts[3u * prim + 1u], v2 = A.verts[3u * prim + 2u];
    rec[0] = make_float4(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z, 0.0f);
    rec[1] = make_float4(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z, 0.0f);
    rec[2] = make_float4(v0.x, v0.y, v0.z, r2.w);
}

// The box of occupied slot `m` (its meta byte): an inner child's refitted box, or the fold over the original vertices of a
// leaf's 1-3 triangles in record order.  inner: inner slots seen so far in this node, advanced.
__device__ __forceinline__ void slot_box(const PTRefitArgs& A, uint32_t m, uint32_t childBase, uint32_t triBase, uint32_t& inner, float mn[3], float mx[3])
{
    if (refit_slot_inner(m)) {
        const float* b = A.nodeBox + (size_t)(A.nodeOff + childBase + inner++) * 6u;
        for (int a = 0; a < 3; ++a) { mn[a] = b[a]; mx[a] = b[3 + a]; }
        return;
    }
    for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
    const uint32_t count = __popc(m >> 5);
    const float4* rec = A.tris + (size_t)A.triOff + triBase + 3u * (m & 31u);
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t prim = __float_as_uint(rec[3u * j + 2u].w);
        for (uint32_t v = 0; v < 3u; ++v) {
            const float4 p = A.verts[3u * prim + v];
            mn[0] = refit_min(mn[0], p.x); mx[0] = refit_max(mx[0], p.x);
            mn[1] = refit_min(mn[1], p.y); mx[1] = refit_max(mx[1], p.y);
            mn[2] = refit_min(mn[2], p.z); mx[2] = refit_max(mx[2], p.z);
        }
    }
}

// The slots are walked twice -- once for the node's box, once to quantise against it -- instead of keeping eight child boxes
// in an array indexed by the slot, which would live in scratch.  The second walk's loads hit the cache.
__global__ __launch_bounds__(64) void pt_refit_level(PTRefitArgs A, uint32_t first, uint32_t end)
{
    const uint32_t k = first + blockIdx.x * 64u + threadIdx.x;
    if (k >= end) return;
    const uint32_t node = A.order[k];
    uint4* n = A.nodes + (size_t)node * 5u;
    const uint32_t imaskBits = n[0].w & 0xFF000000u;
    const uint4 n1 = n[1];                                          // childBaseIndex, triBaseIndex, meta[8]
    float nmn[3], nmx[3];
    for (int a = 0; a < 3; ++a) { nmn[a] = INFINITY; nmx[a] = -INFINITY; }
    uint32_t inner = 0;
    for (uint32_t s = 0; s < 8u; ++s) {
        const uint32_t m = ((s < 4u ? n1.z : n1.w) >> (8u * (s & 3u))) & 255u;
        if (m == 0u) continue;
        float mn[3], mx[3];
        slot_box(A, m, n1.x, n1.y, inner, mn, mx);
        for (int a = 0; a < 3; ++a) { nmn[a] = refit_min(nmn[a], mn[a]); nmx[a] = refit_max(nmx[a], mx[a]); }
    }
    float* box = A.nodeBox + (size_t)node * 6u;
    for (int a = 0; a < 3; ++a) { box[a] = nmn[a]; box[3 + a] = nmx[a]; }
    int e[3];
    float p[3];
    for (int a = 0; a < 3; ++a) { e[a] = refit_exponent(nmx[a] - nmn[a]); p[a] = ldexpf(1.0f, e[a]); }
    unsigned long long qlo[3] = {0ull, 0ull, 0ull}, qhi[3] = {0ull, 0ull, 0ull};      // byte s of axis a: slot s
    inner = 0;
    for (uint32_t s = 0; s < 8u; ++s) {
        const uint32_t m = ((s < 4u ? n1.z : n1.w) >> (8u * (s & 3u))) & 255u;
        if (m == 0u) continue;
        float mn[3], mx[3];
        slot_box(A, m, n1.x, n1.y, inner, mn, mx);
        for (int a = 0; a < 3; ++a) {
            qlo[a] |= (unsigned long long)refit_quant_lo(mn[a], nmn[a], p[a]) << (8u * s);
            qhi[a] |= (unsigned long long)refit_quant_hi(mx[a], nmn[a], p[a]) << (8u * s);
        }
    }
    n[0] = make_uint4(__float_as_uint(nmn[0]), __float_as_uint(nmn[1]), __float_as_uint(nmn[2]),
                      ((uint32_t)e[0] & 255u) | (((uint32_t)e[1] & 255u) << 8) | (((uint32_t)e[2] & 255u) << 16) | imaskBits);
    n[2] = make_uint4((uint32_t)qlo[0], (uint32_t)(qlo[0] >> 32), (uint32_t)qlo[1], (uint32_t)(qlo[1] >> 32));
    n[3] = make_uint4((uint32_t)qlo[2], (uint32_t)(qlo[2] >> 32), (uint32_t)qhi[0], (uint32_t)(qhi[0] >> 32));
    n[4] = make_uint4((uint32_t)qhi[1], (uint32_t)(qhi[1] >> 32), (uint32_t)qhi[2], (uint32_t)(qhi[2] >> 32));
}

// one thread per 16-byte row; materialIndex is word 2 of a record's last row
__global__ __launch_bounds__(256) void pt_refit_attrs(float4* __restrict__ dst, const float4* __restrict__ src, uint32_t rows, uint32_t materialCount)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rows) return;
    float4 v = src[i];
    if ((i & 7u) == 7u && __float_as_uint(v.z) >= materialCount) v.z = dst[i].z;
    dst[i] = v;
}

} // namespace

hipError_t pt_launch_refit(const PTRefitArgs& A, const uint32_t* levelStart, uint32_t levels, hipStream_t stream, uint32_t* launches)
{
    hipLaunchKernelGGL(pt_refit_tris, dim3((A.triCount + 255u) / 256u), dim3(256), 0, stream, A);
    for (uint32_t lv = levels; lv-- > 0u;) {
        const uint32_t first = levelStart[lv], end = levelStart[lv + 1];
        hipLaunchKernelGGL(pt_refit_level, dim3((end - first + 63u) / 64u), dim3(64), 0, stream, A, first, end);
    }
    if (launches) *launches += 1u + levels;
    return hipGetLastError();
}

hipError_t pt_launch_refit_attrs(float4* dst, const float4* src, uint32_t count, uint32_t materialCount, hipStream_t stream)
{
    const uint32_t rows = count * 8u;
    hipLaunchKernelGGL(pt_refit_attrs, dim3((rows + 255u) / 256u), dim3(256), 0, stream, dst, src, rows, materialCount);
    return hipGetLastError();
}
