// pt_unwrap.hip — lightmap UVs on the MI355X (include/ptmi_plugin.h Part 23): the rule of unwrap_rule.h in kernels,
// one lane per triangle record, primitive, corner or sorted entry.
//   pt_uw_corners      record or vertex rows -> corners[3 p .. 3 p + 2] (+ 0.0f applied), cls[p]; the first sort's keys (z) and values
//   rocprim::radix_sort_pairs x 3, stable, over the z, y and x words (pt_uw_gather_key in between): corners with equal 96 bits
//                      are adjacent (a library sort, as in bvh_builder_gpu.hip: not part of the render hot path)
//   pt_uw_vertex_count / pt_uw_scan / pt_uw_vertex_ids      run heads and the compaction of pt_compact.h: a vertex id per corner
//   pt_uw_edge_keys    (lo id, hi id, class) per edge of an included primitive, all ones for an excluded one; value = primitive
//   rocprim::radix_sort_pairs over the 64 bits: equal neighbours are linked
//   pt_uw_hook / pt_uw_compress      one sweep: every link hooks the larger of its two roots under the smaller with atomicMin, then
//                      every label becomes its root.  Labels only fall and label[p] <= p, so there is no cycle; at the fixed point
//                      every link has one root, which is the lowest primIdx of its component whatever the arrival order.
//   pt_uw_count_tris / pt_uw_head_count / pt_uw_scan      triangles per label, the heads label[p] == p counted and scanned
//   pt_uw_chart_init / pt_uw_extents / pt_uw_chart_finish  the records; extents by integer atomicMin / atomicMax on order keys
//   pt_uw_emit         the six UVs of a primitive: one 32-byte chart record, one 8-byte origin, 24 bytes out
// The only atomics are integer min, max and add on 4-byte words: the same input gives the same bytes.
#include <rocprim/device/device_radix_sort.hpp>

#include "pt_unwrap.h"
#include "pt_compact.h"
#include "unwrap_rule.h"

using namespace ptunwrap;

namespace {

constexpr uint64_t kNoEdge = ~0ull;

__device__ __forceinline__ uint32_t wave_count(bool flag) { return (uint32_t)__popcll(__ballot(flag)); }
__device__ __forceinline__ bool first_lane() { return rank_below(__ballot(true)) == 0u; }

// The corners of what lane t stands for -- primitive t of the vertex rows, or record t -- with + 0.0f applied, its primitive and
// class.  false: t is past the BLAS, or the record names no primitive of it.
__device__ __forceinline__ bool load_corners(const float4* __restrict__ tris, const float4* __restrict__ vertices, uint32_t T, uint32_t t, uint32_t& p,
                                             float c[3][3], uint32_t& cls)
{
    if (t >= T) return false;
    if (vertices) {
        const float4 a = vertices[(size_t)t * 3u], b = vertices[(size_t)t * 3u + 1u], d = vertices[(size_t)t * 3u + 2u];
        p = t;
        c[0][0] = a.x; c[0][1] = a.y; c[0][2] = a.z; c[1][0] = b.x; c[1][1] = b.y; c[1][2] = b.z; c[2][0] = d.x; c[2][1] = d.y; c[2][2] = d.z;
    } else {
        const float4 e2 = tris[(size_t)t * 3u], e1 = tris[(size_t)t * 3u + 1u], v0 = tris[(size_t)t * 3u + 2u];
        p = unwrap_bits(v0.w);
        if (p >= T) return false;
        const float a0[3] = {v0.x, v0.y, v0.z}, a1[3] = {e1.x, e1.y, e1.z}, a2[3] = {e2.x, e2.y, e2.z};
        unwrap_record_corners(a0, a1, a2, c);
    }
    cls = unwrap_class(c);
    return true;
}

__global__ __launch_bounds__(256) void pt_uw_corners(PTUnwrapArgs A)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < A.triCount) {
        A.label[t] = t; A.triOfLabel[t] = 0u;
        A.valA[(size_t)t * 3u] = t * 3u; A.valA[(size_t)t * 3u + 1u] = t * 3u + 1u; A.valA[(size_t)t * 3u + 2u] = t * 3u + 2u;
    }
    uint32_t p = 0u, cls = kExcluded;
    float c[3][3];
    const bool in = load_corners(A.tris, A.vertices, A.triCount, t, p, c, cls);
    if (in) {
        A.cls[p] = cls;
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) {
            A.corners[(size_t)p * 3u + k] = make_float4(c[k][0], c[k][1], c[k][2], 0.0f);
            A.keyA[(size_t)p * 3u + k] = unwrap_bits(c[k][2]);
        }
    }
    const uint32_t n = wave_count(in && cls == kExcluded);
    if (n && first_lane()) atomicAdd(A.small + 0, n);
}

// the key of the next pass: word `comp` (1: y, 0: x) of the corner at place j of the order so far
__global__ __launch_bounds__(256) void pt_uw_gather_key(const float4* __restrict__ corners, const uint32_t* __restrict__ order, uint32_t n, uint32_t comp,
                                                        uint32_t* __restrict__ key)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = order[j];
    if (i >= n) { key[j] = 0u; return; }                            // cannot happen: the values are a permutation
    const float4 v = corners[i];
    key[j] = unwrap_bits(comp ? v.y : v.x);
}

// place j of the sorted order starts a run of equal corners
__device__ __forceinline__ bool run_head(const float4* __restrict__ corners, const uint32_t* __restrict__ order, uint32_t n, uint32_t j)
{
    if (j >= n) return false;
    if (j == 0u) return true;
    const uint32_t i = order[j], h = order[j - 1u];
    if (i >= n || h >= n) return true;
    const float4 a = corners[i], b = corners[h];
    return unwrap_bits(a.x) != unwrap_bits(b.x) || unwrap_bits(a.y) != unwrap_bits(b.y) || unwrap_bits(a.z) != unwrap_bits(b.z);
}

__global__ __launch_bounds__(256) void pt_uw_vertex_count(PTUnwrapArgs A, const uint32_t* __restrict__ order)
{
    __shared__ uint32_t waveCount[4];
    uint32_t total;
    compact_rank_in_block(run_head(A.corners, order, A.triCount * 3u, blockIdx.x * 256u + threadIdx.x), waveCount, total);
    if (threadIdx.x == 0u) A.blockBase[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void pt_uw_scan(uint32_t* __restrict__ blockBase, uint32_t blocks, uint32_t* __restrict__ total)
{
    __shared__ uint32_t waveSum[16];
    const uint32_t all = compact_scan_blocks(blockBase, blocks, waveSum, [](uint32_t, uint32_t) {});
    if (threadIdx.x == 0u) *total = all;
}

__global__ __launch_bounds__(256) void pt_uw_vertex_ids(PTUnwrapArgs A, const uint32_t* __restrict__ order)
{
    __shared__ uint32_t waveCount[4];
    const uint32_t n = A.triCount * 3u, j = blockIdx.x * 256u + threadIdx.x;
    const bool head = run_head(A.corners, order, n, j);
    uint32_t total;
    const uint32_t before = A.blockBase[blockIdx.x] + compact_rank_in_block(head, waveCount, total);
    if (j >= n) return;
    const uint32_t i = order[j];
    // a head is vertex `before`; the others belong to the last head before them (place 0 is a head, so before >= 1 there)
    if (i < n) A.vid[i] = head ? before : before - 1u;
}

__global__ __launch_bounds__(256) void pt_uw_edge_keys(PTUnwrapArgs A, uint32_t idBits, uint32_t* __restrict__ edgeVal)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= A.triCount) return;
    const uint32_t cls = A.cls[p];
    const uint32_t i0 = A.vid[(size_t)p * 3u], i1 = A.vid[(size_t)p * 3u + 1u], i2 = A.vid[(size_t)p * 3u + 2u];
    const bool in = cls != kExcluded;
    A.edgeKey[(size_t)p * 3u] = in ? unwrap_edge_key(i0, i1, cls, idBits) : kNoEdge;
    A.edgeKey[(size_t)p * 3u + 1u] = in ? unwrap_edge_key(i1, i2, cls, idBits) : kNoEdge;
    A.edgeKey[(size_t)p * 3u + 2u] = in ? unwrap_edge_key(i2, i0, cls, idBits) : kNoEdge;
    edgeVal[(size_t)p * 3u] = p; edgeVal[(size_t)p * 3u + 1u] = p; edgeVal[(size_t)p * 3u + 2u] = p;
}

// the root of x: labels fall while other lanes hook, and every value a label ever holds is an ancestor of its primitive
__device__ __forceinline__ uint32_t root_of(uint32_t* label, uint32_t x, uint32_t T)
{
    for (uint32_t step = 0; step <= T; ++step) {                     // a chain is never longer than the BLAS
        const uint32_t n = __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n >= x) return x;                                       // n == x: the root (n > x cannot happen)
        x = n;
    }
    return x;
}

__global__ __launch_bounds__(256) void pt_uw_hook(PTUnwrapArgs A, const uint32_t* __restrict__ edgeVal, uint32_t sweep)
{
    const uint32_t n = A.triCount * 3u, j = blockIdx.x * 256u + threadIdx.x;
    bool linked = false, changed = false;
    if (j >= 1u && j < n) {
        const uint64_t k = A.edgeKeySorted[j];
        if (k != kNoEdge && k == A.edgeKeySorted[j - 1u]) {
            const uint32_t p = edgeVal[j], q = edgeVal[j - 1u];
            if (p < A.triCount && q < A.triCount) {
                linked = true;
                const uint32_t a = root_of(A.label, p, A.triCount), b = root_of(A.label, q, A.triCount);
                if (a != b) {
                    atomicMin(A.label + (a > b ? a : b), a > b ? b : a);
                    changed = true;
                }
            }
        }
    }
    const uint32_t links = wave_count(linked);
    const bool any = __ballot(changed) != 0ull;
    if (first_lane()) {
        if (sweep == 0u && links) atomicAdd(A.small + 1, links);
        if (any) A.small[8u + sweep] = 1u;
    }
}

__global__ __launch_bounds__(256) void pt_uw_compress(PTUnwrapArgs A)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= A.triCount) return;
    const uint32_t r = root_of(A.label, p, A.triCount);
    if (r < p) atomicMin(A.label + p, r);
}

__global__ __launch_bounds__(256) void pt_uw_count_tris(PTUnwrapArgs A)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const bool in = p < A.triCount && A.cls[p] != kExcluded;
    const uint32_t r = in ? A.label[p] : kNoChart;
    const bool counts = in && r < A.triCount;
    // neighbours in primitive order mostly share a chart: a wave whose counting lanes all have one label adds once
    const unsigned long long m = __ballot(counts);
    if (m == 0ull) return;
    const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)r, (int)__builtin_ctzll(m));
    if (__ballot(counts && r != lead) == 0ull) {
        if (counts && rank_below(m) == 0u) atomicAdd(A.triOfLabel + lead, (uint32_t)__popcll(m));
    } else if (counts) {
        atomicAdd(A.triOfLabel + r, 1u);
    }
}

__device__ __forceinline__ bool chart_head(const PTUnwrapArgs& A, uint32_t p) { return p < A.triCount && A.cls[p] != kExcluded && A.label[p] == p; }

__global__ __launch_bounds__(256) void pt_uw_head_count(PTUnwrapArgs A)
{
    __shared__ uint32_t waveCount[4];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const bool head = chart_head(A, p);
    uint32_t total;
    compact_rank_in_block(head, waveCount, total);
    if (threadIdx.x == 0u) A.blockBase[blockIdx.x] = total;
    const uint32_t singles = wave_count(head && A.triOfLabel[p] == 1u);
    if (singles && first_lane()) atomicAdd(A.small + 2, singles);
}

__global__ __launch_bounds__(256) void pt_uw_chart_init(PTUnwrapArgs A, uint4* __restrict__ charts, uint32_t chartCount)
{
    __shared__ uint32_t waveCount[4];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const bool head = chart_head(A, p);
    uint32_t total;
    const uint32_t k = A.blockBase[blockIdx.x] + compact_rank_in_block(head, waveCount, total);
    if (p < A.triCount) A.place[p] = head && k < chartCount ? k : kNoChart;
    if (!head || k >= chartCount) return;
    charts[(size_t)k * 2u] = make_uint4(p, A.cls[p], A.triOfLabel[p], 0u);
    charts[(size_t)k * 2u + 1u] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);          // order keys: umin vmin umax vmax
}

__global__ __launch_bounds__(256) void pt_uw_extents(PTUnwrapArgs A, uint32_t* __restrict__ chartOfPrim, uint32_t* __restrict__ charts, uint32_t chartCount)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= A.triCount) return;
    const uint32_t cls = A.cls[p], r = A.label[p];
    const uint32_t c = (cls != kExcluded && r < A.triCount) ? A.place[r] : kNoChart;
    chartOfPrim[p] = c < chartCount ? c : kNoChart;
    if (c >= chartCount) return;
    const uint32_t a = cls >> 1, ua = (a + 1u) % 3u, va = (a + 2u) % 3u;
    uint32_t umin = 0xFFFFFFFFu, vmin = 0xFFFFFFFFu, umax = 0u, vmax = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        const float4 q = A.corners[(size_t)p * 3u + k];
        const float v[3] = {q.x, q.y, q.z};
        const uint32_t ku = unwrap_order_key(unwrap_pick(v, ua)), kv = unwrap_order_key(unwrap_pick(v, va));
        umin = ku < umin ? ku : umin; umax = ku > umax ? ku : umax;
        vmin = kv < vmin ? kv : vmin; vmax = kv > vmax ? kv : vmax;
    }
    // A few hundred records take the extremes of every primitive: the atomic is left out where the word already holds a value
    // at least as extreme.  The words only move one way, so a value read a moment ago can only ask for an atomic too many.
    uint32_t* rec = charts + (size_t)c * 8u + 4u;
    if (umin < __hip_atomic_load(rec + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(rec + 0, umin);
    if (vmin < __hip_atomic_load(rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(rec + 1, vmin);
    if (umax > __hip_atomic_load(rec + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(rec + 2, umax);
    if (vmax > __hip_atomic_load(rec + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(rec + 3, vmax);
}

__global__ __launch_bounds__(256) void pt_uw_chart_finish(uint4* __restrict__ charts, uint32_t chartCount)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= chartCount) return;
    const uint4 e = charts[(size_t)k * 2u + 1u];
    charts[(size_t)k * 2u + 1u] = make_uint4(unwrap_bits(unwrap_order_value(e.x)), unwrap_bits(unwrap_order_value(e.y)), unwrap_bits(unwrap_order_value(e.z)),
                                             unwrap_bits(unwrap_order_value(e.w)));
}

__global__ __launch_bounds__(256) void pt_uw_emit(const float4* __restrict__ tris, const float4* __restrict__ vertices, uint32_t T,
                                                  const uint32_t* __restrict__ chartOfPrim, const float4* __restrict__ charts, const int2* __restrict__ origins,
                                                  uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float tpu, float2* __restrict__ uvs)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t p = 0u, cls;
    float c[3][3];
    if (!load_corners(tris, vertices, T, t, p, c, cls)) return;
    const uint32_t k = chartOfPrim[p];
    float uv[6];
    if (k < chartCount) {
        const float4 head = charts[(size_t)k * 2u], ext = charts[(size_t)k * 2u + 1u];
        const int2 o = origins[k];
        PTUnwrapChart ch;
        ch.firstPrim = unwrap_bits(head.x); ch.cls = unwrap_bits(head.y); ch.triCount = unwrap_bits(head.z); ch.reserved = 0u;
        ch.umin = ext.x; ch.vmin = ext.y; ch.umax = ext.z; ch.vmax = ext.w;
        unwrap_uvs(c, ch, o.x, o.y, width, height, padding, tpu, uv);
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) uv[i] = unwrap_float(kQuietNaN);
    }
    uvs[(size_t)p * 3u] = make_float2(uv[0], uv[1]);
    uvs[(size_t)p * 3u + 1u] = make_float2(uv[2], uv[3]);
    uvs[(size_t)p * 3u + 2u] = make_float2(uv[4], uv[5]);
}

inline uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }
inline size_t al256(size_t b) { return (b + 255u) & ~(size_t)255u; }

size_t sort_temp_bytes(uint32_t n)
{
    size_t a = 0, b = 0;
    if (rocprim::radix_sort_pairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32, nullptr) != hipSuccess) return 0;
    if (rocprim::radix_sort_pairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 64, nullptr) != hipSuccess) return 0;
    return (a > b ? a : b) + 256u;
}

} // namespace

size_t pt_unwrap_work_bytes(uint32_t T)
{
    const size_t n = (size_t)T * 3u, temp = sort_temp_bytes((uint32_t)n);
    if (!temp) return 0;
    return al256(n * 16u) + al256((size_t)T * 4u) + al256(n * 8u) + 2u * al256(n * 4u) + al256(n * 4u) + al256(n * 8u) + 3u * al256((size_t)T * 4u) +
           al256((size_t)blocks_of((uint32_t)n) * 4u + 4u) + al256(kUnwrapSmallWords * 4u) + al256(temp);
}

void pt_unwrap_carve(void* base, uint32_t T, PTUnwrapArgs& A)
{
    const size_t n = (size_t)T * 3u;
    char* p = (char*)base;
    auto take = [&](size_t bytes) { char* q = p; p += al256(bytes); return (void*)q; };
    A.triCount = T;
    A.corners = (float4*)take(n * 16u);
    A.cls = (uint32_t*)take((size_t)T * 4u);
    A.keyA = (uint32_t*)take(n * 8u); A.keyB = A.keyA + n;           // together: the 3 T edge keys
    A.valA = (uint32_t*)take(n * 4u); A.valB = (uint32_t*)take(n * 4u);
    A.vid = (uint32_t*)take(n * 4u);
    A.edgeKey = (uint64_t*)A.keyA;
    A.edgeKeySorted = (uint64_t*)take(n * 8u);
    A.label = (uint32_t*)take((size_t)T * 4u); A.triOfLabel = (uint32_t*)take((size_t)T * 4u); A.place = (uint32_t*)take((size_t)T * 4u);
    A.blockBase = (uint32_t*)take((size_t)blocks_of((uint32_t)n) * 4u + 4u);
    A.small = (uint32_t*)take(kUnwrapSmallWords * 4u);
    A.sortTempBytes = sort_temp_bytes((uint32_t)n);
    A.sortTemp = take(A.sortTempBytes);
}

hipError_t pt_launch_unwrap_edges(const PTUnwrapArgs& A, hipStream_t stream)
{
    const uint32_t T = A.triCount, n = T * 3u;
    hipError_t e;
    if ((e = hipMemsetAsync(A.small, 0, kUnwrapSmallWords * 4u, stream)) != hipSuccess) return e;
    // a primitive no record names stays excluded; its corners are zeros
    if ((e = hipMemsetAsync(A.cls, 0xFF, (size_t)T * 4u, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(A.corners, 0, (size_t)n * 16u, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(A.keyA, 0, (size_t)n * 4u, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt_uw_corners, dim3(blocks_of(T)), dim3(256), 0, stream, A);
    size_t temp = A.sortTempBytes;
    // z: keyA / valA -> keyB / valB;  y: gathered into keyA by valB -> keyB / valA;  x: gathered by valA -> keyB / valB
    if ((e = rocprim::radix_sort_pairs(A.sortTemp, temp, A.keyA, A.keyB, A.valA, A.valB, n, 0, 32, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt_uw_gather_key, dim3(blocks_of(n)), dim3(256), 0, stream, A.corners, A.valB, n, 1u, A.keyA);
    if ((e = rocprim::radix_sort_pairs(A.sortTemp, temp, A.keyA, A.keyB, A.valB, A.valA, n, 0, 32, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt_uw_gather_key, dim3(blocks_of(n)), dim3(256), 0, stream, A.corners, A.valA, n, 0u, A.keyA);
    if ((e = rocprim::radix_sort_pairs(A.sortTemp, temp, A.keyA, A.keyB, A.valA, A.valB, n, 0, 32, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt_uw_vertex_count, dim3(blocks_of(n)), dim3(256), 0, stream, A, A.valB);
    hipLaunchKernelGGL(pt_uw_scan, dim3(1), dim3(1024), 0, stream, A.blockBase, blocks_of(n), A.small + 3);
    hipLaunchKernelGGL(pt_uw_vertex_ids, dim3(blocks_of(n)), dim3(256), 0, stream, A, A.valB);
    // the edge keys take the place of the vertex sort's keys, their values that of its values
    hipLaunchKernelGGL(pt_uw_edge_keys, dim3(blocks_of(T)), dim3(256), 0, stream, A, unwrap_id_bits(n), A.valA);
    if ((e = rocprim::radix_sort_pairs(A.sortTemp, temp, A.edgeKey, A.edgeKeySorted, A.valA, A.valB, n, 0, 64, stream)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t pt_launch_unwrap_sweep(const PTUnwrapArgs& A, uint32_t s, hipStream_t stream)
{
    if (s >= PT_UNWRAP_MAX_SWEEPS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_uw_hook, dim3(blocks_of(A.triCount * 3u)), dim3(256), 0, stream, A, A.valB, s);
    hipLaunchKernelGGL(pt_uw_compress, dim3(blocks_of(A.triCount)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

hipError_t pt_launch_unwrap_count(const PTUnwrapArgs& A, hipStream_t stream)
{
    const uint32_t blocks = blocks_of(A.triCount);
    hipLaunchKernelGGL(pt_uw_count_tris, dim3(blocks), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(pt_uw_head_count, dim3(blocks), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(pt_uw_scan, dim3(1), dim3(1024), 0, stream, A.blockBase, blocks, A.small + 4);
    return hipGetLastError();
}

hipError_t pt_launch_unwrap_charts(const PTUnwrapArgs& A, uint32_t* chartOfPrim, PTUnwrapChart* charts, uint32_t chartCount, hipStream_t stream)
{
    const uint32_t blocks = blocks_of(A.triCount);
    hipLaunchKernelGGL(pt_uw_chart_init, dim3(blocks), dim3(256), 0, stream, A, (uint4*)charts, chartCount);
    hipLaunchKernelGGL(pt_uw_extents, dim3(blocks), dim3(256), 0, stream, A, chartOfPrim, (uint32_t*)charts, chartCount);
    if (chartCount) hipLaunchKernelGGL(pt_uw_chart_finish, dim3(blocks_of(chartCount)), dim3(256), 0, stream, (uint4*)charts, chartCount);
    return hipGetLastError();
}

hipError_t pt_launch_unwrap_emit(const float4* tris, const float4* vertices, uint32_t T, const uint32_t* chartOfPrim, const PTUnwrapChart* charts,
                                 const int32_t* origins, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float tpu, float* uvs,
                                 hipStream_t stream)
{
    hipLaunchKernelGGL(pt_uw_emit, dim3(blocks_of(T)), dim3(256), 0, stream, tris, vertices, T, chartOfPrim, (const float4*)charts, (const int2*)origins,
                       chartCount, width, height, padding, tpu, (float2*)uvs);
    return hipGetLastError();
}
