// pt_tlas.hip — the TLAS of PTUpdateInstances built on the GPU, byte-identical to BuildTLAS (bvh_builder.cpp Tlas::build).
//
// Three launches, in stream order, no host readback:
//   1. pt_tlas_prep   (many workgroups): instance AABBs -> box[], idx[i] = i.
//   2. pt_tlas_build  (ONE workgroup of 512 threads): root bounds, then the tree level by level.  A node of
//      kTlasCoopMin instances or more is binned and partitioned by the whole workgroup, one such node at a time;
//      smaller nodes are built one per thread, exactly as the host code does it.  Nodes are numbered breadth-first
//      (children of the level's splitting nodes in level order, left first), then subtree sizes bottom-up and preorder
//      positions top-down give the depth-first numbering Tlas::build lays out.
//   3. pt_tlas_emit   (many workgroups): both node layouts, the index list, instByLeaf, the instance matrices.
//
// What makes the bytes equal to the host build's:
//   - lo / hi are compare-and-select (a < b ? a : b), never v_min / v_max; the Makefile compiles without FMA contraction.
//   - A cooperative bin is reduced in element order: every thread folds a contiguous slice, the wave combines neighbouring
//     slices in order, the waves' partials are folded in order.  For non-NaN input, compare-and-select keeps the last
//     element of the minimum under `<`, which does not depend on how the sequence is bracketed (+0 / -0 included).
//   - float -> int is x86 cvttss2si: NaN or out of range gives INT32_MIN (and 0 for the low word of the 64-bit form).
//   - The cooperative partition places elements where the host's swap loop does (the placement rule is in DESIGN.md 5.10).
//   - The task-stack cut-off: a node with 256 left edges above it does not split (nlt).
// Everything stays in bounds for any input: node ids are < 2n by construction (every split has two non-empty sides),
// partition positions are clamped to the node's range, and there is no private array (no scratch).
#include "pt_tlas.h"

#include <climits>

namespace {

constexpr float kFar = 1e30f;
constexpr uint32_t kThreads = 512u;
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kTlasCoopMin = 1024u;      // nodes at least this large are built by the whole workgroup
constexpr uint32_t kLeafBit = 0xFFFFFFFFu;
constexpr uint32_t kLdsInstances = 4096u;   // up to this many, the boxes and the index list live in LDS during the build (144 KB)

struct F3 { float x, y, z; };
__device__ inline F3 f3(float a) { return {a, a, a}; }
__device__ inline float lo(float a, float b) { return a < b ? a : b; }
__device__ inline float hi(float a, float b) { return a > b ? a : b; }
__device__ inline F3 lo3(F3 a, F3 b) { return {lo(a.x, b.x), lo(a.y, b.y), lo(a.z, b.z)}; }
__device__ inline F3 hi3(F3 a, F3 b) { return {hi(a.x, b.x), hi(a.y, b.y), hi(a.z, b.z)}; }
__device__ inline F3 sub(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline float comp(F3 v, uint32_t a) { return a == 0u ? v.x : (a == 1u ? v.y : v.z); }
__device__ inline float half_area(F3 v) { return v.x < -kFar ? 0.0f : (v.x * v.y + v.y * v.z + v.z * v.x); }
__device__ inline F3 xyz(float4 v) { return {v.x, v.y, v.z}; }
__device__ inline float4 f4(F3 v, float w) { return make_float4(v.x, v.y, v.z, w); }
// x86 cvttss2si, 32- and 64-bit forms (the host build's conversions)
__device__ inline int32_t trunc_i32(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : INT_MIN; }
__device__ inline uint32_t trunc_u32(float f)
{
    return (f >= -9223372036854775808.0f && f < 9223372036854775808.0f) ? (uint32_t)(uint64_t)(int64_t)f : 0u;
}
__device__ inline int32_t clampi(int32_t x, int32_t a, int32_t b) { return x > a ? (x < b ? x : b) : a; }

// the 8 bins of one axis: min xyz, max xyz, count
struct Bins {
    F3 mn[8], mx[8];
    uint32_t cnt[8];
};

__device__ inline void bins_clear(Bins& B)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) { B.mn[k] = f3(kFar); B.mx[k] = f3(-kFar); B.cnt[k] = 0u; }
}

__device__ inline void bins_add(Bins& B, int32_t b, F3 bmin, F3 bmax)
{
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (b == k) { B.mn[k] = lo3(B.mn[k], bmin); B.mx[k] = hi3(B.mx[k], bmax); B.cnt[k]++; }
}

struct Node { F3 mn, mx; uint32_t first, count, lt; };

__device__ inline Node load_node(const PTTlasWork& W, uint32_t p)
{
    const float4 a = W.nb0[p], b = W.nb1[p];
    return {xyz(a), xyz(b), __float_as_uint(a.w), __float_as_uint(b.w), W.nlt[p]};
}

struct Best {
    float cost;
    uint32_t axis, pos;
    F3 lmin, lmax, rmin, rmax;
};

// the SAH sweep of one axis (bvh_builder.cpp Bvh2::build), updating the running best over the axes in order 0, 1, 2
__device__ inline void sah_axis(const Bins& B, uint32_t a, Best& best)
{
    float ANR[7];
    {
        F3 r1 = f3(kFar), r2 = f3(-kFar);
        uint32_t rN = 0u;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            r1 = lo3(r1, B.mn[7 - i]);
            r2 = hi3(r2, B.mx[7 - i]);
            rN += B.cnt[7 - i];
            ANR[6 - i] = rN == 0u ? kFar : (half_area(sub(r2, r1)) * (float)rN);
        }
    }
    F3 l1 = f3(kFar), l2 = f3(-kFar);
    uint32_t lN = 0u;
    int32_t found = -1;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        l1 = lo3(l1, B.mn[i]);
        l2 = hi3(l2, B.mx[i]);
        lN += B.cnt[i];
        const float ANL = lN == 0u ? kFar : (half_area(sub(l2, l1)) * (float)lN);
        const float C = ANL + ANR[i];
        if (C < best.cost) { best.cost = C; best.axis = a; best.pos = (uint32_t)i; best.lmin = l1; best.lmax = l2; found = i; }
    }
    if (found >= 0) {           // the right-hand bounds of the chosen plane, folded in the host's order
        F3 r1 = f3(kFar), r2 = f3(-kFar);
#pragma unroll
        for (int i = 0; i < 7; ++i)
            if (6 - i >= found) { r1 = lo3(r1, B.mn[7 - i]); r2 = hi3(r2, B.mx[7 - i]); }
        best.rmin = r1; best.rmax = r2;
    }
}

// boxes and the index list are addressed through generic pointers: LDS copies for up to kLdsInstances, else global memory
__device__ inline F3 box_min(const float4* box, uint32_t prim) { return xyz(box[2u * prim]); }
__device__ inline F3 box_max(const float4* box, uint32_t prim) { return xyz(box[2u * prim + 1u]); }

__device__ inline int32_t bin_of(F3 bmin, F3 bmax, uint32_t a, float nmin, float rpd)
{
    return clampi(trunc_i32(((comp(bmin, a) + comp(bmax, a)) * 0.5f - nmin) * rpd), 0, 7);
}
__device__ inline bool goes_right(F3 bmin, F3 bmax, uint32_t a, float nmin, float rpd, uint32_t pos)
{
    int32_t bi = (int32_t)trunc_u32(((comp(bmin, a) + comp(bmax, a)) * 0.5f - nmin) * rpd);
    bi = clampi(bi, 0, 7);
    return (uint32_t)bi > pos;
}

__device__ inline bool axis_ok(const Node& N, uint32_t a, F3 minDim) { return (comp(N.mx, a) - comp(N.mn, a)) > comp(minDim, a); }

__device__ inline void store_split(const PTTlasWork& W, uint32_t p, bool split, const Best& b, uint32_t leftCount)
{
    W.nsplit[p] = split ? 1u : 0u;
    if (!split) return;
    W.nleft[p] = leftCount;
    W.sp[4u * p + 0u] = f4(b.lmin, 0.0f);
    W.sp[4u * p + 1u] = f4(b.lmax, 0.0f);
    W.sp[4u * p + 2u] = f4(b.rmin, 0.0f);
    W.sp[4u * p + 3u] = f4(b.rmax, 0.0f);
}

// One node by one thread: Bvh2::build's loop body, partition included.
__device__ void build_node_serial(const PTTlasWork& W, uint32_t p, F3 minDim, const float4* box, uint32_t* idx)
{
    const Node N = load_node(W, p);
    const F3 ext = sub(N.mx, N.mn);
    const F3 rpd3 = {8.0f / ext.x, 8.0f / ext.y, 8.0f / ext.z};
    const float rSAV = 1.0f / (ext.x * ext.y + ext.y * ext.z + ext.z * ext.x);
    Best best = {kFar, 0u, 0u, f3(0.0f), f3(0.0f), f3(0.0f), f3(0.0f)};
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!axis_ok(N, a, minDim)) continue;
        Bins B;
        bins_clear(B);
        const float nmin = comp(N.mn, a), rpd = comp(rpd3, a);
#pragma unroll 4
        for (uint32_t i = 0; i < N.count; ++i) {
            const uint32_t prim = idx[N.first + i];
            const F3 bmin = box_min(box, prim), bmax = box_max(box, prim);
            bins_add(B, bin_of(bmin, bmax, a, nmin, rpd), bmin, bmax);
        }
        sah_axis(B, a, best);
    }
    const float splitCost = 1.0f + 1.0f * rSAV * best.cost;
    if (splitCost >= (float)N.count * 1.0f) { store_split(W, p, false, best, 0u); return; }
    uint32_t j = N.first + N.count, src = N.first;
    const float rpd = comp(rpd3, best.axis), nmin = comp(N.mn, best.axis);
    for (uint32_t i = 0; i < N.count; ++i) {
        const uint32_t prim = idx[src];
        if (!goes_right(box_min(box, prim), box_max(box, prim), best.axis, nmin, rpd, best.pos)) src++;
        else { --j; const uint32_t t = idx[j]; idx[j] = prim; idx[src] = t; }
    }
    const uint32_t leftCount = src - N.first;
    store_split(W, p, !(leftCount == 0u || leftCount == N.count || N.lt == 256u), best, leftCount);
}

// in-order combine of neighbouring slices across the wave (butterfly; the lower lane's value goes first)
__device__ inline float wave_lo(float v)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const float o = __shfl_xor(v, (int)d, 64);
        v = (lane & d) ? lo(o, v) : lo(v, o);
    }
    return v;
}
__device__ inline float wave_hi(float v)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const float o = __shfl_xor(v, (int)d, 64);
        v = (lane & d) ? hi(o, v) : hi(v, o);
    }
    return v;
}
__device__ inline uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) v += (uint32_t)__shfl_xor((int)v, (int)d, 64);
    return v;
}

// exclusive prefix of a 0/1 flag over the workgroup, in thread order; *total = sum.  Contains two barriers.
__device__ inline uint32_t block_scan(uint32_t flag, uint32_t* s_wsum, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t bal = __ballot(flag != 0u);
    const uint32_t pre = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0u) s_wsum[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t off = 0u, tot = 0u;
    for (uint32_t w = 0; w < kWaves; ++w) { const uint32_t s = s_wsum[w]; if (w < wave) off += s; tot += s; }
    __syncthreads();
    *total = tot;
    return off + pre;
}

struct Shared {
    float part[kWaves][56];     // per-wave partial bins of one axis (min xyz x 8, max xyz x 8, count x 8)
    float bins[56];
    uint32_t wsum[kWaves];
    uint32_t nbig, totR, split, pad;
    float dec[16];              // the cooperative node's decision, written by thread 0
};

// One node by the whole workgroup: binning in slices, thread 0 sweeps the SAH, the partition by placement rule.
__device__ void build_node_coop(const PTTlasWork& W, uint32_t p, F3 minDim, Shared& sh, const float4* box, uint32_t* idx)
{
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const Node N = load_node(W, p);
    const F3 ext = sub(N.mx, N.mn);
    const F3 rpd3 = {8.0f / ext.x, 8.0f / ext.y, 8.0f / ext.z};
    const float rSAV = 1.0f / (ext.x * ext.y + ext.y * ext.z + ext.z * ext.x);
    const uint32_t m = N.count, chunk = (m + kThreads - 1u) / kThreads;
    const uint32_t i0 = t * chunk < m ? t * chunk : m, i1 = i0 + chunk < m ? i0 + chunk : m;
    Best best = {kFar, 0u, 0u, f3(0.0f), f3(0.0f), f3(0.0f), f3(0.0f)};
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!axis_ok(N, a, minDim)) continue;
        Bins B;
        bins_clear(B);
        const float nmin = comp(N.mn, a), rpd = comp(rpd3, a);
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t prim = idx[N.first + i];
            const F3 bmin = box_min(box, prim), bmax = box_max(box, prim);
            bins_add(B, bin_of(bmin, bmax, a, nmin, rpd), bmin, bmax);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v0 = wave_lo(B.mn[k].x), v1 = wave_lo(B.mn[k].y), v2 = wave_lo(B.mn[k].z);
            const float v3 = wave_hi(B.mx[k].x), v4 = wave_hi(B.mx[k].y), v5 = wave_hi(B.mx[k].z);
            const uint32_t c = wave_sum(B.cnt[k]);
            if (lane == 0u) {
                sh.part[wave][k * 3 + 0] = v0; sh.part[wave][k * 3 + 1] = v1; sh.part[wave][k * 3 + 2] = v2;
                sh.part[wave][24 + k * 3 + 0] = v3; sh.part[wave][24 + k * 3 + 1] = v4; sh.part[wave][24 + k * 3 + 2] = v5;
                sh.part[wave][48 + k] = __uint_as_float(c);
            }
        }
        __syncthreads();
        if (t < 56u) {
            float v = t < 24u ? kFar : -kFar;
            uint32_t c = 0u;
            for (uint32_t w = 0; w < kWaves; ++w) {
                const float o = sh.part[w][t];
                if (t < 24u) v = lo(v, o);
                else if (t < 48u) v = hi(v, o);
                else c += __float_as_uint(o);
            }
            sh.bins[t] = t < 48u ? v : __uint_as_float(c);
        }
        __syncthreads();
        if (t == 0u) {
            Bins S;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                S.mn[k] = {sh.bins[k * 3], sh.bins[k * 3 + 1], sh.bins[k * 3 + 2]};
                S.mx[k] = {sh.bins[24 + k * 3], sh.bins[24 + k * 3 + 1], sh.bins[24 + k * 3 + 2]};
                S.cnt[k] = __float_as_uint(sh.bins[48 + k]);
            }
            sah_axis(S, a, best);
        }
    }
    if (t == 0u) {
        const float splitCost = 1.0f + 1.0f * rSAV * best.cost;
        sh.split = splitCost >= (float)m * 1.0f ? 0u : 1u;
        sh.dec[0] = __uint_as_float(best.axis); sh.dec[1] = __uint_as_float(best.pos);
        sh.dec[2] = best.lmin.x; sh.dec[3] = best.lmin.y; sh.dec[4] = best.lmin.z;
        sh.dec[5] = best.lmax.x; sh.dec[6] = best.lmax.y; sh.dec[7] = best.lmax.z;
        sh.dec[8] = best.rmin.x; sh.dec[9] = best.rmin.y; sh.dec[10] = best.rmin.z;
        sh.dec[11] = best.rmax.x; sh.dec[12] = best.rmax.y; sh.dec[13] = best.rmax.z;
    }
    __syncthreads();
    if (!sh.split) {
        if (t == 0u) store_split(W, p, false, best, 0u);
        __syncthreads();
        return;
    }
    const uint32_t axis = __float_as_uint(sh.dec[0]), pos = __float_as_uint(sh.dec[1]);
    const float rpd = comp(rpd3, axis), nmin = comp(N.mn, axis);
    // pass A: right flags and the count of right elements before each position
    uint32_t totR = 0u;
    for (uint32_t base = 0; base < m; base += kThreads) {
        const uint32_t i = base + t;
        uint32_t f = 0u;
        if (i < m) { const uint32_t prim = idx[N.first + i]; f = goes_right(box_min(box, prim), box_max(box, prim), axis, nmin, rpd, pos) ? 1u : 0u; }
        uint32_t tot;
        const uint32_t ex = block_scan(f, sh.wsum, &tot);
        if (i < m) W.tmpR[i] = (totR + ex) | (f << 31);
        totR += tot;
    }
    __syncthreads();
    // The host's loop consumes a front scan (ascending, up to and including the next right element) and a back scan
    // (descending, up to and including the next left element) in turn; they meet at s = L, or L + 1 when position L holds a
    // right element (L = number of left elements).  Front lefts stay; the k-th front right goes to Lb[k - 1] - 1 (m - 1 for
    // the first); the k-th back left (from the top) goes to Rf[k]; back rights move down by one.
    const uint32_t L = m - totR;
    const uint32_t s = (L == m || !(W.tmpR[L] >> 31)) ? L : L + 1u;
    for (uint32_t i = t; i < m; i += kThreads) {
        const uint32_t v = W.tmpR[i], f = v >> 31, R = v & 0x7FFFFFFFu;
        if (i < s && f) W.rf[R < m ? R : m - 1u] = i;
        if (i >= s && !f) { const uint32_t k = (m - 1u - i) - (totR - R - f); W.lb[k < m ? k : m - 1u] = i; }
    }
    __syncthreads();
    for (uint32_t i = t; i < m; i += kThreads) {
        const uint32_t v = W.tmpR[i], f = v >> 31, R = v & 0x7FFFFFFFu;
        uint32_t out;
        if (i < s) out = !f ? i : (R == 0u ? m - 1u : W.lb[R - 1u < m ? R - 1u : m - 1u] - 1u);
        else if (f) out = i - 1u;
        else { const uint32_t k = (m - 1u - i) - (totR - R - f); out = W.rf[k < m ? k : m - 1u]; }
        W.tmpIdx[N.first + (out < m ? out : m - 1u)] = idx[N.first + i];
    }
    __syncthreads();
    for (uint32_t i = t; i < m; i += kThreads) idx[N.first + i] = W.tmpIdx[N.first + i];
    if (t == 0u) {
        const Best b = {0.0f, axis, pos, {sh.dec[2], sh.dec[3], sh.dec[4]}, {sh.dec[5], sh.dec[6], sh.dec[7]},
                        {sh.dec[8], sh.dec[9], sh.dec[10]}, {sh.dec[11], sh.dec[12], sh.dec[13]}};
        store_split(W, p, !(L == 0u || L == m || N.lt == 256u), b, L);
    }
    __syncthreads();
}

__global__ void pt_tlas_prep(PTTlasWork W, const PTBlasInstance* __restrict__ in)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < W.n; i += gridDim.x * blockDim.x) {
        const PTBlasInstance& r = in[i];
        W.box[2u * i] = make_float4(r.aabbMin[0], r.aabbMin[1], r.aabbMin[2], 0.0f);
        W.box[2u * i + 1u] = make_float4(r.aabbMax[0], r.aabbMax[1], r.aabbMax[2], 0.0f);
        W.idx[i] = i;
    }
}

__global__ __launch_bounds__(512) void pt_tlas_build(PTTlasWork W)
{
    __shared__ Shared sh;
    __shared__ float4 s_box[2u * kLdsInstances];
    __shared__ uint32_t s_idx[kLdsInstances];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, n = W.n;
    const bool inLds = n <= kLdsInstances;
    const float4* box = inLds ? (const float4*)s_box : W.box;
    uint32_t* idx = inLds ? s_idx : W.idx;
    if (inLds) {
        for (uint32_t i = t; i < 2u * n; i += kThreads) s_box[i] = W.box[i];
        for (uint32_t i = t; i < n; i += kThreads) s_idx[i] = W.idx[i];
        __syncthreads();
    }
    // root bounds: the host folds all boxes in order (Bvh2::prepareBoxes)
    {
        const uint32_t chunk = (n + kThreads - 1u) / kThreads;
        const uint32_t i0 = t * chunk < n ? t * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
        F3 mn = f3(kFar), mx = f3(-kFar);
        for (uint32_t i = i0; i < i1; ++i) { mn = lo3(mn, box_min(box, i)); mx = hi3(mx, box_max(box, i)); }
        const float v0 = wave_lo(mn.x), v1 = wave_lo(mn.y), v2 = wave_lo(mn.z);
        const float v3 = wave_hi(mx.x), v4 = wave_hi(mx.y), v5 = wave_hi(mx.z);
        if (lane == 0u) { sh.part[wave][0] = v0; sh.part[wave][1] = v1; sh.part[wave][2] = v2; sh.part[wave][3] = v3; sh.part[wave][4] = v4; sh.part[wave][5] = v5; }
        __syncthreads();
        if (t < 6u) {
            float v = t < 3u ? kFar : -kFar;
            for (uint32_t w = 0; w < kWaves; ++w) v = t < 3u ? lo(v, sh.part[w][t]) : hi(v, sh.part[w][t]);
            sh.bins[t] = v;
        }
        __syncthreads();
    }
    const F3 rmin = {sh.bins[0], sh.bins[1], sh.bins[2]}, rmax = {sh.bins[3], sh.bins[4], sh.bins[5]};
    const F3 rootExt = sub(rmax, rmin);
    const F3 minDim = {rootExt.x * 1e-20f, rootExt.y * 1e-20f, rootExt.z * 1e-20f};
    if (t == 0u) {
        W.nb0[0] = f4(rmin, __uint_as_float(0u));
        W.nb1[0] = f4(rmax, __uint_as_float(n));
        W.nlt[0] = 0u;
    }
    __syncthreads();
    uint32_t levelStart = 0u, levelCount = 1u, nLevels = 0u;
    while (levelCount > 0u) {
        if (t == 0u) { W.levels[nLevels] = levelStart; sh.nbig = 0u; }
        nLevels++;
        __syncthreads();
        for (uint32_t q = t; q < levelCount; q += kThreads) {
            const uint32_t p = levelStart + q;
            if (__float_as_uint(W.nb1[p].w) >= kTlasCoopMin) W.big[atomicAdd(&sh.nbig, 1u)] = p;
        }
        __syncthreads();
        const uint32_t nbig = sh.nbig;
        for (uint32_t b = 0; b < nbig; ++b) build_node_coop(W, W.big[b], minDim, sh, box, idx);
        for (uint32_t q = t; q < levelCount; q += kThreads) {
            const uint32_t p = levelStart + q;
            if (__float_as_uint(W.nb1[p].w) < kTlasCoopMin) build_node_serial(W, p, minDim, box, idx);
        }
        __syncthreads();
        // children of the splitting nodes, in level order, left first: breadth-first ids
        const uint32_t next = levelStart + levelCount;
        uint32_t splits = 0u;
        for (uint32_t base = 0; base < levelCount; base += kThreads) {
            const uint32_t q = base + t, p = levelStart + q;
            uint32_t f = q < levelCount ? W.nsplit[p] : 0u;
            uint32_t tot;
            const uint32_t ex = block_scan(f, sh.wsum, &tot);
            if (q < levelCount) {
                const uint32_t c = next + 2u * (splits + ex);
                if (f && c + 1u < 2u * n) {
                    const Node N = load_node(W, p);
                    const uint32_t L = W.nleft[p];
                    W.nb0[c] = make_float4(W.sp[4u * p].x, W.sp[4u * p].y, W.sp[4u * p].z, __uint_as_float(N.first));
                    W.nb1[c] = make_float4(W.sp[4u * p + 1u].x, W.sp[4u * p + 1u].y, W.sp[4u * p + 1u].z, __uint_as_float(L));
                    W.nlt[c] = N.lt + 1u;
                    W.nb0[c + 1u] = make_float4(W.sp[4u * p + 2u].x, W.sp[4u * p + 2u].y, W.sp[4u * p + 2u].z, __uint_as_float(N.first + L));
                    W.nb1[c + 1u] = make_float4(W.sp[4u * p + 3u].x, W.sp[4u * p + 3u].y, W.sp[4u * p + 3u].z, __uint_as_float(N.count - L));
                    W.nlt[c + 1u] = N.lt;
                    W.nchild[p] = c;
                } else {
                    W.nchild[p] = kLeafBit;
                }
            }
            splits += tot;
        }
        __syncthreads();
        levelStart = next;
        levelCount = 2u * splits;
        if (levelStart + levelCount > 2u * n) levelCount = 0u;          // cannot happen: every split has two non-empty sides
    }
    const uint32_t total = levelStart;
    if (t == 0u) { W.levels[nLevels] = total; W.ctrl[0] = total; }
    if (inLds)
        for (uint32_t i = t; i < n; i += kThreads) W.idx[i] = s_idx[i];
    __syncthreads();
    // subtree sizes bottom-up, preorder positions top-down (Tlas::build numbers nodes depth-first, left child first)
    for (uint32_t l = nLevels; l-- > 0u;) {
        const uint32_t a = W.levels[l], b = W.levels[l + 1u];
        for (uint32_t p = a + t; p < b; p += kThreads) {
            const uint32_t c = W.nchild[p];
            W.nsize[p] = c == kLeafBit ? 1u : 1u + W.nsize[c] + W.nsize[c + 1u];
        }
        __syncthreads();
    }
    if (t == 0u) W.npre[0] = 0u;
    __syncthreads();
    for (uint32_t l = 0; l < nLevels; ++l) {
        const uint32_t a = W.levels[l], b = W.levels[l + 1u];
        for (uint32_t p = a + t; p < b; p += kThreads) {
            const uint32_t c = W.nchild[p];
            if (c == kLeafBit) continue;
            const uint32_t pre = W.npre[p];
            W.npre[c] = pre + 1u;
            W.npre[c + 1u] = pre + 1u + W.nsize[c];
        }
        __syncthreads();
    }
}

__global__ void pt_tlas_emit(PTTlasWork W, const PTBlasInstance* __restrict__ in, float4* __restrict__ raw, float4* __restrict__ bfs,
                             float4* __restrict__ byLeaf, float4* __restrict__ inst)
{
    const uint32_t n = W.n, slots = 2u * n - 1u, total = W.ctrl[0] < slots ? W.ctrl[0] : slots;
    uint32_t* rawIdx = (uint32_t*)(raw + 4u * (size_t)slots);
    const uint32_t end = slots > n ? slots : n;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < end; q += gridDim.x * blockDim.x) {
        if (q < slots) {
            if (q < total) {
                const uint32_t c = W.nchild[q];
                float4 r[4];
                if (c == kLeafBit) {
                    const float4 b0 = W.nb0[q], b1 = W.nb1[q];
                    r[0] = r[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    r[2] = make_float4(0.0f, 0.0f, 0.0f, b1.w);         // triCount
                    r[3] = make_float4(0.0f, 0.0f, 0.0f, b0.w);         // firstTri
                    raw[4u * (size_t)W.npre[q] + 0u] = r[0]; raw[4u * (size_t)W.npre[q] + 1u] = r[1];
                    raw[4u * (size_t)W.npre[q] + 2u] = r[2]; raw[4u * (size_t)W.npre[q] + 3u] = r[3];
                    for (int k = 0; k < 4; ++k) bfs[4u * (size_t)q + k] = r[k];
                } else {
                    const float4 l0 = W.nb0[c], l1 = W.nb1[c], q0 = W.nb0[c + 1u], q1 = W.nb1[c + 1u];
                    const size_t d = 4u * (size_t)W.npre[q];
                    raw[d + 0u] = make_float4(l0.x, l0.y, l0.z, __uint_as_float(W.npre[c]));
                    raw[d + 1u] = make_float4(l1.x, l1.y, l1.z, __uint_as_float(W.npre[c + 1u]));
                    raw[d + 2u] = make_float4(q0.x, q0.y, q0.z, 0.0f);
                    raw[d + 3u] = make_float4(q1.x, q1.y, q1.z, 0.0f);
                    bfs[4u * (size_t)q + 0u] = make_float4(l0.x, l0.y, l0.z, __uint_as_float(c));
                    bfs[4u * (size_t)q + 1u] = make_float4(l1.x, l1.y, l1.z, __uint_as_float(c + 1u));
                    bfs[4u * (size_t)q + 2u] = make_float4(q0.x, q0.y, q0.z, 0.0f);
                    bfs[4u * (size_t)q + 3u] = make_float4(q1.x, q1.y, q1.z, 0.0f);
                }
            } else {            // unreachable padding (raw positions and breadth-first ids both run 0 .. total - 1)
                for (int k = 0; k < 4; ++k) { raw[4u * (size_t)q + k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); bfs[4u * (size_t)q + k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
            }
        }
        if (q < n) {
            uint32_t k = W.idx[q];
            rawIdx[q] = k;
            k = k < n ? k : 0u;
            const float4* w2l = (const float4*)in[k].worldToLocal;
            float4* e = byLeaf + 6u * (size_t)q;
            e[0] = w2l[0]; e[1] = w2l[1]; e[2] = w2l[2]; e[3] = w2l[3];
            e[4] = inst[9u * (size_t)k + 8u];                          // bvhOffset, triOffset, triAttributeOffset, materialIndex
            e[5] = make_float4(__uint_as_float(k), 0.0f, 0.0f, 0.0f);
            const float4* src = (const float4*)in[q].localToWorld;     // localToWorld and worldToLocal: 8 float4, the offsets row stays
            for (int r = 0; r < 8; ++r) inst[9u * (size_t)q + r] = src[r];
        }
    }
}

} // namespace

size_t pt_tlas_work_bytes(uint32_t n)
{
    const size_t N = n, a = 256;
    auto al = [&](size_t b) { return (b + a - 1) / a * a; };
    return al(N * 32) + al(N * 4) * 6 + al(N * 32) * 2 + al(N * 8) * 8 + al(N * 128) + al(N * 8 + 4) + al(16) + al(N * 192);
}

PTTlasWork pt_tlas_carve(void* base, uint32_t n)
{
    const size_t N = n;
    char* p = (char*)base;
    auto carve = [&](size_t b) { char* q = p; p += (b + 255) / 256 * 256; return (void*)q; };
    PTTlasWork W;
    W.n = n;
    W.box = (float4*)carve(N * 32);
    W.idx = (uint32_t*)carve(N * 4);
    W.tmpIdx = (uint32_t*)carve(N * 4);
    W.tmpR = (uint32_t*)carve(N * 4);
    W.rf = (uint32_t*)carve(N * 4);
    W.lb = (uint32_t*)carve(N * 4);
    W.big = (uint32_t*)carve(N * 4);
    W.nb0 = (float4*)carve(N * 32);
    W.nb1 = (float4*)carve(N * 32);
    W.nlt = (uint32_t*)carve(N * 8);
    W.nchild = (uint32_t*)carve(N * 8);
    W.nsplit = (uint32_t*)carve(N * 8);
    W.nleft = (uint32_t*)carve(N * 8);
    W.nsize = (uint32_t*)carve(N * 8);
    W.npre = (uint32_t*)carve(N * 8);
    carve(N * 8);
    carve(N * 8);
    W.sp = (float4*)carve(N * 128);
    W.levels = (uint32_t*)carve(N * 8 + 4);
    W.ctrl = (uint32_t*)carve(16);
    W.input = (PTBlasInstance*)carve(N * 192);
    return W;
}

hipError_t pt_launch_tlas_update(const PTTlasWork& W, const PTBlasInstance* in, float* rawTlas, float* bfs, float* instByLeaf,
                                 float* instances, hipStream_t stream)
{
    const uint32_t n = W.n;
    const uint32_t items = 2u * n - 1u > n ? 2u * n - 1u : n;
    uint32_t blocks = (items + 255u) / 256u;
    if (blocks > 1024u) blocks = 1024u;
    hipLaunchKernelGGL(pt_tlas_prep, dim3(blocks), dim3(256), 0, stream, W, in);
    hipLaunchKernelGGL(pt_tlas_build, dim3(1), dim3(kThreads), 0, stream, W);
    hipLaunchKernelGGL(pt_tlas_emit, dim3(blocks), dim3(256), 0, stream, W, in, (float4*)rawTlas, (float4*)bfs, (float4*)instByLeaf,
                       (float4*)instances);
    return hipGetLastError();
}
