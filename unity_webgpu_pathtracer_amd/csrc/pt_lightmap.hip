// pt_lightmap.hip — lightmap charts on the MI355X (include/ptmi_plugin.h Part 14): the rule of chart_rule.h in
// kernels.  Rasterise: pt_lm_coverage runs a 16-lane group per triangle record over the 4x4-texel tiles of its snapped box and
// ends in one atomicMin on the owner word per covered texel; a record whose box holds more than kLargeBox texels is put on a list
// instead, and pt_lm_coverage_large spreads the 64x64-texel tiles of those boxes over all workgroups (a tile is rejected by the
// edge values at its corner samples; a wave covers 32x2 texels per step, two 128-byte segments of owner words).  The owner map
// is then compacted in the three steps of pt_compact.h: pt_lm_count, pt_lm_scan, pt_lm_emit (one lane per texel: its place in the
// list, the receiver by chart_receiver).  Resolve: pt_lm_scatter and pt_lm_dilate.  The only atomics are integer min and add on
// 4-byte words, so the same input gives the same bytes.
#include "pt_lightmap.h"
#include "pt_compact.h"
#include "chart_rule.h"

using namespace ptchart;

namespace {

constexpr uint32_t kLargeBox = 1024u;         // texels of a snapped box beyond which a record goes to pt_lm_coverage_large
constexpr uint32_t kLargeBlocks = 2048u;      // its grid: 8 workgroups of 4 waves per CU
constexpr int32_t kTile = 64;                 // its tile edge in texels

struct Record {
    Snapped s;
    uint32_t prim;
    int32_t x0, y0, x1, y1;
};

// the UVs of primitive p: the caller's, or the attribute record's
__device__ __forceinline__ void prim_uvs(const PTChartArgs& A, uint32_t p, float uv[6])
{
    if (A.uvs) {
        const float2* u = (const float2*)(A.uvs + (size_t)p * 6u);
        const float2 a = u[0], b = u[1], c = u[2];
        uv[0] = a.x; uv[1] = a.y; uv[2] = b.x; uv[3] = b.y; uv[4] = c.x; uv[5] = c.y;
    } else {
        const float4 uv01 = A.attrs[(size_t)p * 8u + 6u], uv2m = A.attrs[(size_t)p * 8u + 7u];
        uv[0] = uv01.x; uv[1] = uv01.y; uv[2] = uv01.z; uv[3] = uv01.w; uv[4] = uv2m.x; uv[5] = uv2m.y;
    }
}

// Record t of the BLAS, snapped.  false: it is not in the chart, or covers no texel of the image.  A primIdx the BLAS cannot have
// (PTSetScene's validation and the plan's walk exclude it) is never used as an index.
__device__ __forceinline__ bool load_record(const PTChartArgs& A, uint32_t t, Record& r)
{
    const float4 e2 = A.tris[(size_t)t * 3u], e1 = A.tris[(size_t)t * 3u + 1u], v0 = A.tris[(size_t)t * 3u + 2u];
    r.prim = pt_asuint(v0.w);
    if (r.prim >= A.triCount) return false;
    float uv[6], g[3];
    prim_uvs(A, r.prim, uv);
    const float a1[3] = {e1.x, e1.y, e1.z}, a2[3] = {e2.x, e2.y, e2.z};
    if (!chart_setup(uv, A.width, A.height, r.s) || !chart_geometric_normal(a1, a2, g)) return false;
    return chart_bounds(r.s, A.width, A.height, r.x0, r.y0, r.x1, r.y1);
}

__global__ __launch_bounds__(256) void pt_lm_coverage(PTChartArgs A)
{
    const uint32_t t = blockIdx.x * 16u + (threadIdx.x >> 4), lane = threadIdx.x & 15u;
    if (t >= A.triCount) return;
    Record r;
    const bool in = load_record(A, t, r);
    if (r.prim < A.triCount && lane == 0u) A.recOfPrim[r.prim] = t;
    if (!in) return;
    if ((uint32_t)(r.x1 - r.x0 + 1) * (uint32_t)(r.y1 - r.y0 + 1) > kLargeBox) {
        if (lane == 0u) A.large[1u + atomicAdd(A.large, 1u)] = t;          // at most one entry per record: the list holds triCount
        return;
    }
    for (int32_t ty = r.y0; ty <= r.y1; ty += 4)
        for (int32_t tx = r.x0; tx <= r.x1; tx += 4) {
            const int32_t x = tx + (int32_t)(lane & 3u), y = ty + (int32_t)(lane >> 2);
            if (x <= r.x1 && y <= r.y1 && chart_covers(r.s, (uint32_t)x, (uint32_t)y))
                atomicMin(A.owner + ((size_t)y * A.width + (size_t)x), r.prim);
        }
}

// true: the whole tile [x0, x1] x [y0, y1] lies outside one edge.  An edge value is linear in the sample, so over the tile's
// samples it is largest at one of the four corner samples.
__device__ __forceinline__ bool tile_outside(const Snapped& s, int32_t x0, int32_t y0, int32_t x1, int32_t y1)
{
    int64_t mx[3];
    for (int c = 0; c < 4; ++c) {
        int64_t w[3];
        chart_edges(s, ((c & 1) ? x1 : x0) * kSubTexel + kHalfTexel, ((c & 2) ? y1 : y0) * kSubTexel + kHalfTexel, w);
        for (int k = 0; k < 3; ++k) {
            const int64_t v = s.A < 0 ? -w[k] : w[k];
            mx[k] = (c == 0 || v > mx[k]) ? v : mx[k];
        }
    }
    return mx[0] < 0 || mx[1] < 0 || mx[2] < 0;
}

__global__ __launch_bounds__(256) void pt_lm_coverage_large(PTChartArgs A)
{
    const uint32_t count = A.large[0] < A.triCount ? A.large[0] : A.triCount;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t t = A.large[1u + i];
        Record r;
        if (t >= A.triCount || !load_record(A, t, r)) continue;
        const uint32_t nx = (uint32_t)(r.x1 - r.x0) / (uint32_t)kTile + 1u, ny = (uint32_t)(r.y1 - r.y0) / (uint32_t)kTile + 1u;
        // every workgroup visits every listed record; record i's tiles start at another workgroup than record i - 1's
        for (uint32_t st = (blockIdx.x + i * 37u) % gridDim.x; st < nx * ny; st += gridDim.x) {
            const int32_t bx0 = r.x0 + (int32_t)(st % nx) * kTile, by0 = r.y0 + (int32_t)(st / nx) * kTile;
            const int32_t bx1 = bx0 + kTile - 1 < r.x1 ? bx0 + kTile - 1 : r.x1, by1 = by0 + kTile - 1 < r.y1 ? by0 + kTile - 1 : r.y1;
            if (tile_outside(r.s, bx0, by0, bx1, by1)) continue;
            // 64 steps of 32x2 texels, 16 per wave
            for (uint32_t k = wave; k < 64u; k += 4u) {
                const int32_t x = bx0 + (int32_t)(k & 1u) * 32 + (int32_t)(lane & 31u), y = by0 + (int32_t)(k >> 1) * 2 + (int32_t)(lane >> 5);
                if (x <= bx1 && y <= by1 && chart_covers(r.s, (uint32_t)x, (uint32_t)y))
                    atomicMin(A.owner + ((size_t)y * A.width + (size_t)x), r.prim);
            }
        }
    }
}

__global__ __launch_bounds__(256) void pt_lm_count(const uint32_t* __restrict__ owner, uint32_t n, uint32_t* __restrict__ blockBase)
{
    __shared__ uint32_t waveCount[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t total;
    compact_rank_in_block(i < n && owner[i] != kNoOwner, waveCount, total);
    if (threadIdx.x == 0u) blockBase[blockIdx.x] = total;
}

// at most 2^26 / 256 counts: 256 per thread
__global__ __launch_bounds__(1024) void pt_lm_scan(uint32_t* __restrict__ blockBase, uint32_t blocks, uint64_t* __restrict__ total)
{
    __shared__ uint32_t waveSum[16];
    const uint32_t all = compact_scan_blocks(blockBase, blocks, waveSum, [](uint32_t, uint32_t) {});
    if (threadIdx.x == 0u) *total = all;
}

__global__ __launch_bounds__(256) void pt_lm_emit(PTChartArgs A, uint32_t* __restrict__ texels, float4* __restrict__ recv)
{
    __shared__ uint32_t waveCount[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, n = A.width * A.height;
    const uint32_t p = i < n ? A.owner[i] : kNoOwner;
    const bool covered = p < A.triCount;
    uint32_t total;
    const uint32_t k = A.blockBase[blockIdx.x] + compact_rank_in_block(covered, waveCount, total);
    if (!covered) return;
    const uint32_t t = A.recOfPrim[p];
    if (t >= A.triCount) return;                                    // cannot happen: the coverage kernel wrote it
    const float4 r0 = A.tris[(size_t)t * 3u], r1 = A.tris[(size_t)t * 3u + 1u], r2 = A.tris[(size_t)t * 3u + 2u];
    const float4 a0 = A.attrs[(size_t)p * 8u], a1 = A.attrs[(size_t)p * 8u + 1u], a2 = A.attrs[(size_t)p * 8u + 2u];
    float uv[6];
    prim_uvs(A, p, uv);
    Snapped s;
    (void)chart_setup(uv, A.width, A.height, s);
    const float v0[3] = {r2.x, r2.y, r2.z}, e1[3] = {r1.x, r1.y, r1.z}, e2[3] = {r0.x, r0.y, r0.z};
    const float n0[3] = {a0.x, a0.y, a0.z}, n1[3] = {a1.x, a1.y, a1.z}, n2[3] = {a2.x, a2.y, a2.z};
    PTReceiver out;
    if (A.instance) {                                               // two calls: the matrices stay in registers
        float m[32];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 row = A.instance[q];
            m[4 * q] = row.x; m[4 * q + 1] = row.y; m[4 * q + 2] = row.z; m[4 * q + 3] = row.w;
        }
        chart_receiver(s, i % A.width, i / A.width, v0, e1, e2, n0, n1, n2, m, m + 16, A.seedBase + i, out);
    } else {
        chart_receiver(s, i % A.width, i / A.width, v0, e1, e2, n0, n1, n2, nullptr, nullptr, A.seedBase + i, out);
    }
    texels[k] = i;
    recv[(size_t)k * 2u] = make_float4(out.position[0], out.position[1], out.position[2], pt_asfloat(out.seed));
    recv[(size_t)k * 2u + 1u] = make_float4(out.normal[0], out.normal[1], out.normal[2], pt_asfloat(0u));
}

__global__ __launch_bounds__(256) void pt_lm_scatter(const uint32_t* __restrict__ texels, const float4* __restrict__ irr, uint64_t count, uint32_t n,
                                                     float4* __restrict__ image)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t t = texels[i];
    if (t >= n) return;
    const float4 e = irr[i];
    image[t] = make_float4(e.x, e.y, e.z, 1.0f);
}

__global__ __launch_bounds__(256) void pt_lm_dilate(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t width, uint32_t height)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const float4 c = src[i];
    if (c.w != 0.0f) { dst[i] = c; return; }                        // chart_dilate's first line, before the neighbours are fetched
    const int32_t x = (int32_t)(i % width), y = (int32_t)(i / width);
    float nb[8][4];
    uint32_t inside = 0;
    int k = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int32_t xx = x + dx, yy = y + dy;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (xx >= 0 && yy >= 0 && xx < (int32_t)width && yy < (int32_t)height) {
                inside |= 1u << k;
                v = src[(size_t)yy * width + (size_t)xx];
            }
            nb[k][0] = v.x; nb[k][1] = v.y; nb[k][2] = v.z; nb[k][3] = v.w;
            ++k;
        }
    const float self[4] = {c.x, c.y, c.z, c.w};
    float o[4];
    chart_dilate(self, nb, inside, o);
    dst[i] = make_float4(o[0], o[1], o[2], o[3]);
}

} // namespace

size_t pt_lm_blocks(uint32_t width, uint32_t height) { return ((size_t)width * height + 255u) / 256u; }

hipError_t pt_launch_lm_coverage(const PTChartArgs& A, hipStream_t stream)
{
    const size_t n = (size_t)A.width * A.height;
    const uint32_t blocks = (uint32_t)pt_lm_blocks(A.width, A.height);
    hipError_t e;
    if ((e = hipMemsetAsync(A.owner, 0xFF, n * 4u, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(A.large, 0, 4u, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt_lm_coverage, dim3((A.triCount + 15u) / 16u), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(pt_lm_coverage_large, dim3(kLargeBlocks), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(pt_lm_count, dim3(blocks), dim3(256), 0, stream, A.owner, (uint32_t)n, A.blockBase);
    hipLaunchKernelGGL(pt_lm_scan, dim3(1), dim3(1024), 0, stream, A.blockBase, blocks, A.total);
    return hipGetLastError();
}

hipError_t pt_launch_lm_emit(const PTChartArgs& A, uint32_t* texels, PTReceiver* recv, hipStream_t stream)
{
    hipLaunchKernelGGL(pt_lm_emit, dim3((uint32_t)pt_lm_blocks(A.width, A.height)), dim3(256), 0, stream, A, texels, (float4*)recv);
    return hipGetLastError();
}

hipError_t pt_launch_lm_resolve(const uint32_t* texels, const PTIrradiance* irr, uint64_t count, uint32_t width, uint32_t height, uint32_t dilate,
                                float4* image, float4* other, hipStream_t stream)
{
    const size_t n = (size_t)width * height;
    const uint32_t blocks = (uint32_t)pt_lm_blocks(width, height);
    // pass p reads the image of pass p - 1: an even number of passes starts in `image`, an odd one in `other`
    float4* cur = (dilate & 1u) ? other : image;
    float4* nxt = (dilate & 1u) ? image : other;
    hipError_t e;
    if ((e = hipMemsetAsync(cur, 0, n * 16u, stream)) != hipSuccess) return e;
    if (count) hipLaunchKernelGGL(pt_lm_scatter, dim3((uint32_t)((count + 255u) / 256u)), dim3(256), 0, stream, texels, (const float4*)irr, count, (uint32_t)n, cur);
    for (uint32_t p = 0; p < dilate; ++p) {
        hipLaunchKernelGGL(pt_lm_dilate, dim3(blocks), dim3(256), 0, stream, cur, nxt, width, height);
        float4* t = cur; cur = nxt; nxt = t;
    }
    return hipGetLastError();
}
