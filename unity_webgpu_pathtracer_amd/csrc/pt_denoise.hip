// pt_denoise.hip — first-hit guide buffers and the a-trous denoiser (include/ptmi_plugin.h Part 4: PTRenderGuides / PTDenoise).
//
// Guides: one 64-lane wave per workgroup takes an 8x8 pixel block (lane = 8 * row + column), so its camera rays are coherent.
// The walk is the ray queries' (pt_query.hip): the render's traverse_cwbvh / traverse_tlas and fetch_hit_attributes[_tlas] from
// pt_device.h, the CWBVH stack PT_Q_LDS_STACK entries per lane in LDS ([entry][lane]) and the rest in an HBM slab of the
// context, addressed through spill_row on the wave index held in LDS: no private array, so the CWBVH kernel has no scratch.
// The grid is capped at the kernel's resident waves (pt_guide_grid_caps) and walks the 8x8 blocks grid-stride.  The albedo is
// GetBaseColorOpacity's base colour (get_material's first texture lookup, sample_texture's arithmetic).
//
// Filter: SVGF's spatial a-trous (DESIGN.md 5.9 states the formula).  Per pixel the filter state is one float4 (e.rgb, v) --
// v < 0 marks a background pixel -- and the guide one float4 (n.xyz, z): 32 bytes per tap.  One 256-thread workgroup per
// 16x16 tile.  Steps 1, 2 and 4 stage the tile plus its 2s halo (state and guide) in LDS; steps 8 and up read their taps
// through L2 / the Infinity Cache.  Launches: prepass + one per level + remodulation, ping-ponging between context buffers.
#include "pt_device.h"
#include "pt_launch.h"

namespace {

// GetBaseColorOpacity (util/material.hlsl:56-69) as get_material computes it: the material's base colour, times the bilinear
// texel of its base-colour texture at the transformed uv
PT_DEV v3 base_color(const DScene& S, const SurfHit& hit, Counters& cn)
{
    const float4* mp = S.materials + (size_t)hit.materialIndex * 8;
    const float4 d1 = mp[0], d6t1 = mp[5], tr = mp[7];
    v4 bco = {d1.x, d1.y, d1.z, d1.w};
    if (S.hasTextures != 0u && !(d6t1.z < 0.0f)) {
        const v2 tuv = {hit.uv.x * tr.x + tr.z, hit.uv.y * tr.y + tr.w};
        bco = sample_texture<false>(S, pt_f2i(d6t1.z), tuv, cn) * bco;
    }
    return mk3(bco.x, bco.y, bco.z);
}

template <bool TLAS>
PT_DEV void guide_body(const DScene& S, const PTFrameParams& P, uint32_t n, float4* __restrict__ albedo,
                       float4* __restrict__ normalDepth, uint2* __restrict__ slab)
{
    const uint32_t lane = threadIdx.x;
    Counters cn = {};
    TravStackT<PT_Q_LDS_STACK, true> st;
    resident_wave_stack(st, slab);

    const uint32_t W = P.OutputWidth, H = P.OutputHeight;
    const uint32_t bw = (W + 7u) / 8u, blocks = bw * ((H + 7u) / 8u);
    const float fn = (float)n, samples = (float)(n * n);
    // generate_camera_ray without jitter and lens: the origin, then the ray through (x + (i + 0.5) / n, y + (j + 0.5) / n)
    const v4 o4 = mul44(P.CamToWorld, v4{0.0f, 0.0f, 0.0f, 1.0f});
    const v3 o = mk3(o4.x, o4.y, o4.z);
    for (uint32_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint32_t x = (b % bw) * 8u + (lane & 7u), y = (b / bw) * 8u + (lane >> 3);
        if (x >= W || y >= H) continue;
        v3 asum = mk3(0.0f), nsum = mk3(0.0f);
        float dsum = 0.0f;
        uint32_t hits = 0u;
        for (uint32_t j = 0; j < n; ++j) {
            for (uint32_t i = 0; i < n; ++i) {
                const float pcx = (float)x + ((float)i + 0.5f) / fn;       // exact: a dyadic offset
                const float pcy = (float)y + ((float)j + 0.5f) / fn;
                const float uvx = pcx / (float)W * 2.0f - 1.0f;
                const float uvy = pcy / (float)H * 2.0f - 1.0f;
                const v4 d4 = mul44(P.CamInvProj, v4{uvx, uvy, 0.0f, 1.0f});
                const v4 w4 = mul44(P.CamToWorld, v4{d4.x, d4.y, d4.z, 0.0f});
                const v3 d = normalize3(mk3(w4.x, w4.y, w4.z));
                HitRecord rec = miss_record(PT_FAR_PLANE);
                bool found;
                if (TLAS) {
                    traverse_tlas<false>(S, o, d, false, rec, st, cn);
                    found = rec.inst != 0xFFFFFFFFu;
                } else {
                    traverse_cwbvh<false>(S, o, d, false, rec.h, st, cn);
                    found = rec.h.t < PT_FAR_PLANE;
                }
                if (found) {
                    SurfHit sh;
                    if (TLAS) fetch_hit_attributes_tlas(S, d, rec, sh);
                    else fetch_hit_attributes<false>(S, o, d, rec.h, sh, cn);
                    asum = asum + base_color(S, sh, cn);
                    // the first hitting sample's normal and distance are taken as they are (no 0 + x: keeps a -0 component)
                    nsum = hits == 0u ? sh.normal : nsum + sh.normal;
                    dsum = hits == 0u ? sh.distance : dsum + sh.distance;
                    ++hits;
                } else {
                    asum = asum + mk3(1.0f);
                }
            }
        }
        v3 nrm = nsum;
        if (hits > 1u) nrm = dot3(nsum, nsum) > 0.0f ? normalize3(nsum) : mk3(0.0f);
        const size_t p = (size_t)y * W + x;
        albedo[p] = make_float4(asum.x / samples, asum.y / samples, asum.z / samples, (float)hits / samples);
        normalDepth[p] = make_float4(nrm.x, nrm.y, nrm.z, hits ? dsum / (float)hits : 0.0f);
    }
}

} // namespace

// Stable, unmangled kernel names (rocprofv3 --kernel-trace lists them as they are written here).
extern "C" __global__ __launch_bounds__(64) void pt_guides(DScene S, PTFrameParams P, uint32_t n, float4* __restrict__ albedo,
                                                           float4* __restrict__ normalDepth, uint2* __restrict__ slab)
{
    guide_body<false>(S, P, n, albedo, normalDepth, slab);
}
extern "C" __global__ __launch_bounds__(64) void pt_guides_tlas(DScene S, PTFrameParams P, uint32_t n, float4* __restrict__ albedo,
                                                                float4* __restrict__ normalDepth, uint2* __restrict__ slab)
{
    guide_body<true>(S, P, n, albedo, normalDepth, slab);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the a-trous filter
// ---------------------------------------------------------------------------------------------------------------------------
#define PT_DN_TILE 16u          // 16x16 pixels per 256-thread workgroup

namespace {

PT_DEV float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

PT_DEV float4 dn_demod(float4 c, float4 a, bool demod)
{
    if (!demod) return c;
    return make_float4(c.x / pt_max(a.x, 1e-3f), c.y / pt_max(a.y, 1e-3f), c.z / pt_max(a.z, 1e-3f), c.w);
}

// One level for pixel (x, y).  TAP(qx, qy, s, g) fetches the state and guide of a pixel inside the image; taps outside the image
// or with s.w < 0 (background) take no part.  INSIDE(qx, qy) says whether (qx, qy) lies in the image.
template <class Tap, class Inside>
PT_DEV float4 atrous_pixel(const PTDenoiseArgs& A, int step, int x, int y, float4 sp, float4 gp, float2 gz, Tap tap, Inside inside)
{
    // g3x3(v): the {1/4, 1/2, 1/4}^2 blur of v over the covered pixels around p (p itself is covered)
    float vw = 0.0f, vs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (!inside(qx, qy)) continue;
            float4 s, g;
            tap(qx, qy, s, g);
            if (s.w < 0.0f) continue;
            const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            vw += k;
            vs += k * s.w;
        }
    }
    const float lp = dn_lum(sp.x, sp.y, sp.z);
    const float denomL = A.sigmaL * pt_sqrt(pt_max(vs / vw, 0.0f)) + 1e-6f;
    const float zp = gp.w;
    float sw = 0.0f, sv = 0.0f, er = 0.0f, eg = 0.0f, eb = 0.0f;
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx, qy = y + step * dy;
            if (!inside(qx, qy)) continue;
            float4 s, g;
            tap(qx, qy, s, g);
            if (s.w < 0.0f) continue;
            const float wl = expf(-fabsf(lp - dn_lum(s.x, s.y, s.z)) / denomL);
            const float wn = powf(pt_max(0.0f, gp.x * g.x + gp.y * g.y + gp.z * g.z), A.sigmaN);
            const float dz = fabsf(gz.x * (float)(step * dx) + gz.y * (float)(step * dy));
            const float wz = expf(-fabsf(zp - g.w) / (A.sigmaZ * dz + 1e-3f * zp + 1e-6f));
            const float w = h[dx + 2] * h[dy + 2] * wl * wn * wz;
            sw += w;
            sv += w * w * s.w;
            er += w * s.x; eg += w * s.y; eb += w * s.z;
        }
    }
    if (!(sw > 0.0f)) return sp;                                        // every weight underflowed: keep the pixel
    return make_float4(er / sw, eg / sw, eb / sw, sv / (sw * sw));
}

} // namespace

// Prepass: demodulated colour, its luminance variance over the covered 3x3 and the depth gradient.
extern "C" __global__ __launch_bounds__(256) void pt_denoise_prepass(PTDenoiseArgs A, const float4* __restrict__ src,
                                                                     const float4* __restrict__ albedo,
                                                                     const float4* __restrict__ normalDepth,
                                                                     float4* __restrict__ state, float2* __restrict__ gradz)
{
    const int W = (int)A.width, H = (int)A.height;
    const int x = (int)(blockIdx.x * PT_DN_TILE + threadIdx.x % PT_DN_TILE), y = (int)(blockIdx.y * PT_DN_TILE + threadIdx.x / PT_DN_TILE);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 a = albedo[p];
    if (!(a.w > 0.0f)) {
        state[p] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        gradz[p] = make_float2(0.0f, 0.0f);
        return;
    }
    const bool demod = (A.flags & PT_DENOISE_DEMODULATE_ALBEDO) != 0u;
    float l[9];
    bool cov[9];
    float lsum = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int qx = x + k % 3 - 1, qy = y + k / 3 - 1;
        cov[k] = false;
        l[k] = 0.0f;
        if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
        const size_t q = (size_t)qy * W + qx;
        const float4 aq = albedo[q];
        if (!(aq.w > 0.0f)) continue;
        const float4 e = dn_demod(src[q], aq, demod);
        cov[k] = true;
        l[k] = dn_lum(e.x, e.y, e.z);
        lsum += l[k];
        ++cnt;
    }
    const float mean = lsum / (float)cnt;
    float var = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        if (cov[k]) var += (l[k] - mean) * (l[k] - mean);
    var = pt_max(var / (float)cnt, 0.0f);
    const float4 e = dn_demod(src[p], a, demod);
    state[p] = make_float4(e.x, e.y, e.z, var);
    // central difference on covered neighbours, one-sided where one is uncovered, 0 where both are
    const float zc = normalDepth[p].w;
    float g[2];
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
        const bool cm = cov[axis == 0 ? 3 : 1], cp = cov[axis == 0 ? 5 : 7];
        const size_t qm = axis == 0 ? p - 1 : p - (size_t)W, qp = axis == 0 ? p + 1 : p + (size_t)W;
        const float zm = cm ? normalDepth[qm].w : 0.0f, zq = cp ? normalDepth[qp].w : 0.0f;
        g[axis] = cm && cp ? (zq - zm) * 0.5f : cp ? zq - zc : cm ? zc - zm : 0.0f;
    }
    gradz[p] = make_float2(g[0], g[1]);
}

// The prepass of PTDenoiseMoments: the same state and depth gradient, but v at a covered pixel is the variance of the MEAN of the
// filter luminance, from the moment planes of PTAccumulateMoments (include/ptmi_plugin.h Part 6).  The demodulated luminance is
// sum_c (w_c / max(albedo_c, 1e-3)) e_c, linear in rgb with per-pixel constants, so its variance is the quadratic form of the
// rgb covariance.  Only the four axis neighbours' coverage is read (for the gradient).
extern "C" __global__ __launch_bounds__(256) void pt_denoise_prepass_moments(PTDenoiseArgs A, PTDenoiseVariance V,
                                                                             const float4* __restrict__ src,
                                                                             const float4* __restrict__ albedo,
                                                                             const float4* __restrict__ normalDepth,
                                                                             float4* __restrict__ state, float2* __restrict__ gradz)
{
    const int W = (int)A.width, H = (int)A.height;
    const int x = (int)(blockIdx.x * PT_DN_TILE + threadIdx.x % PT_DN_TILE), y = (int)(blockIdx.y * PT_DN_TILE + threadIdx.x / PT_DN_TILE);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 a = albedo[p];
    if (!(a.w > 0.0f)) {
        state[p] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        gradz[p] = make_float2(0.0f, 0.0f);
        return;
    }
    const bool demod = (A.flags & PT_DENOISE_DEMODULATE_ALBEDO) != 0u;
    const float4 s0 = V.plane0[p];
    // adaptive sampling: every 16x16 block has its own observation and sample counts
    const float invDof = V.blockInvDof ? V.blockInvDof[(size_t)(y >> 4) * (size_t)((W + 15) >> 4) + (size_t)(x >> 4)] : V.invDof;
    float var;
    if (demod) {
        const float4 s1 = V.plane1[p];
        const float qr = 0.2126f / pt_max(a.x, 1e-3f), qg = 0.7152f / pt_max(a.y, 1e-3f), qb = 0.0722f / pt_max(a.z, 1e-3f);
        const float diag = (qr * qr) * s0.x + (qg * qg) * s0.y + (qb * qb) * s0.z;
        const float cross = (qr * qg) * s1.x + (qr * qb) * s1.y + (qg * qb) * s1.z;
        var = pt_max((diag + 2.0f * cross) * invDof, 0.0f);
    } else {
        var = pt_max(s0.w * invDof, 0.0f);
    }
    const float4 e = dn_demod(src[p], a, demod);
    state[p] = make_float4(e.x, e.y, e.z, var);
    // central difference on covered neighbours, one-sided where one is uncovered, 0 where both are (pt_denoise_prepass's rule)
    const float zc = normalDepth[p].w;
    float g[2];
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
        const bool im = axis == 0 ? x > 0 : y > 0, ip = axis == 0 ? x + 1 < W : y + 1 < H;
        const size_t qm = axis == 0 ? p - 1 : p - (size_t)W, qp = axis == 0 ? p + 1 : p + (size_t)W;
        const bool cm = im && albedo[qm].w > 0.0f, cp = ip && albedo[qp].w > 0.0f;
        const float zm = cm ? normalDepth[qm].w : 0.0f, zq = cp ? normalDepth[qp].w : 0.0f;
        g[axis] = cm && cp ? (zq - zm) * 0.5f : cp ? zq - zc : cm ? zc - zm : 0.0f;
    }
    gradz[p] = make_float2(g[0], g[1]);
}

// One a-trous level.  STEP > 0: the tile and its 2 * STEP halo staged in LDS; STEP == 0: step `step`, taps read from memory.
template <int STEP>
PT_DEV void atrous_level(const PTDenoiseArgs& A, int step, const float4* __restrict__ stateIn, const float4* __restrict__ normalDepth,
                         const float2* __restrict__ gradz, float4* __restrict__ stateOut)
{
    const int W = (int)A.width, H = (int)A.height;
    const int lx = (int)(threadIdx.x % PT_DN_TILE), ly = (int)(threadIdx.x / PT_DN_TILE);
    const int x0 = (int)(blockIdx.x * PT_DN_TILE), y0 = (int)(blockIdx.y * PT_DN_TILE);
    const int x = x0 + lx, y = y0 + ly;
    auto inside = [&](int qx, int qy) { return qx >= 0 && qy >= 0 && qx < W && qy < H; };
    if constexpr (STEP > 0) {
        constexpr int HALO = 2 * (STEP > 0 ? STEP : 1);
        constexpr int T = (int)PT_DN_TILE + 2 * HALO;
        __shared__ float4 s_state[T * T];
        __shared__ float4 s_guide[T * T];
        for (int k = (int)threadIdx.x; k < T * T; k += (int)blockDim.x) {
            const int gx = x0 - HALO + k % T, gy = y0 - HALO + k / T;
            float4 s = make_float4(0.0f, 0.0f, 0.0f, -1.0f), g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (inside(gx, gy)) {
                const size_t q = (size_t)gy * W + gx;
                s = stateIn[q];
                g = normalDepth[q];
            }
            s_state[k] = s;
            s_guide[k] = g;
        }
        __syncthreads();
        if (x >= W || y >= H) return;
        const int c = (ly + HALO) * T + (lx + HALO);
        const float4 sp = s_state[c];
        const size_t p = (size_t)y * W + x;
        if (sp.w < 0.0f) { stateOut[p] = sp; return; }
        // taps outside the image were staged as background: no bounds test needed
        auto tap = [&](int qx, int qy, float4& s, float4& g) {
            const int k = (qy - y0 + HALO) * T + (qx - x0 + HALO);
            s = s_state[k];
            g = s_guide[k];
        };
        auto always = [](int, int) { return true; };
        stateOut[p] = atrous_pixel(A, STEP, x, y, sp, s_guide[c], gradz[p], tap, always);
    } else {
        if (x >= W || y >= H) return;
        const size_t p = (size_t)y * W + x;
        const float4 sp = stateIn[p];
        if (sp.w < 0.0f) { stateOut[p] = sp; return; }
        auto tap = [&](int qx, int qy, float4& s, float4& g) {
            const size_t q = (size_t)qy * W + qx;
            s = stateIn[q];
            g = normalDepth[q];
        };
        stateOut[p] = atrous_pixel(A, step, x, y, sp, normalDepth[p], gradz[p], tap, inside);
    }
}

#define PT_DN_LEVEL(name, STEP)                                                                                                 \
    extern "C" __global__ __launch_bounds__(256) void name(PTDenoiseArgs A, int step, const float4* __restrict__ stateIn,       \
                                                           const float4* __restrict__ normalDepth,                              \
                                                           const float2* __restrict__ gradz, float4* __restrict__ stateOut)     \
    {                                                                                                                           \
        atrous_level<STEP>(A, step, stateIn, normalDepth, gradz, stateOut);                                                    \
    }
PT_DN_LEVEL(pt_denoise_atrous_s1, 1)
PT_DN_LEVEL(pt_denoise_atrous_s2, 2)
PT_DN_LEVEL(pt_denoise_atrous_s4, 4)
PT_DN_LEVEL(pt_denoise_atrous, 0)
#undef PT_DN_LEVEL

// out.rgb = e * max(albedo, 1e-3) (or e), out.a = the input's alpha; background pixels are the input's bits
extern "C" __global__ __launch_bounds__(256) void pt_denoise_remodulate(PTDenoiseArgs A, const float4* __restrict__ src,
                                                                        const float4* __restrict__ albedo,
                                                                        const float4* __restrict__ state, float4* dst)
{
    const int W = (int)A.width, H = (int)A.height;
    const int x = (int)(blockIdx.x * PT_DN_TILE + threadIdx.x % PT_DN_TILE), y = (int)(blockIdx.y * PT_DN_TILE + threadIdx.x / PT_DN_TILE);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 c = src[p];            // src may be dst (in place): each thread reads its pixel before it writes it
    const float4 a = albedo[p];
    if (!(a.w > 0.0f)) { dst[p] = c; return; }
    const float4 s = state[p];
    if ((A.flags & PT_DENOISE_DEMODULATE_ALBEDO) != 0u)
        dst[p] = make_float4(s.x * pt_max(a.x, 1e-3f), s.y * pt_max(a.y, 1e-3f), s.z * pt_max(a.z, 1e-3f), c.w);
    else
        dst[p] = make_float4(s.x, s.y, s.z, c.w);
}

namespace {
typedef void (*GuideKernel)(DScene, PTFrameParams, uint32_t, float4*, float4*, uint2*);
const GuideKernel kGuideKernels[2] = {pt_guides, pt_guides_tlas};
} // namespace

hipError_t pt_guide_grid_caps(int device, uint32_t caps[2])
{
    return pt_resident_wave_caps(device, kGuideKernels, 2, caps);
}

hipError_t pt_launch_guides(const DScene& S, const PTFrameParams& P, uint32_t n, float4* albedo, float4* normalDepth, uint2* slab,
                            uint32_t gridCap, hipStream_t stream)
{
    const uint32_t blocks = ((P.OutputWidth + 7u) / 8u) * ((P.OutputHeight + 7u) / 8u);
    const uint32_t grid = blocks < gridCap ? blocks : gridCap;
    if (grid == 0u) return hipSuccess;
    hipLaunchKernelGGL(kGuideKernels[S.hasTlas != 0u ? 1 : 0], dim3(grid), dim3(64), 0, stream, S, P, n, albedo, normalDepth, slab);
    return hipGetLastError();
}

hipError_t pt_launch_denoise(const PTDenoiseArgs& A, int iterations, const float4* src, float4* dst, const float4* albedo,
                             const float4* normalDepth, float4* state0, float4* state1, float2* gradz,
                             const PTDenoiseVariance* variance, hipStream_t stream)
{
    const dim3 grid((A.width + PT_DN_TILE - 1u) / PT_DN_TILE, (A.height + PT_DN_TILE - 1u) / PT_DN_TILE), block(PT_DN_TILE * PT_DN_TILE);
    if (variance) hipLaunchKernelGGL(pt_denoise_prepass_moments, grid, block, 0, stream, A, *variance, src, albedo, normalDepth, state0, gradz);
    else hipLaunchKernelGGL(pt_denoise_prepass, grid, block, 0, stream, A, src, albedo, normalDepth, state0, gradz);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    float4* in = state0;
    float4* out = state1;
    for (int k = 0; k < iterations; ++k) {
        const int step = 1 << k;
        if (step == 1) hipLaunchKernelGGL(pt_denoise_atrous_s1, grid, block, 0, stream, A, step, in, normalDepth, gradz, out);
        else if (step == 2) hipLaunchKernelGGL(pt_denoise_atrous_s2, grid, block, 0, stream, A, step, in, normalDepth, gradz, out);
        else if (step == 4) hipLaunchKernelGGL(pt_denoise_atrous_s4, grid, block, 0, stream, A, step, in, normalDepth, gradz, out);
        else hipLaunchKernelGGL(pt_denoise_atrous, grid, block, 0, stream, A, step, in, normalDepth, gradz, out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        float4* t = in; in = out; out = t;
    }
    hipLaunchKernelGGL(pt_denoise_remodulate, grid, block, 0, stream, A, src, albedo, in, dst);
    return hipGetLastError();
}
