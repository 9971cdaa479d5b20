// lightmap_lookup_rule.h — first hits shaded from baked lightmaps (include/ptmi_plugin.h Part 22): the one
// definition of the rule -- the side rule, the binding choice, the UV interpolation, the texel footprint and the filter clamped to
// the valid taps -- shared by the kernels (pt_shade_lightmap.hip) and the host twin (lightmap_lookup_host.cpp).  Every fp32
// operator is one IEEE binary32 operation in the order written, and both sides are compiled with -ffp-contract=off, so both give
// the same bits.  tests/lightmap_lookup_ref.py restates it.  The view vector and d are shade_rule.h's.
#pragma once
#include "shade_rule.h"

#define PT_LM_HD PT_SHADE_HD

namespace ptlm {

// step 1: a hit seen from behind (d of Part 21 step 2, before the flip)
PT_LM_HD bool seen_from_behind(const float D[3], const float N[3])
{
    float Vd[3];
    return ptshade::view_dot(D, N, Vd) < 0.0f;
}

// step 2 for one record
PT_LM_HD bool matches(const PTLightmapBinding& b, uint32_t prim, uint32_t instance, bool back)
{
    return (uint32_t)(prim - b.firstPrim) < b.primCount && (b.instance == 0xFFFFFFFFu || b.instance == instance) &&
           (!back || (b.flags & PT_LIGHTMAP_TWO_SIDED) != 0u);
}

// what a lane keeps of the binding it chose
struct Chosen {
    uint32_t index, firstPrim, width, height;
    const void* image;
    const float* uvs;
};

// Step 2.  loadBinding(k) returns record k; allDone(done) says whether the walk may stop: the host answers `done`, a kernel
// whether every lane of the wave is done (k stays the same in every lane).  A miss starts done.
template <class LoadBinding, class AllDone>
PT_LM_HD void choose(bool miss, uint32_t prim, uint32_t instance, bool back, uint32_t bindingCount, LoadBinding loadBinding, AllDone allDone, Chosen& c)
{
    c = {PT_LIGHTMAP_NONE, 0u, 0u, 0u, nullptr, nullptr};
    bool done = miss;
    for (uint32_t k = 0; k < bindingCount; ++k) {
        if (allDone(done)) break;
        const PTLightmapBinding b = loadBinding(k);
        if (!done && matches(b, prim, instance, back)) {
            c = {k, b.firstPrim, b.width, b.height, b.dImage, b.dUvs};
            done = true;
        }
    }
}

// step 3, one coordinate
PT_LM_HD float interpolate(float u0, float u1, float u2, float b1, float b2)
{
    const float w0 = 1.0f - b1 - b2;
    return (u0 * w0 + u1 * b1) + u2 * b2;
}

// step 4, one axis: false: outside the footprint's reach (a NaN too).  f: the fraction; in0, in1: the taps lie inside; c0, c1: the
// taps clamped into the image, which is what is loaded -- a tap outside is never valid, so what the clamped load returns is not used
PT_LM_HD bool axis(float u, uint32_t size, float& f, bool& in0, bool& in1, uint32_t& c0, uint32_t& c1)
{
    const float x = u * (float)size - 0.5f;
    if (!(x > -1.0f && x < (float)size)) return false;
    const float xf = pt_floor(x);
    const int32_t x0 = (int32_t)xf;
    f = x - xf;
    in0 = x0 >= 0;
    in1 = x0 + 1 < (int32_t)size;
    c0 = in0 ? (uint32_t)x0 : 0u;
    c1 = in1 ? (uint32_t)(x0 + 1) : size - 1u;
    return true;
}

// step 5, one row or the two rows: a and b are used only where valid
PT_LM_HD bool blend(bool va, bool vb, const float a[3], const float b[3], float f, float r[3])
{
    for (uint32_t c = 0; c < 3u; ++c) r[c] = (va && vb) ? a[c] + f * (b[c] - a[c]) : (va ? a[c] : b[c]);
    return va || vb;
}

// Steps 4 and 5.  loadTaps(const uint32_t index[4], float t[4][4]) reads the texels index = y * width + x of c00, c10, c01, c11: a
// kernel requests the four before the first is used.
template <class LoadTaps>
PT_LM_HD bool filter(uint32_t width, uint32_t height, float U, float V, LoadTaps loadTaps, float E[3])
{
    float fx, fy;
    bool inx0, inx1, iny0, iny1;
    uint32_t cx0, cx1, cy0, cy1;
    const bool okx = axis(U, width, fx, inx0, inx1, cx0, cx1);
    const bool oky = axis(V, height, fy, iny0, iny1, cy0, cy1);
    if (!(okx && oky)) return false;
    const uint32_t index[4] = {cy0 * width + cx0, cy0 * width + cx1, cy1 * width + cx0, cy1 * width + cx1};
    float t[4][4];
    loadTaps(index, t);
    const float *t00 = t[0], *t10 = t[1], *t01 = t[2], *t11 = t[3];
    const bool v00 = inx0 && iny0 && t00[3] > 0.0f, v10 = inx1 && iny0 && t10[3] > 0.0f;
    const bool v01 = inx0 && iny1 && t01[3] > 0.0f, v11 = inx1 && iny1 && t11[3] > 0.0f;
    float r0[3], r1[3];
    const bool row0 = blend(v00, v10, t00, t10, fx, r0);
    const bool row1 = blend(v01, v11, t01, t11, fx, r1);
    return blend(row0, row1, r0, r1, fy, E);
}

// Steps 2 to 6 for one entry whose step 1 the caller has taken (miss, back).  loadUv(chosen, prim, float uv[6]) gives the corners
// u0 v0 u1 v1 u2 v2; loadTaps(chosen, index, t) as filter takes it.  Returns the binding's index, E set; or PT_LIGHTMAP_NONE, E zero.
template <class LoadBinding, class AllDone, class LoadUv, class LoadTaps>
PT_LM_HD uint32_t lookup(bool miss, bool back, uint32_t prim, float b1, float b2, uint32_t instance, uint32_t bindingCount, LoadBinding loadBinding,
                         AllDone allDone, LoadUv loadUv, LoadTaps loadTaps, float E[4])
{
    for (uint32_t c = 0; c < 4u; ++c) E[c] = 0.0f;
    Chosen ch;
    choose(miss, prim, instance, back, bindingCount, loadBinding, allDone, ch);
    if (ch.index == PT_LIGHTMAP_NONE) return PT_LIGHTMAP_NONE;
    float uv[6];
    loadUv(ch, prim, uv);
    const float U = interpolate(uv[0], uv[2], uv[4], b1, b2), V = interpolate(uv[1], uv[3], uv[5], b1, b2);
    float e[3];
    if (!filter(ch.width, ch.height, U, V, [&](const uint32_t index[4], float t[4][4]) { loadTaps(ch, index, t); }, e)) return PT_LIGHTMAP_NONE;
    E[0] = e[0]; E[1] = e[1]; E[2] = e[2];
    return ch.index;
}

// ---- the host twin and the check PTBindLightmaps shares with it (lightmap_lookup_host.cpp); false: err says why ----
// attrCount: the scene's attribute records; instanceCount: the scene's instances, or 0xFFFFFFFF: instances are not checked
bool check_bindings(const PTLightmapBinding* bindings, uint32_t count, uint64_t attrCount, uint32_t instanceCount, std::string& err);
bool lookup_host(const PTLightmapBinding* bindings, uint32_t bindingCount, const PTTriangleAttributes* attrs, uint64_t attrCount, uint32_t materialCount,
                 const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces, uint64_t count, PTIrradiance* out, uint32_t* outBinding,
                 std::string& err);

} // namespace ptlm
