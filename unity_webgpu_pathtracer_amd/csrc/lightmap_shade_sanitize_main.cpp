// lightmap_shade_sanitize_main.cpp — the host twin of the lightmap lookup (lightmap_lookup_host.cpp) under AddressSanitizer +
// UBSan, stand-alone: `make lightmap-shade-sanitize` builds and runs it.  It walks the shapes tests/test_lightmap_shade.py uses --
// images of 1 x 1, 2 x 2, 8 x 8 and 24 x 8, full, with every other texel cleared, with one filled texel, cleared, with w of 1, 0.5, 0,
// -1 and NaN; UVs that put x on -1, on the width, on a texel centre and edge, and a NaN; UV arrays given and not; 0, 1, 3 and 64
// bindings, overlapping spans, instances, both sides; a miss every seventh entry and material indices out of range -- with every
// array allocated at its exact size, so that a read past an end is reported.  No GPU involved.
#include "lightmap_lookup_rule.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

namespace {

uint32_t g_state = 0x2468ACEu;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int fail(const char* what, const std::string& err)
{
    std::fprintf(stderr, "lightmap-shade-sanitize: %s: %s\n", what, err.c_str());
    return 1;
}

// an image at its exact size, 16-byte aligned (operator new's alignment); kind: 0 full, 1 every other texel cleared, 2 one filled
// texel, 3 cleared, 4 w runs through five values; the rgb of a texel that is not valid is NaN
std::vector<float> make_image(uint32_t w, uint32_t h, int kind)
{
    const float wv[5] = {1.0f, 0.5f, 0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN()};
    std::vector<float> img((size_t)w * h * 4);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            float* t = &img[4 * ((size_t)y * w + x)];
            t[3] = kind == 0 ? 1.0f : kind == 1 ? ((x + y) % 2 == 0 ? 1.0f : 0.0f) : kind == 2 ? (x == w / 2 && y == h / 2 ? 1.0f : 0.0f) : kind == 3 ? 0.0f : wv[(x + 2 * y) % 5];
            for (int c = 0; c < 3; ++c) t[c] = t[3] > 0.0f ? rnd() * 4.0f : std::numeric_limits<float>::quiet_NaN();
        }
    return img;
}

} // namespace

int main()
{
    std::string err;
    const uint32_t prims = 80, materials = 5;
    const float special[8] = {-0.0625f, 1.0625f, 0.4375f, 0.5f, std::numeric_limits<float>::quiet_NaN(), 0.0f, 1.0f, -0.07f};
    std::vector<PTTriangleAttributes> attrs(prims);
    std::vector<float> uvs((size_t)prims * 6);
    for (uint32_t p = 0; p < prims; ++p) {
        PTTriangleAttributes& a = attrs[p];
        a = PTTriangleAttributes{};
        for (int k = 0; k < 2; ++k) { a.uv0[k] = 0.02f + 0.96f * rnd(); a.uv1[k] = 0.02f + 0.96f * rnd(); a.uv2[k] = 0.02f + 0.96f * rnd(); }
        if (p >= 64 && p < 72) { a.uv0[0] = special[p - 64]; a.uv0[1] = 0.4375f; }
        if (p >= 72) { a.uv0[0] = 0.4375f; a.uv0[1] = special[p - 72]; }
        const float row[6] = {a.uv0[0], a.uv0[1], a.uv1[0], a.uv1[1], a.uv2[0], a.uv2[1]};
        for (int k = 0; k < 6; ++k) uvs[6 * (size_t)p + k] = row[k];
    }
    const uint64_t n = 1024;
    std::vector<PTRay> rays(n);
    std::vector<PTRayHit> hits(n);
    std::vector<PTRaySurface> S(n);
    for (uint64_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) {
            rays[i].origin[a] = rnd() * 2.0f - 1.0f;
            rays[i].direction[a] = (rnd() * 2.0f - 1.0f) * 1.5f;
            S[i].position[a] = rnd() * 2.0f - 1.0f;
            S[i].normal[a] = rnd() * 2.0f - 1.0f;               // about half face away
        }
        rays[i].tmax = 1e30f;
        rays[i].reserved = 0u;
        float b1 = rnd(), b2 = rnd();
        if (b1 + b2 > 1.0f) { b1 = 1.0f - b1; b2 = 1.0f - b2; }
        hits[i] = PTRayHit{rnd() * 3.0f, b1, b2, (uint32_t)(rnd() * 64.0f) % 64u};
        S[i].t = hits[i].t;
        S[i].materialIndex = (int32_t)(i % materials);
        S[i].uv[0] = rnd(); S[i].uv[1] = rnd();
        S[i].instance = i % 4 == 3 ? 0xFFFFFFFFu : (uint32_t)(i % 4);
        S[i].prim = hits[i].prim;
        if (i < 16) { hits[i].prim = 64u + (uint32_t)i; hits[i].u = hits[i].v = 0.0f; }
        if (i >= 16 && i < 20) { const uint32_t around[4] = {9u, 10u, 19u, 20u}; hits[i].prim = around[i - 16]; }
        if (i < 20) for (int a = 0; a < 3; ++a) S[i].normal[a] = -rays[i].direction[a];
        if (i >= 20 && i % 50 == 25) S[i].materialIndex = (int32_t)materials;
        if (i >= 20 && i % 50 == 26) S[i].materialIndex = -1;
        if (i >= 20 && i % 7 == 3) hits[i] = PTRayHit{1e30f, 0.0f, 0.0f, 0xFFFFFFFFu};
    }
    std::vector<PTIrradiance> out(n);
    std::vector<uint32_t> which(n);
    const uint32_t sizes[4][2] = {{1, 1}, {2, 2}, {8, 8}, {24, 8}};
    uint64_t found = 0, looked = 0;
    const auto run = [&](const std::vector<PTLightmapBinding>& table, const char* what) {
        if (!ptlm::lookup_host(table.data(), (uint32_t)table.size(), attrs.data(), prims, materials, rays.data(), hits.data(), S.data(), n, out.data(),
                               which.data(), err))
            return fail(what, err);
        for (uint64_t i = 0; i < n; ++i) {
            looked++;
            if (which[i] == PT_LIGHTMAP_NONE) {
                if (out[i].rgb[0] != 0.0f || out[i].rgb[1] != 0.0f || out[i].rgb[2] != 0.0f || out[i].m2 != 0.0f) return fail(what, "a not-found entry is not zero");
                continue;
            }
            found++;
            if (which[i] >= table.size() || hits[i].prim == 0xFFFFFFFFu) return fail(what, "a binding index out of range, or a miss found one");
            for (int c = 0; c < 3; ++c)
                if (!(out[i].rgb[c] >= 0.0f && out[i].rgb[c] <= 4.0f)) return fail(what, "a found entry read a texel that is not valid");
        }
        return 0;
    };
    // 1. every size and kind, whole span, UVs from the records and from the array, one- and two-sided
    std::vector<std::vector<float>> images;
    for (int s = 0; s < 4; ++s)
        for (int kind = 0; kind < 5; ++kind) images.push_back(make_image(sizes[s][0], sizes[s][1], kind));
    for (int s = 0; s < 4; ++s)
        for (int kind = 0; kind < 5; ++kind) {
            PTLightmapBinding b = {0u, prims, 0xFFFFFFFFu, (s + kind) % 3 == 0 ? PT_LIGHTMAP_TWO_SIDED : 0u, sizes[s][0], sizes[s][1], {0u, 0u},
                                   images[(size_t)s * 5 + kind].data(), (s + kind) % 2 ? uvs.data() : nullptr};
            if (int rc = run({b}, "one binding")) return rc;
        }
    // 2. no binding; three; overlapping spans; the same span for two instances; 64 bindings of one primitive each
    if (int rc = run({}, "no binding")) return rc;
    const auto full = [&](int s, uint32_t first, uint32_t count, uint32_t instance, uint32_t flags, const float* uv) {
        return PTLightmapBinding{first, count, instance, flags, sizes[s][0], sizes[s][1], {0u, 0u}, images[(size_t)s * 5].data(), uv};
    };
    if (int rc = run({full(2, 0, 10, 0xFFFFFFFFu, 0u, nullptr), full(3, 10, 10, 0xFFFFFFFFu, 1u, nullptr), full(1, 20, prims - 20, 0xFFFFFFFFu, 0u, uvs.data() + 6 * 20)},
                     "three bindings"))
        return rc;
    if (int rc = run({full(2, 0, 40, 0xFFFFFFFFu, 1u, nullptr), full(3, 20, 40, 0xFFFFFFFFu, 1u, nullptr)}, "overlap")) return rc;
    if (int rc = run({full(2, 0, prims, 1u, 1u, nullptr), full(3, 0, prims, 2u, 1u, nullptr)}, "instances")) return rc;
    std::vector<PTLightmapBinding> many;
    for (uint32_t k = 0; k < 64; ++k) many.push_back(full((int)(k % 4), k, 1u, 0xFFFFFFFFu, k % 2 ? 0u : 1u, k % 3 ? nullptr : uvs.data() + 6 * (size_t)k));
    if (int rc = run(many, "64 bindings")) return rc;
    // 3. refusals
    const PTLightmapBinding good = full(2, 0, prims, 0xFFFFFFFFu, 0u, nullptr);
    std::vector<PTLightmapBinding> bad(9, good);
    bad[0].dImage = nullptr;
    bad[1].dImage = (const char*)good.dImage + 4;
    bad[2].dUvs = (const float*)((const char*)uvs.data() + 4);
    bad[3].width = 0u;
    bad[4].height = PT_CHART_MAX_SIZE + 1u;
    bad[5].primCount = 0u;
    bad[6].firstPrim = 1u;                              // 1 + 80 is past the 80 records
    bad[7].flags = 2u;
    bad[8].reserved[1] = 1u;
    for (const PTLightmapBinding& b : bad)
        if (ptlm::lookup_host(&b, 1u, attrs.data(), prims, materials, rays.data(), hits.data(), S.data(), n, out.data(), which.data(), err))
            return fail("refusals", "accepted a bad binding");
    many.push_back(good);
    if (ptlm::lookup_host(many.data(), 65u, attrs.data(), prims, materials, rays.data(), hits.data(), S.data(), n, out.data(), which.data(), err) ||
        ptlm::lookup_host(nullptr, 1u, attrs.data(), prims, materials, rays.data(), hits.data(), S.data(), n, out.data(), which.data(), err) ||
        ptlm::lookup_host(&good, 1u, nullptr, prims, materials, rays.data(), hits.data(), S.data(), n, out.data(), which.data(), err) ||
        ptlm::lookup_host(&good, 1u, attrs.data(), prims, materials, nullptr, hits.data(), S.data(), n, out.data(), which.data(), err))
        return fail("refusals", "accepted bad arguments");
    if (!ptlm::lookup_host(&good, 1u, attrs.data(), prims, materials, nullptr, nullptr, nullptr, 0, nullptr, nullptr, err)) return fail("count 0", err);
    if (found == 0 || found == looked) return fail("coverage", "every entry found a lightmap, or none did");
    std::printf("lightmap shade ok: %llu of %llu lookups found a lightmap\n", (unsigned long long)found, (unsigned long long)looked);
    return 0;
}
