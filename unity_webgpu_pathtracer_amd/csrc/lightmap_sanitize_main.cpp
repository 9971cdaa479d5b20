// lightmap_sanitize_main.cpp — the host twin of the lightmap kernels (chart_host.cpp) in a stand-alone program for
// `make lightmap-sanitize` (AddressSanitizer + UBSan, host code only, no GPU): rasterises a generated chart into exactly sized
// heap arrays (a unit quad that must cover every texel once, then a soup with NaN, far-away, mirrored and degenerate triangles),
// resolves it with dilation, and makes the refusals.  Prints "lightmap ok" and returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "chart_rule.h"

namespace {

uint32_t g_state = 4242u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("lightmap-sanitize: %s\n", what); return 1; }

// record t = primitive prim with corners a, b, c
void put(std::vector<PTFloat4>& tris, uint32_t t, uint32_t prim, const float a[3], const float b[3], const float c[3])
{
    tris[3 * t] = PTFloat4{c[0] - a[0], c[1] - a[1], c[2] - a[2], 0.0f};
    tris[3 * t + 1] = PTFloat4{b[0] - a[0], b[1] - a[1], b[2] - a[2], 0.0f};
    tris[3 * t + 2] = PTFloat4{a[0], a[1], a[2], 0.0f};
    std::memcpy(&tris[3 * t + 2].w, &prim, 4);
}

} // namespace

int main()
{
    using namespace ptchart;
    std::string err;
    // ---- the unit quad, records in reverse primitive order: every texel once
    {
        const uint32_t W = 37, H = 23;
        std::vector<PTFloat4> tris(6);
        std::vector<PTTriangleAttributes> attrs(2);
        const float p00[3] = {0, 0, 0}, p10[3] = {2, 0, 0}, p11[3] = {2, 0, 2}, p01[3] = {0, 0, 2};
        put(tris, 0, 1, p00, p11, p01);
        put(tris, 1, 0, p00, p10, p11);
        std::memset(attrs.data(), 0, attrs.size() * sizeof(attrs[0]));
        for (auto& a : attrs) a.normal0[1] = a.normal1[1] = a.normal2[1] = 1.0f;
        attrs[0].uv1[0] = 1; attrs[0].uv2[0] = 1; attrs[0].uv2[1] = 1;
        attrs[1].uv1[0] = 1; attrs[1].uv1[1] = 1; attrs[1].uv2[1] = 1;
        const ChartInput in = {tris.data(), attrs.data(), nullptr, nullptr, nullptr, 2, W, H, 0xFFFFFFF0u};
        uint64_t count = 0;
        if (!chart_rasterize_host(in, nullptr, nullptr, 0, count, err)) return bad(err.c_str());
        if (count != (uint64_t)W * H) return bad("the quad does not cover every texel");
        std::vector<uint32_t> texels(count);
        std::vector<PTReceiver> recv(count);
        if (!chart_rasterize_host(in, texels.data(), recv.data(), count, count, err)) return bad(err.c_str());
        for (uint64_t i = 0; i < count; ++i) {
            if (texels[i] != i || recv[i].seed != 0xFFFFFFF0u + (uint32_t)i || recv[i].normal[1] != 1.0f) return bad("a quad receiver is wrong");
            const float wx = 2.0f * ((float)(i % W) + 0.5f) / (float)W, wz = 2.0f * ((float)(i / W) + 0.5f) / (float)H;
            if (std::fabs(recv[i].position[0] - wx) > 2e-6f || std::fabs(recv[i].position[2] - wz) > 2e-6f) return bad("a quad receiver is misplaced");
        }
        uint64_t c2 = 0;
        if (chart_rasterize_host(in, texels.data(), recv.data(), count - 1, c2, err) || c2 != count) return bad("a capacity of one less was not refused");
    }
    // ---- a soup with everything the rule excludes, an instance, caller UVs
    {
        const uint32_t T = 257, W = 64, H = 61;
        std::vector<PTFloat4> tris(3 * T);
        std::vector<PTTriangleAttributes> attrs(T);
        std::vector<float> uvs((size_t)T * 6);
        for (uint32_t t = 0; t < T; ++t) {
            float v[3][3];
            for (auto& c : v) for (float& x : c) x = rnd() * 4 - 2;
            if (t % 17 == 3) std::memcpy(v[2], v[1], sizeof(v[1]));                   // degenerate in space
            put(tris, t, T - 1 - t, v[0], v[1], v[2]);
            float* r = reinterpret_cast<float*>(&attrs[t]);
            for (int k = 0; k < 32; ++k) r[k] = rnd() - 0.5f;
            if (t % 13 == 5) std::memset(r, 0, 48);                                   // zero normals: the geometric fallback
            const float cx = rnd() * 1.4f - 0.2f, cy = rnd() * 1.4f - 0.2f, s = t % 29 == 0 ? 0.9f : 0.12f;
            for (int k = 0; k < 3; ++k) { uvs[6 * t + 2 * k] = cx + (rnd() - 0.5f) * s; uvs[6 * t + 2 * k + 1] = cy + (rnd() - 0.5f) * s; }
            if (t % 19 == 1) uvs[6 * t + 2] = std::numeric_limits<float>::quiet_NaN();
            if (t % 23 == 2) uvs[6 * t + 5] = 600.0f;                                 // beyond 2^23 sub-texels
            if (t % 31 == 4) { uvs[6 * t + 4] = uvs[6 * t]; uvs[6 * t + 5] = uvs[6 * t + 1]; }     // no area
        }
        const float l2w[16] = {0, 2, 0, 0, -1.5f, 0, 0, 0, 0, 0, 0.5f, 0, 3, -1, 2, 1};
        const float w2l[16] = {0, -1 / 1.5f, 0, 0, 0.5f, 0, 0, 0, 0, 0, 2, 0, 0.5f, 2, -4, 1};
        for (int pass = 0; pass < 2; ++pass) {
            const ChartInput in = {tris.data(), attrs.data(), pass ? uvs.data() : nullptr, pass ? l2w : nullptr, pass ? w2l : nullptr, T, W, H, 7u};
            uint64_t count = 0;
            if (!chart_rasterize_host(in, nullptr, nullptr, 0, count, err)) return bad(err.c_str());
            std::vector<uint32_t> texels(count);
            std::vector<PTReceiver> recv(count);
            std::vector<PTIrradiance> irr(count);
            if (!chart_rasterize_host(in, texels.data(), recv.data(), count, count, err)) return bad(err.c_str());
            for (uint64_t i = 0; i < count; ++i) {
                if (i && texels[i] <= texels[i - 1]) return bad("texels are not ascending");
                for (float n : recv[i].normal) if (!std::isfinite(n)) return bad("a normal is not finite");
                irr[i] = PTIrradiance{{rnd(), rnd(), rnd()}, rnd()};
            }
            if (pass && count == 0) return bad("the soup covers nothing");
            for (uint32_t dilate : {0u, 1u, 16u}) {
                std::vector<float> image((size_t)W * H * 4);
                if (!chart_resolve_host(texels.data(), irr.data(), count, W, H, dilate, image.data(), err)) return bad(err.c_str());
                uint64_t ones = 0;
                for (size_t k = 0; k < (size_t)W * H; ++k) ones += image[4 * k + 3] == 1.0f;
                if (ones != count) return bad("the scatter lost or invented a texel");
            }
            std::vector<float> image((size_t)W * H * 4);
            if (count) {
                texels[count - 1] = W * H;
                if (chart_resolve_host(texels.data(), irr.data(), count, W, H, 1, image.data(), err)) return bad("an index past the image was not refused");
            }
            if (chart_resolve_host(texels.data(), irr.data(), 0, W, H, 17, image.data(), err)) return bad("dilate 17 was not refused");
        }
        // a primIdx the BLAS cannot have
        const uint32_t big = T;
        std::memcpy(&tris[2].w, &big, 4);
        const ChartInput in = {tris.data(), attrs.data(), nullptr, nullptr, nullptr, T, W, H, 0u};
        uint64_t count = 0;
        if (chart_rasterize_host(in, nullptr, nullptr, 0, count, err)) return bad("a primIdx >= triangleCount was not refused");
        const ChartInput zero = {tris.data(), attrs.data(), nullptr, nullptr, nullptr, T, 0, H, 0u};
        if (chart_rasterize_host(zero, nullptr, nullptr, 0, count, err)) return bad("width 0 was not refused");
    }
    std::printf("lightmap ok\n");
    return 0;
}
