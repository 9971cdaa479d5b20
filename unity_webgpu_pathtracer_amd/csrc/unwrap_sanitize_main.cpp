// unwrap_sanitize_main.cpp — the host twins of the unwrap kernels and the shelf packer (unwrap_host.cpp) in a stand-alone program for
// `make unwrap-sanitize` (AddressSanitizer + UBSan, host code only, no GPU): a cube (6 charts), a permuted strip with excluded
// triangles in exactly sized heap arrays, both corner sources, the packer past the height, and the refusals.  Prints "unwrap ok" and
// returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "unwrap_rule.h"

namespace {

uint32_t g_state = 977u;
uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

int bad(const char* what) { std::printf("unwrap-sanitize: %s\n", what); return 1; }

// vertices (3 rows per primitive) -> records in reverse order, as a builder may leave them
std::vector<PTFloat4> records(const std::vector<PTFloat4>& v)
{
    const uint32_t T = (uint32_t)(v.size() / 3u);
    std::vector<PTFloat4> tris(v.size());
    for (uint32_t p = 0; p < T; ++p) {
        const uint32_t t = T - 1u - p;
        const PTFloat4 &a = v[3 * p], &b = v[3 * p + 1], &c = v[3 * p + 2];
        tris[3 * t] = PTFloat4{c.x - a.x, c.y - a.y, c.z - a.z, 0.0f};
        tris[3 * t + 1] = PTFloat4{b.x - a.x, b.y - a.y, b.z - a.z, 0.0f};
        tris[3 * t + 2] = PTFloat4{a.x, a.y, a.z, 0.0f};
        std::memcpy(&tris[3 * t + 2].w, &p, 4);
    }
    return tris;
}

void quad(std::vector<PTFloat4>& v, const float a[3], const float b[3], const float c[3], const float d[3])
{
    for (const float* q : {a, b, c, a, c, d}) v.push_back(PTFloat4{q[0], q[1], q[2], 0.0f});
}

} // namespace

int main()
{
    using namespace ptunwrap;
    std::string err;
    // ---- a cube of integer corners (the record form welds it too): 12 triangles, 6 charts of 2
    {
        std::vector<PTFloat4> v;
        const float P[8][3] = {{0, 0, 0}, {2, 0, 0}, {2, 2, 0}, {0, 2, 0}, {0, 0, 2}, {2, 0, 2}, {2, 2, 2}, {0, 2, 2}};
        const int F[6][4] = {{0, 3, 2, 1}, {4, 5, 6, 7}, {0, 1, 5, 4}, {2, 3, 7, 6}, {1, 2, 6, 5}, {0, 4, 7, 3}};
        for (const auto& f : F) quad(v, P[f[0]], P[f[1]], P[f[2]], P[f[3]]);
        const std::vector<PTFloat4> tris = records(v);
        for (int form = 0; form < 2; ++form) {
            uint32_t count = 0;
            PTUnwrapStats st;
            if (!unwrap_charts_host(tris.data(), form ? v.data() : nullptr, 12, nullptr, nullptr, 0, count, &st, err)) return bad(err.c_str());
            if (count != 6 || st.excluded != 0 || st.linkedEdges != 6 || st.singleCharts != 0) return bad("the cube is not 6 charts of 2");
            std::vector<uint32_t> of(12);
            std::vector<PTUnwrapChart> charts(count);
            uint32_t c2 = 0;
            if (unwrap_charts_host(tris.data(), form ? v.data() : nullptr, 12, of.data(), charts.data(), 5, c2, nullptr, err) || c2 != 6) return bad("a capacity of one less was not refused");
            if (!unwrap_charts_host(tris.data(), form ? v.data() : nullptr, 12, of.data(), charts.data(), 6, count, nullptr, err)) return bad(err.c_str());
            for (uint32_t p = 0; p < 12; ++p) if (of[p] != p / 2u) return bad("a cube face is in the wrong chart");
            std::vector<int32_t> origins(2 * count);
            uint32_t rows = 0;
            if (!pack_charts_host(charts.data(), count, 64, 64, 2, 8.0f, origins.data(), rows, err)) return bad(err.c_str());
            if (rows != 2u * (16u + 1u + 4u)) return bad("six 21 x 21 rectangles in 64 columns are two shelves");
            if (pack_charts_host(charts.data(), count, 64, 41, 2, 8.0f, origins.data(), rows, err) || rows != 42u) return bad("rows past the height were not refused with rowsUsed set");
            if (pack_charts_host(charts.data(), count, 20, 64, 2, 8.0f, origins.data(), rows, err) || rows != 0u) return bad("a chart wider than the atlas was not refused");
            if (!pack_charts_host(charts.data(), count, 64, 64, 2, 8.0f, origins.data(), rows, err)) return bad(err.c_str());
            std::vector<float> uvs(12 * 6);
            if (!emit_uvs_host(tris.data(), form ? v.data() : nullptr, 12, of.data(), charts.data(), origins.data(), count, 64, 64, 2, 8.0f, uvs.data(), err)) return bad(err.c_str());
            for (float u : uvs) if (!(u > 0.0f && u < 1.0f)) return bad("a cube UV is outside the atlas");
        }
    }
    // ---- a strip in the plane z = 1 whose primitives are a permutation, with a degenerate and a NaN triangle in it
    {
        const uint32_t T = 302;
        std::vector<uint32_t> perm(T);
        for (uint32_t i = 0; i < T; ++i) perm[i] = i;
        for (uint32_t i = T - 1; i > 0; --i) std::swap(perm[i], perm[rnd() % (i + 1u)]);
        std::vector<PTFloat4> v(3 * T);
        for (uint32_t i = 0; i < T; ++i) {
            // triangle i of the strip over the columns i / 2, i / 2 + 1
            const float x = (float)(i / 2u);
            const float a[3] = {x, 0, 1}, b[3] = {x + 1, 0, 1}, c[3] = {x + 1, 1, 1}, d[3] = {x, 1, 1};
            const float* q[3] = {a, (i & 1u) ? c : b, (i & 1u) ? d : c};
            for (int k = 0; k < 3; ++k) v[3 * perm[i] + k] = PTFloat4{q[k][0], q[k][1], q[k][2], 0.0f};
        }
        // cut the strip twice: three charts remain
        v[3 * perm[100] + 1] = v[3 * perm[100]];
        v[3 * perm[200] + 2].y = std::numeric_limits<float>::quiet_NaN();
        const std::vector<PTFloat4> tris = records(v);
        for (int form = 0; form < 2; ++form) {
            uint32_t count = 0;
            PTUnwrapStats st;
            std::vector<uint32_t> of(T);
            std::vector<PTUnwrapChart> charts(3);
            if (!unwrap_charts_host(tris.data(), form ? v.data() : nullptr, T, of.data(), charts.data(), 3, count, &st, err)) return bad(err.c_str());
            if (count != 3 || st.excluded != 2) return bad("the cut strip is not three charts");
            if (of[perm[100]] != kNoChart || of[perm[200]] != kNoChart) return bad("an excluded triangle has a chart");
            uint32_t tri = 0;
            for (const PTUnwrapChart& ch : charts) { tri += ch.triCount; if (ch.cls != 4u || ch.vmin != 0.0f || ch.vmax != 1.0f) return bad("a strip chart record is wrong"); }
            if (tri != T - 2u) return bad("the strip charts do not hold every included triangle");
            std::vector<int32_t> origins(6);
            uint32_t rows = 0;
            if (!pack_charts_host(charts.data(), 3, 1024, 64, 0, 4.0f, origins.data(), rows, err)) return bad(err.c_str());
            std::vector<float> uvs((size_t)T * 6);
            if (!emit_uvs_host(tris.data(), form ? v.data() : nullptr, T, of.data(), charts.data(), origins.data(), 3, 1024, 64, 0, 4.0f, uvs.data(), err)) return bad(err.c_str());
            for (int k = 0; k < 6; ++k) if (!std::isnan(uvs[6 * perm[100] + k])) return bad("an excluded triangle has UVs");
        }
    }
    // ---- refusals
    {
        uint32_t count = 0, rows = 0;
        const PTFloat4 one[3] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {0, 1, 0, 0}};
        if (unwrap_charts_host(nullptr, nullptr, 1, nullptr, nullptr, 0, count, nullptr, err)) return bad("no source was not refused");
        if (unwrap_charts_host(nullptr, one, 0, nullptr, nullptr, 0, count, nullptr, err)) return bad("T = 0 was not refused");
        if (unwrap_charts_host(nullptr, one, 357913942u, nullptr, nullptr, 0, count, nullptr, err)) return bad("a T beyond the edge key was not refused");
        uint32_t of = 0;
        if (unwrap_charts_host(nullptr, one, 1, &of, nullptr, 0, count, nullptr, err)) return bad("chartOfPrim without charts was not refused");
        PTUnwrapChart ch = {0, 4, 1, 0, 0.0f, 0.0f, 1.0f, 1.0f};
        int32_t o[2];
        for (float tpu : {0.0f, -1.0f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()})
            if (pack_charts_host(&ch, 1, 64, 64, 2, tpu, o, rows, err)) return bad("a bad density was not refused");
        if (pack_charts_host(&ch, 1, 0, 64, 2, 1.0f, o, rows, err) || pack_charts_host(&ch, 1, 64, 8193, 2, 1.0f, o, rows, err)) return bad("a bad size was not refused");
        if (pack_charts_host(&ch, 1, 64, 64, 17, 1.0f, o, rows, err)) return bad("padding 17 was not refused");
        if (!pack_charts_host(nullptr, 0, 64, 64, 2, 1.0f, nullptr, rows, err) || rows != 0) return bad("an empty list was refused");
        PTFloat4 rec[3] = {{0, 1, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0}};
        const uint32_t big = 1;
        std::memcpy(&rec[2].w, &big, 4);
        if (unwrap_charts_host(rec, nullptr, 1, nullptr, nullptr, 0, count, nullptr, err)) return bad("a primIdx >= triangleCount was not refused");
    }
    std::printf("unwrap ok\n");
    return 0;
}
