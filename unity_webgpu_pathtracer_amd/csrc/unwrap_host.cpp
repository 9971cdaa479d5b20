// unwrap_host.cpp — the unwrap rule on the host (unwrap_rule.h; include/ptmi_plugin.h Part 23): the twin of
// pt_unwrap.hip, and the shelf packer, which has no device form.  No GPU involved.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>
#include "unwrap_rule.h"

namespace ptunwrap {

namespace {

struct Corner { uint32_t x, y, z; };
inline bool operator<(const Corner& a, const Corner& b) { return a.x != b.x ? a.x < b.x : a.y != b.y ? a.y < b.y : a.z < b.z; }
inline bool operator==(const Corner& a, const Corner& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// corners[p] and cls[p] of every primitive, + 0.0f applied.  false: a record's primIdx is not below triCount
bool load_corners(const PTFloat4* tris, const PTFloat4* vertices, uint32_t T, std::vector<float>& corners, std::vector<uint32_t>& cls, std::string& err)
{
    corners.assign((size_t)T * 9u, 0.0f);
    cls.assign(T, kExcluded);
    std::vector<uint8_t> seen(vertices ? 0u : T, 0);
    for (uint32_t t = 0; t < T; ++t) {
        float c[3][3];
        uint32_t p = t;
        if (vertices) {
            for (int k = 0; k < 3; ++k) { c[k][0] = vertices[3u * t + k].x; c[k][1] = vertices[3u * t + k].y; c[k][2] = vertices[3u * t + k].z; }
        } else {
            const PTFloat4 &e2 = tris[3u * (size_t)t], &e1 = tris[3u * (size_t)t + 1u], &v0 = tris[3u * (size_t)t + 2u];
            std::memcpy(&p, &v0.w, 4);
            if (p >= T || seen[p]) { err = "a triangle record's primIdx is not a primitive of the BLAS, or appears twice"; return false; }
            seen[p] = 1;
            const float a0[3] = {v0.x, v0.y, v0.z}, a1[3] = {e1.x, e1.y, e1.z}, a2[3] = {e2.x, e2.y, e2.z};
            unwrap_record_corners(a0, a1, a2, c);
        }
        cls[p] = unwrap_class(c);
        std::memcpy(&corners[(size_t)p * 9u], c, sizeof(c));
    }
    return true;
}

uint32_t find_root(std::vector<uint32_t>& label, uint32_t x)
{
    uint32_t r = x;
    while (label[r] != r) r = label[r];
    while (label[x] != r) { const uint32_t n = label[x]; label[x] = r; x = n; }
    return r;
}

} // namespace

bool unwrap_charts_host(const PTFloat4* tris, const PTFloat4* vertices, uint32_t T, uint32_t* chartOfPrim, PTUnwrapChart* charts, uint32_t capacity,
                        uint32_t& count, PTUnwrapStats* stats, std::string& err)
{
    count = 0;
    if (!unwrap_check_count((int64_t)T, "PTUnwrapChartsHost", err)) return false;
    if (!tris && !vertices) { err = "PTUnwrapChartsHost: tris == NULL and vertices == NULL"; return false; }
    if ((chartOfPrim == nullptr) != (charts == nullptr)) { err = "PTUnwrapChartsHost: chartOfPrim and charts come together (both NULL: only the count)"; return false; }
    std::vector<float> corners;
    std::vector<uint32_t> cls;
    if (!load_corners(tris, vertices, T, corners, cls, err)) return false;
    // vertex identity: the rank of a corner's 96 bits among the distinct ones
    const size_t N = (size_t)T * 3u;
    std::vector<Corner> key(N);
    for (size_t i = 0; i < N; ++i) key[i] = Corner{unwrap_bits(corners[3 * i]), unwrap_bits(corners[3 * i + 1]), unwrap_bits(corners[3 * i + 2])};
    std::vector<uint32_t> order(N), vid(N);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    uint32_t id = 0;
    for (size_t j = 0; j < N; ++j) {
        if (j && !(key[order[j]] == key[order[j - 1]])) ++id;
        vid[order[j]] = id;
    }
    // edges of the included primitives, sorted; equal neighbours are linked
    const uint32_t idBits = unwrap_id_bits(N);
    std::vector<std::pair<uint64_t, uint32_t>> edges;
    edges.reserve(N);
    uint32_t excluded = 0;
    for (uint32_t p = 0; p < T; ++p) {
        if (cls[p] == kExcluded) { ++excluded; continue; }
        for (uint32_t k = 0; k < 3u; ++k) edges.emplace_back(unwrap_edge_key(vid[3u * p + k], vid[3u * p + (k + 1u) % 3u], cls[p], idBits), p);
    }
    std::sort(edges.begin(), edges.end());
    std::vector<uint32_t> label(T);
    std::iota(label.begin(), label.end(), 0u);
    uint32_t linked = 0;
    for (size_t j = 1; j < edges.size(); ++j)
        if (edges[j].first == edges[j - 1].first) {
            ++linked;
            const uint32_t a = find_root(label, edges[j].second), b = find_root(label, edges[j - 1].second);
            if (a != b) label[a > b ? a : b] = a > b ? b : a;          // the lower primIdx is the root: the label
        }
    std::vector<uint32_t> place(T, kNoChart), tri(T, 0u);
    uint32_t singles = 0;
    for (uint32_t p = 0; p < T; ++p)
        if (cls[p] != kExcluded) ++tri[find_root(label, p)];
    for (uint32_t p = 0; p < T; ++p)
        if (cls[p] != kExcluded && label[p] == p) { place[p] = count++; singles += tri[p] == 1u; }
    if (stats) { stats->excluded = excluded; stats->linkedEdges = linked; stats->singleCharts = singles; stats->sweeps = 0u; }
    if (!charts) return true;
    if (count > capacity) { err = "PTUnwrapChartsHost: the mesh has " + std::to_string(count) + " charts, the array holds " + std::to_string(capacity); return false; }
    for (uint32_t p = 0; p < T; ++p) {
        if (cls[p] == kExcluded) { chartOfPrim[p] = kNoChart; continue; }
        const uint32_t root = label[p], c = place[root];
        chartOfPrim[p] = c;
        PTUnwrapChart& ch = charts[c];
        const uint32_t a = cls[root] >> 1, ua = (a + 1u) % 3u, va = (a + 2u) % 3u;
        const float* q = &corners[(size_t)p * 9u];
        if (p == root) {                                                // the lowest primitive of the chart comes first
            ch.firstPrim = p; ch.cls = cls[p]; ch.triCount = tri[p]; ch.reserved = 0u;
            ch.umin = ch.umax = q[ua]; ch.vmin = ch.vmax = q[va];
        }
        for (int k = 0; k < 3; ++k) {
            const float u = q[3 * k + ua], v = q[3 * k + va];
            ch.umin = u < ch.umin ? u : ch.umin; ch.umax = u > ch.umax ? u : ch.umax;
            ch.vmin = v < ch.vmin ? v : ch.vmin; ch.vmax = v > ch.vmax ? v : ch.vmax;
        }
    }
    return true;
}

bool pack_charts_host(const PTUnwrapChart* charts, uint32_t n, uint32_t width, uint32_t height, uint32_t padding, float tpu, int32_t* origins,
                      uint32_t& rowsUsed, std::string& err)
{
    rowsUsed = 0;
    if (!unwrap_check_atlas(width, height, padding, tpu, "PTPackChartsHost", err)) return false;
    if (n && (!charts || !origins)) { err = "PTPackChartsHost: charts or origins == NULL"; return false; }
    std::vector<uint32_t> w(n), h(n), order(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (!unwrap_side(charts[i].umin, charts[i].umax, tpu, padding, w[i]) || !unwrap_side(charts[i].vmin, charts[i].vmax, tpu, padding, h[i]) || w[i] > width) {
            err = "PTPackChartsHost: chart " + std::to_string(i) + " is wider than the atlas at this density (or its size is not finite)";
            return false;
        }
    }
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (h[a] != h[b]) return h[a] > h[b];
        if (w[a] != w[b]) return w[a] > w[b];
        if (charts[a].firstPrim != charts[b].firstPrim) return charts[a].firstPrim < charts[b].firstPrim;
        return a < b;
    });
    // past the height the walk goes on, so that rowsUsed says what would fit (a y beyond 31 bits is clamped: it fits no atlas)
    uint32_t x = 0, shelf = 0;
    uint64_t y = 0;
    bool fits = true;
    for (uint32_t i : order) {
        if (x + w[i] > width) { y += shelf; x = 0; shelf = 0; }
        if (x == 0) shelf = h[i];
        if (y + h[i] > height) fits = false;
        origins[2u * i] = (int32_t)x; origins[2u * i + 1u] = (int32_t)(y < 0x7FFFFFFFull ? y : 0x7FFFFFFFull);
        x += w[i];
    }
    rowsUsed = (uint32_t)(y + shelf < 0xFFFFFFFFull ? y + shelf : 0xFFFFFFFFull);
    if (!fits) { err = "PTPackChartsHost: the charts need " + std::to_string(rowsUsed) + " rows, the atlas has " + std::to_string(height); return false; }
    return true;
}

bool emit_uvs_host(const PTFloat4* tris, const PTFloat4* vertices, uint32_t T, const uint32_t* chartOfPrim, const PTUnwrapChart* charts, const int32_t* origins,
                   uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float tpu, float* uvs, std::string& err)
{
    if (!unwrap_check_count((int64_t)T, "PTEmitChartUVsHost", err) || !unwrap_check_atlas(width, height, padding, tpu, "PTEmitChartUVsHost", err)) return false;
    if ((!tris && !vertices) || !chartOfPrim || !uvs || (chartCount && (!charts || !origins))) { err = "PTEmitChartUVsHost: a NULL array"; return false; }
    std::vector<float> corners;
    std::vector<uint32_t> cls;
    if (!load_corners(tris, vertices, T, corners, cls, err)) return false;
    for (uint32_t p = 0; p < T; ++p) {
        float uv[6];
        const uint32_t c = chartOfPrim[p];
        if (c < chartCount) {
            float q[3][3];
            std::memcpy(q, &corners[(size_t)p * 9u], sizeof(q));
            unwrap_uvs(q, charts[c], origins[2u * c], origins[2u * c + 1u], width, height, padding, tpu, uv);
        } else {
            for (float& v : uv) v = unwrap_float(kQuietNaN);
        }
        std::memcpy(uvs + (size_t)p * 6u, uv, sizeof(uv));
    }
    return true;
}

} // namespace ptunwrap
