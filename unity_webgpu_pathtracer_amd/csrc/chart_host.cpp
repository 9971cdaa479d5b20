// chart_host.cpp — the host twin of the lightmap kernels (include/ptmi_plugin.h Part 14): the rule of chart_rule.h
// in plain loops, texel by texel.  No GPU involved.
#include "chart_rule.h"

#include <cstring>
#include <vector>

namespace ptchart {

namespace {

// the UVs of primitive p: the caller's, or the attribute record's
void prim_uvs(const ChartInput& in, uint32_t p, float uv[6])
{
    if (in.uvs) { memcpy(uv, in.uvs + (size_t)p * 6u, 6 * sizeof(float)); return; }
    const PTTriangleAttributes& a = in.attrs[p];
    uv[0] = a.uv0[0]; uv[1] = a.uv0[1]; uv[2] = a.uv1[0]; uv[3] = a.uv1[1]; uv[4] = a.uv2[0]; uv[5] = a.uv2[1];
}

struct Record {
    float v0[3], e1[3], e2[3];
    uint32_t prim;
};

Record read_record(const PTFloat4* tris, uint32_t t)
{
    const PTFloat4 &r0 = tris[(size_t)t * 3u], &r1 = tris[(size_t)t * 3u + 1u], &r2 = tris[(size_t)t * 3u + 2u];
    Record r = {{r2.x, r2.y, r2.z}, {r1.x, r1.y, r1.z}, {r0.x, r0.y, r0.z}, 0u};
    memcpy(&r.prim, &r2.w, 4);
    return r;
}

} // namespace

bool chart_rasterize_host(const ChartInput& in, uint32_t* texels, PTReceiver* recv, uint64_t capacity, uint64_t& count, std::string& err)
{
    count = 0;
    if (!in.tris || !in.attrs) { err = "tris / attrs == NULL"; return false; }
    if ((in.l2w == nullptr) != (in.w2l == nullptr)) { err = "localToWorld and worldToLocal come together"; return false; }
    if (in.width < 1u || in.width > kMaxSize || in.height < 1u || in.height > kMaxSize) { err = "width / height outside 1 ... 8192"; return false; }
    if ((texels == nullptr) != (recv == nullptr)) { err = "texels and receivers come together (both NULL: only the count)"; return false; }
    const size_t n = (size_t)in.width * in.height;
    std::vector<uint32_t> owner(n, kNoOwner), recOf(in.triCount, 0u);
    for (uint32_t t = 0; t < in.triCount; ++t) {
        const Record r = read_record(in.tris, t);
        if (r.prim >= in.triCount) { err = "record " + std::to_string(t) + ": primIdx " + std::to_string(r.prim) + " >= triangleCount"; return false; }
        recOf[r.prim] = t;
        float uv[6], g[3];
        Snapped s;
        prim_uvs(in, r.prim, uv);
        if (!chart_setup(uv, in.width, in.height, s) || !chart_geometric_normal(r.e1, r.e2, g)) continue;
        int32_t x0, y0, x1, y1;
        if (!chart_bounds(s, in.width, in.height, x0, y0, x1, y1)) continue;
        for (int32_t y = y0; y <= y1; ++y)
            for (int32_t x = x0; x <= x1; ++x) {
                uint32_t& o = owner[(size_t)y * in.width + (size_t)x];
                if (r.prim < o && chart_covers(s, (uint32_t)x, (uint32_t)y)) o = r.prim;
            }
    }
    for (size_t i = 0; i < n; ++i) count += owner[i] != kNoOwner;
    if (!texels) return true;
    if (count > capacity) { err = "the chart covers " + std::to_string(count) + " texels, the arrays hold " + std::to_string(capacity); return false; }
    uint64_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t p = owner[i];
        if (p == kNoOwner) continue;
        const Record r = read_record(in.tris, recOf[p]);
        const PTTriangleAttributes& a = in.attrs[p];
        float uv[6];
        Snapped s;
        prim_uvs(in, p, uv);
        (void)chart_setup(uv, in.width, in.height, s);
        texels[k] = (uint32_t)i;
        chart_receiver(s, (uint32_t)(i % in.width), (uint32_t)(i / in.width), r.v0, r.e1, r.e2, a.normal0, a.normal1, a.normal2, in.l2w, in.w2l,
                       in.seedBase + (uint32_t)i, recv[k]);
        ++k;
    }
    return true;
}

bool chart_resolve_host(const uint32_t* texels, const PTIrradiance* irr, uint64_t count, uint32_t width, uint32_t height, uint32_t dilate, float* image,
                        std::string& err)
{
    if (!image || (count && (!texels || !irr))) { err = "texels / irradiance / image == NULL"; return false; }
    if (width < 1u || width > kMaxSize || height < 1u || height > kMaxSize) { err = "width / height outside 1 ... 8192"; return false; }
    if (dilate > kMaxDilate) { err = "dilate (" + std::to_string(dilate) + ") > 16"; return false; }
    const size_t n = (size_t)width * height;
    for (uint64_t i = 0; i < count; ++i)
        if (texels[i] >= n) { err = "texels[" + std::to_string(i) + "] = " + std::to_string(texels[i]) + " >= width * height"; return false; }
    std::vector<float> a(n * 4u, 0.0f), b(dilate ? n * 4u : 0u);
    for (uint64_t i = 0; i < count; ++i) {
        float* px = &a[(size_t)texels[i] * 4u];
        px[0] = irr[i].rgb[0]; px[1] = irr[i].rgb[1]; px[2] = irr[i].rgb[2]; px[3] = 1.0f;
    }
    static const int kDy[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, kDx[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
    for (uint32_t pass = 0; pass < dilate; ++pass) {
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                float nb[8][4] = {};
                uint32_t inside = 0;
                for (int k = 0; k < 8; ++k) {
                    const int64_t yy = (int64_t)y + kDy[k], xx = (int64_t)x + kDx[k];
                    if (yy < 0 || xx < 0 || yy >= (int64_t)height || xx >= (int64_t)width) continue;
                    inside |= 1u << k;
                    memcpy(nb[k], &a[((size_t)yy * width + (size_t)xx) * 4u], 16);
                }
                chart_dilate(&a[((size_t)y * width + x) * 4u], nb, inside, &b[((size_t)y * width + x) * 4u]);
            }
        a.swap(b);
    }
    memcpy(image, a.data(), n * 16u);
    return true;
}

} // namespace ptchart
