// shade_sanitize_main.cpp — the host twins of baked-light shading (shade_host.cpp) under AddressSanitizer + UBSan, stand-alone:
// `make shade-sanitize` builds and runs it.  It walks the shapes tests/test_shade_baked.py uses -- the table at every res, 4,096
// term cases with a back-facing normal, directions of other lengths, the metallic and roughness limits and a miss, the probe sets
// (none, one, five, boxes that hold none, all or some of the points, a tie), the table's corners and edges in the compose step --
// with every array allocated at its exact size, so that a read or write past an end is reported.  No GPU involved.
#include "shade_rule.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

uint32_t g_state = 0x1234567u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int fail(const char* what, const std::string& err)
{
    std::fprintf(stderr, "shade-sanitize: %s: %s\n", what, err.c_str());
    return 1;
}

} // namespace

int main()
{
    std::string err;
    // 1. the table at every res; a bad res is refused
    std::vector<PTShadeDFG> table[3];
    const uint32_t sizes[3] = {16u, 32u, 64u};
    for (int k = 0; k < 3; ++k) {
        table[k].resize((size_t)sizes[k] * sizes[k]);
        if (!ptshade::bake_dfg_host(sizes[k], table[k].data(), err)) return fail("bake_dfg_host", err);
        for (const PTShadeDFG& e : table[k])
            if (!(e.a + e.b > 0.0f && e.a + e.b <= 1.1f)) return fail("bake_dfg_host", "A + B out of range");
    }
    if (ptshade::bake_dfg_host(8u, table[0].data(), err) || ptshade::bake_dfg_host(16u, nullptr, err)) return fail("bake_dfg_host", "accepted bad arguments");

    // 2. terms
    const uint64_t n = 4096;
    std::vector<PTShadeMaterial> M(n);
    std::vector<PTRay> rays(n);
    std::vector<PTRaySurface> S(n);
    for (uint64_t i = 0; i < n; ++i) {
        PTShadeMaterial& m = M[i];
        for (int c = 0; c < 3; ++c) { m.baseColor[c] = rnd(); m.emission[c] = i % 5 ? 0.0f : rnd(); }
        m.metallic = i % 7 == 0 ? 0.0f : i % 7 == 1 ? 1.0f : rnd();
        m.roughness = i % 11 == 0 ? 0.001f : i % 11 == 1 ? 1.0f : std::fmax(rnd() * rnd(), 0.001f);
        m.occlusion = rnd();
        m.opacity = 1.0f;
        m.materialIndex = (uint32_t)(i % 8);
        m.flags = i % 97 == 9 ? PT_SHADE_MISS : 0u;
        const float scale = i % 13 == 2 ? 4.0f : i % 13 == 3 ? 0.25f : 1.0f;
        for (int a = 0; a < 3; ++a) {
            rays[i].origin[a] = rnd() * 2.0f - 1.0f;
            rays[i].direction[a] = (rnd() * 2.0f - 1.0f) * scale;
            S[i].position[a] = rnd() * 2.0f - 1.0f;
            S[i].normal[a] = rnd() * 2.0f - 1.0f;               // about half face away
        }
        rays[i].tmax = 1e30f;
        rays[i].reserved = 0u;
        S[i].t = rnd();
        S[i].materialIndex = (int32_t)m.materialIndex;
        S[i].uv[0] = rnd(); S[i].uv[1] = rnd();
        S[i].instance = 0xFFFFFFFFu;
        S[i].prim = (uint32_t)i;
    }
    const float five[5][3] = {{-0.5f, -0.5f, 0.0f}, {0.5f, -0.5f, 0.0f}, {0.0f, 0.5f, 0.5f}, {0.0f, 0.0f, -0.75f}, {0.5f, 0.5f, 0.5f}};
    struct Set { uint32_t count; bool tie; int boxes; };      // boxes: 0 none given, 1 hold no point, 2 hold all, 3 overlap
    const Set sets[] = {{0u, false, 0}, {1u, false, 0}, {5u, false, 0}, {5u, false, 1}, {5u, false, 2}, {5u, false, 3}, {3u, true, 0}, {3u, true, 2}};
    std::vector<PTShadeTerms> T(n);
    std::vector<PTReceiver> recv(n);
    std::vector<PTReflectionQuery> qr(n);
    for (const Set& s : sets) {
        std::vector<PTProbe> probes(s.count);
        std::vector<PTReflectionBox> boxes(s.boxes ? s.count : 0u);
        for (uint32_t k = 0; k < s.count; ++k) {
            for (int a = 0; a < 3; ++a) probes[k].position[a] = s.tie ? (a == 0 ? (k == 1u ? -0.25f : 0.25f) : 0.0f) : five[k][a];
            probes[k].seed = k;
            if (!s.boxes) continue;
            for (int a = 0; a < 3; ++a) {
                const float p = probes[k].position[a];
                boxes[k].bmin[a] = s.boxes == 1 ? p + 5.0f : s.boxes == 2 ? -2.0f : p - 0.75f;
                boxes[k].bmax[a] = s.boxes == 1 ? p + 6.0f : s.boxes == 2 ? 2.0f : p + 0.75f;
            }
            boxes[k].pad0 = boxes[k].pad1 = 0.0f;
        }
        if (!ptshade::terms_host(M.data(), rays.data(), S.data(), n, s.count ? probes.data() : nullptr, s.boxes ? boxes.data() : nullptr, s.count, T.data(),
                                 recv.data(), qr.data(), err))
            return fail("terms_host", err);
        for (uint64_t i = 0; i < n; ++i) {
            const bool miss = (M[i].flags & PT_SHADE_MISS) != 0u;
            if (miss != (qr[i].probe == 0xFFFFFFFFu && T[i].nDotV == 0.0f) && s.count) return fail("terms_host", "a miss is not marked");
            if (!miss && s.count && qr[i].probe >= s.count) return fail("terms_host", "probe out of range");
            if (!miss && s.tie && qr[i].probe == 2u) return fail("terms_host", "a tie went to the higher index");
            if (!miss && !(T[i].nDotV >= 1e-4f)) return fail("terms_host", "nDotV below its floor");
        }
        // outputs are optional
        if (!ptshade::terms_host(M.data(), rays.data(), S.data(), n, s.count ? probes.data() : nullptr, s.boxes ? boxes.data() : nullptr, s.count, nullptr,
                                 nullptr, nullptr, err))
            return fail("terms_host (no outputs)", err);
    }
    PTReflectionBox box = {};
    if (ptshade::terms_host(M.data(), rays.data(), S.data(), n, nullptr, &box, 0u, T.data(), nullptr, nullptr, err)) return fail("terms_host", "accepted boxes without probes");
    if (!ptshade::terms_host(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0u, nullptr, nullptr, nullptr, err)) return fail("terms_host (count 0)", err);

    // 3. compose: the table's corners and edges, a constant table, a miss
    for (int k = 0; k < 3; ++k) {
        const uint32_t res = sizes[k];
        const float c[8] = {0.0f, 1e-4f, 0.5f / (float)res, 1.0f / (float)res, 0.37f, 1.0f - 1.0f / (float)res, 1.0f - 0.5f / (float)res, 1.0f};
        std::vector<PTShadeTerms> terms;
        for (float nv : c)
            for (float rho : c) {
                PTShadeTerms t = {};
                for (int ch = 0; ch < 3; ++ch) { t.diffuse[ch] = rnd(); t.f0[ch] = rnd(); t.emission[ch] = rnd(); }
                t.rho = rho; t.nDotV = nv; t.occlusion = rnd();
                terms.push_back(t);
            }
        const uint64_t m = terms.size();
        std::vector<PTIrradiance> E(m);
        std::vector<PTReflectionTexel> R(m);
        for (uint64_t i = 0; i < m; ++i)
            for (int ch = 0; ch < 3; ++ch) { E[i].rgb[ch] = rnd() * 4.0f; R[i].rgb[ch] = rnd() * 4.0f; }
        std::vector<float> out(4 * m);
        if (!ptshade::compose_host(terms.data(), E.data(), R.data(), m, table[k].data(), res, out.data(), err)) return fail("compose_host", err);
        for (uint64_t i = 0; i < m; ++i)
            if ((out[4 * i + 3] == 1.0f) != (terms[i].nDotV > 0.0f)) return fail("compose_host", "alpha does not mark the hits");
        std::vector<PTShadeDFG> flat((size_t)res * res, PTShadeDFG{0.625f, 0.125f});
        if (!ptshade::compose_host(terms.data(), E.data(), R.data(), m, flat.data(), res, out.data(), err)) return fail("compose_host (constant table)", err);
        for (uint64_t i = 0; i < m; ++i) {
            if (!(terms[i].nDotV > 0.0f)) continue;
            const float want = terms[i].emission[0] + terms[i].occlusion * ((terms[i].diffuse[0] * E[i].rgb[0]) * ptshade::kInvPi + R[i].rgb[0] * (terms[i].f0[0] * 0.625f + 0.125f));
            if (out[4 * i] != want) return fail("compose_host", "a constant table did not come back exactly");
        }
        if (ptshade::compose_host(terms.data(), E.data(), R.data(), m, table[k].data(), res + 1u, out.data(), err)) return fail("compose_host", "accepted a bad res");
    }
    std::printf("shade ok\n");
    return 0;
}
