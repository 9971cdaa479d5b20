// direct_sanitize_main.cpp — the host twins of the direct-light kernels (direct_host.cpp) under AddressSanitizer + UBSan,
// stand-alone: `make direct-sanitize` builds and runs it.  It walks the shapes tests/test_direct.py uses -- every light type alone
// and together with a directional one in between, S = 1 ... 4, centred and jittered, misses, back-facing lights, lights out of
// range, a NaN position -- with every array allocated at its exact size, so that a read or write past an end is reported.  No
// GPU involved.
#include "direct_rule.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

uint32_t g_state = 0x2468ACEu;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int fail(const char* what, const std::string& err)
{
    std::fprintf(stderr, "direct-sanitize: %s: %s\n", what, err.c_str());
    return 1;
}

PTLight make_light(uint32_t type, float x, float y, float z)
{
    PTLight l = {};
    l.position[0] = x; l.position[1] = y; l.position[2] = z;
    l.type = type;
    l.emission[0] = 10.0f; l.emission[1] = 8.0f; l.emission[2] = 6.0f;
    l.range = 20.0f;
    if (type == PT_LIGHT_TYPE_RECTANGLE) {
        l.u[0] = 1.0f; l.v[2] = 1.0f;                           // normal = cross(u, v) = (0, -1, 0): faces down
        l.area = 1.0f;
    } else {
        l.u[1] = -1.0f;                                         // a spot pointing down
        l.v[0] = 0.5f; l.v[1] = 0.8f;
    }
    return l;
}

} // namespace

int main()
{
    std::string err;
    const uint64_t n = 257;
    std::vector<PTRay> rays(n);
    std::vector<PTShadeTerms> T(n);
    std::vector<PTReceiver> R(n);
    for (uint64_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) {
            rays[i].origin[a] = rnd() * 2.0f - 1.0f;
            rays[i].direction[a] = rnd() * 2.0f - 1.0f;
            R[i].position[a] = rnd() * 2.0f - 1.0f;
            R[i].normal[a] = a == 1 ? 1.0f : 0.0f;
            T[i].diffuse[a] = rnd(); T[i].f0[a] = rnd(); T[i].emission[a] = 0.0f;
        }
        rays[i].direction[1] = -std::fabs(rays[i].direction[1]) - 0.1f;
        rays[i].tmax = PT_FAR_PLANE; rays[i].reserved = 0u;
        R[i].seed = 0u; R[i].reserved = 0u;
        T[i].rho = i % 9 == 0 ? 0.03f : rnd();
        T[i].nDotV = i % 7 == 3 ? 0.0f : std::fmax(rnd(), 1e-4f);     // every seventh entry is a miss
        T[i].occlusion = 1.0f;
        if (i == 5) R[i].position[0] = NAN;
    }
    const PTLight all[5] = {make_light(PT_LIGHT_TYPE_POINT, 0.0f, 3.0f, 0.0f), make_light(PT_LIGHT_TYPE_DIRECTIONAL, 0.0f, 3.0f, 0.0f),
                            make_light(PT_LIGHT_TYPE_RECTANGLE, -0.5f, 2.0f, -0.5f), make_light(PT_LIGHT_TYPE_SPOT, 0.3f, 4.0f, 0.2f),
                            make_light(PT_LIGHT_TYPE_RECTANGLE, -0.5f, -2.0f, -0.5f)};        // the last one shows its back
    struct Set { uint32_t first, count; };
    const Set sets[] = {{0u, 0u}, {0u, 1u}, {2u, 1u}, {3u, 1u}, {1u, 1u}, {0u, 5u}};
    for (const Set& s : sets)
        for (uint32_t strata = 1u; strata <= PT_DIRECT_MAX_STRATA; ++strata)
            for (uint32_t centred = 0u; centred < 2u; ++centred) {
                PTDirectParams p = {};
                p.structSize = sizeof(p); p.strata = strata; p.seed = 77u + strata; p.flags = centred ? PT_DIRECT_CENTERED : 0u;
                p.minAlpha = strata == 2u ? 0.2f : 0.0f;
                uint32_t pairs = 0;
                if (!ptdirect::pair_count_host(all + s.first, s.count, strata, &pairs, err)) return fail("pair_count_host", err);
                std::vector<PTRay> outRays((size_t)n * pairs);
                std::vector<float> contrib((size_t)n * pairs * 4u);
                if (!ptdirect::rays_host(&p, all + s.first, s.count, rays.data(), T.data(), R.data(), n, outRays.data(), contrib.data(), err))
                    return fail("rays_host", err);
                std::vector<PTRayHit> hits((size_t)n * pairs);
                for (size_t k = 0; k < hits.size(); ++k) {
                    const bool counts = outRays[k].tmax > 0.0f;
                    for (int c = 0; c < 4; ++c)
                        if (!std::isfinite(contrib[4 * k + c])) return fail("rays_host", "a contribution that is not finite");
                    if (!counts && (contrib[4 * k] != 0.0f || contrib[4 * k + 1] != 0.0f || contrib[4 * k + 2] != 0.0f))
                        return fail("rays_host", "a pair that does not count has a contribution");
                    hits[k] = PTRayHit{outRays[k].tmax, 0.0f, 0.0f, k % 3 == 1 ? 7u : 0xFFFFFFFFu};          // every third pair is occluded
                }
                std::vector<float> out((size_t)n * 4u);
                if (!ptdirect::accumulate_host(T.data(), contrib.data(), hits.data(), n, pairs, out.data(), err)) return fail("accumulate_host", err);
                for (uint64_t i = 0; i < n; ++i)
                    if ((out[4 * i + 3] == 1.0f) != (T[i].nDotV > 0.0f)) return fail("accumulate_host", "alpha does not mark the hits");
            }
    // refusals
    PTDirectParams ok = {};
    ok.structSize = sizeof(ok); ok.strata = 1u;
    uint32_t pairs = 0;
    PTDirectParams q = ok; q.strata = 0u;
    if (ptdirect::check_params(&q, err)) return fail("check_params", "accepted strata 0");
    q = ok; q.strata = PT_DIRECT_MAX_STRATA + 1u;
    if (ptdirect::check_params(&q, err)) return fail("check_params", "accepted strata above the maximum");
    q = ok; q.flags = 2u;
    if (ptdirect::check_params(&q, err)) return fail("check_params", "accepted an unknown flag");
    q = ok; q.reserved[2] = 1u;
    if (ptdirect::check_params(&q, err)) return fail("check_params", "accepted a reserved word");
    q = ok; q.minAlpha = -0.5f;
    if (ptdirect::check_params(&q, err)) return fail("check_params", "accepted a negative minAlpha");
    q = ok; q.minAlpha = NAN;
    if (ptdirect::check_params(&q, err)) return fail("check_params", "accepted a NaN minAlpha");
    q = ok; q.structSize = 0u;
    if (ptdirect::check_params(&q, err) || ptdirect::check_params(nullptr, err)) return fail("check_params", "accepted no structSize / NULL");
    if (ptdirect::pair_count_host(all, 5u, 5u, &pairs, err) || ptdirect::pair_count_host(nullptr, 5u, 1u, &pairs, err) ||
        ptdirect::pair_count_host(all, 5u, 1u, nullptr, err))
        return fail("pair_count_host", "accepted bad arguments");
    if (!ptdirect::rays_host(&ok, nullptr, 0u, nullptr, nullptr, nullptr, 0, nullptr, nullptr, err)) return fail("rays_host (count 0)", err);
    if (!ptdirect::accumulate_host(nullptr, nullptr, nullptr, 0, 3u, nullptr, err)) return fail("accumulate_host (count 0)", err);
    std::printf("direct ok\n");
    return 0;
}
