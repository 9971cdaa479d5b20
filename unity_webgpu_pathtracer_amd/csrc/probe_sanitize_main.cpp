// probe_sanitize_main.cpp — the host twins of the probe kernels (probe_host.cpp) in a stand-alone program for
// `make probe-sanitize` (AddressSanitizer + UBSan, host code only, no GPU): makes directions into exactly sized heap arrays,
// projects constant and random radiance at sample counts on both sides of 64, evaluates with an index past the array, and makes
// the refusals.  Prints "probe ok" and returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sh_rule.h"

namespace {

uint32_t g_state = 777u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("probe-sanitize: %s\n", what); return 1; }

} // namespace

int main()
{
    using namespace ptsh;
    std::string err;
    const uint32_t counts[] = {1u, 63u, 64u, 70u, 4096u};
    for (uint32_t samples : counts) {
        const uint64_t n = 3;
        std::vector<PTProbe> probes(n);
        for (uint64_t i = 0; i < n; ++i) probes[i] = PTProbe{{rnd(), rnd(), rnd()}, 0xFFFFFFF0u + (uint32_t)i};
        std::vector<PTRadianceRay> rays(n * samples);
        if (!probe_directions_host(probes.data(), n, 0xFFFFFFFEu, samples, rays.data(), err)) return bad(err.c_str());
        std::vector<float> dirs(n * samples * 3), one(n * samples * 3, 1.0f), col(n * samples * 3);
        for (size_t s = 0; s < rays.size(); ++s) {
            const float* d = rays[s].direction;
            const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (!(std::fabs(len - 1.0f) < 1e-6f)) return bad("a direction is not of unit length");
            if (std::memcmp(rays[s].origin, probes[s / samples].position, 12) != 0 || rays[s].reserved != 0u) return bad("a ray's origin or reserved word is wrong");
            std::memcpy(&dirs[3 * s], d, 12);
            for (int c = 0; c < 3; ++c) col[3 * s + c] = rnd() * 4.0f;
        }
        // a split of the sample range gives the same samples
        if (samples > 1u) {
            std::vector<PTRadianceRay> tail(n * (samples - 1u));
            if (!probe_directions_host(probes.data(), n, 0xFFFFFFFFu, samples - 1u, tail.data(), err)) return bad(err.c_str());
            for (uint64_t i = 0; i < n; ++i)
                if (std::memcmp(&tail[i * (samples - 1u)], &rays[i * samples + 1u], (samples - 1u) * sizeof(PTRadianceRay)) != 0) return bad("a split range gives other samples");
        }
        std::vector<PTProbeCoeffs> sh(n), shc(n);
        if (!probe_project_host(dirs.data(), one.data(), n, samples, shc.data(), err)) return bad(err.c_str());
        if (!probe_project_host(dirs.data(), col.data(), n, samples, sh.data(), err)) return bad(err.c_str());
        for (uint64_t i = 0; i < n; ++i) {
            // constant radiance 1: sh[0] = 4 PI * Y0 whatever the directions, m2 = samples
            const float want = 12.566371f * 0.28209479f;
            for (int c = 0; c < 3; ++c)
                if (!(std::fabs(shc[i].sh[0][c] - want) <= want * ((float)samples / 64.0f + 6.0f) * 5.9604645e-8f)) return bad("band 0 of constant radiance is off");
            if (!(std::fabs(shc[i].m2 - (float)samples) <= (float)samples * 1e-5f)) return bad("m2 of constant radiance is off");
            for (int k = 0; k < 9; ++k) for (int c = 0; c < 3; ++c) if (!std::isfinite(sh[i].sh[k][c])) return bad("a coefficient is not finite");
        }
        // evaluation, with an index past the array and the largest index a query can carry
        std::vector<PTProbeQuery> q(5);
        for (size_t k = 0; k < q.size(); ++k) q[k] = PTProbeQuery{{0.0f, 0.6f, 0.8f}, (uint32_t)k};
        q[4].probe = 0xFFFFFFFFu;
        std::vector<PTIrradiance> E(q.size());
        if (!probe_irradiance_host(shc.data(), n, q.data(), q.size(), E.data(), err)) return bad(err.c_str());
        for (size_t k = 0; k < q.size(); ++k) {
            if (E[k].m2 != 0.0f) return bad("an evaluation's m2 is not 0");
            if (k >= n && (E[k].rgb[0] != 0.0f || E[k].rgb[1] != 0.0f || E[k].rgb[2] != 0.0f)) return bad("a probe index out of range does not give zeros");
        }
        if (samples == 4096u && !(std::fabs(E[0].rgb[1] - 3.14159265f) < 0.35f)) return bad("constant radiance 1 does not give E near PI");
    }
    // refusals
    {
        PTProbe p = {{0, 0, 0}, 1u};
        PTRadianceRay r;
        PTProbeCoeffs o;
        float d[3] = {0, 0, 1}, c[3] = {1, 1, 1};
        if (probe_directions_host(&p, 1, 0, 0, &r, err)) return bad("samples 0 was not refused");
        if (probe_directions_host(&p, 1, 0, 65537u, &r, err)) return bad("samples 65537 was not refused");
        if (probe_directions_host(nullptr, 1, 0, 1, &r, err)) return bad("probes == NULL was not refused");
        if (probe_project_host(d, c, 1, 0, &o, err)) return bad("samples 0 was not refused");
        if (probe_project_host(nullptr, c, 1, 1, &o, err)) return bad("directions == NULL was not refused");
        if (probe_irradiance_host(nullptr, 1, nullptr, 1, nullptr, err)) return bad("NULL arrays were not refused");
        if (!probe_directions_host(nullptr, 0, 0, 1, nullptr, err)) return bad("count 0 was refused");
    }
    std::printf("probe ok\n");
    return 0;
}
