// shade_host.cpp — the host twins of the baked-light shading kernels (include/ptmi_plugin.h Part 21): the rule of
// shade_rule.h in plain loops, and the argument checks the context's entry points share with them.  No GPU involved.
#include "shade_rule.h"

#include <cstring>

namespace ptshade {

bool check_dfg_res(uint32_t res, std::string& err)
{
    if (dfg_res_ok(res)) return true;
    err = "DFG res = " + std::to_string(res) + " is not 16, 32 or 64";
    return false;
}

bool bake_dfg_host(uint32_t res, PTShadeDFG* out, std::string& err)
{
    if (!check_dfg_res(res, err)) return false;
    if (!out) { err = "out == NULL"; return false; }
    for (uint32_t j = 0; j < res; ++j)
        for (uint32_t i = 0; i < res; ++i) {
            float a[64], b[64];
            for (uint32_t q = 0; q < 64u; ++q) dfg_lane(res, i, j, q, a[q], b[q]);
            out[j * res + i] = PTShadeDFG{dfg_scale(ptsh::fold(a)), dfg_scale(ptsh::fold(b))};
        }
    return true;
}

bool terms_host(const PTShadeMaterial* materials, const PTRay* rays, const PTRaySurface* surface, uint64_t count, const PTProbe* probes,
                const PTReflectionBox* boxes, uint32_t probeCount, PTShadeTerms* outTerms, PTReceiver* outReceivers, PTReflectionQuery* outQueries,
                std::string& err)
{
    if (count && (!materials || !rays || !surface)) { err = "materials / rays / surface == NULL"; return false; }
    if (probeCount && !probes) { err = "probes == NULL"; return false; }
    if (boxes && !probes) { err = "boxes without probes (the choice needs the probes' positions)"; return false; }
    for (uint64_t i = 0; i < count; ++i) {
        PTShadeTerms T;
        PTReceiver rc;
        PTReflectionQuery q;
        memset(&T, 0, sizeof(T));
        memset(&rc, 0, sizeof(rc));
        memset(&q, 0, sizeof(q));
        q.probe = kNoProbe;
        if (!(materials[i].flags & PT_SHADE_MISS)) {
            const PTRaySurface& S = surface[i];
            float N[3] = {S.normal[0], S.normal[1], S.normal[2]}, R[3];
            terms(materials[i], rays[i].direction, N, R, T);
            q.probe = choose_probe(S.position, probeCount, boxes != nullptr,
                                   [&](uint32_t k, float Q[3]) { for (uint32_t a = 0; a < 3u; ++a) Q[a] = probes[k].position[a]; },
                                   [&](uint32_t k, float bmin[3], float bmax[3]) { for (uint32_t a = 0; a < 3u; ++a) { bmin[a] = boxes[k].bmin[a]; bmax[a] = boxes[k].bmax[a]; } });
            q.roughness = T.rho;
            for (uint32_t a = 0; a < 3u; ++a) {
                rc.position[a] = q.position[a] = S.position[a];
                rc.normal[a] = N[a];
                q.direction[a] = R[a];
            }
        }
        if (outTerms) outTerms[i] = T;
        if (outReceivers) outReceivers[i] = rc;
        if (outQueries) outQueries[i] = q;
    }
    return true;
}

bool compose_host(const PTShadeTerms* terms, const PTIrradiance* irradiance, const PTReflectionTexel* reflection, uint64_t count, const PTShadeDFG* dfg,
                  uint32_t dfgRes, float* out, std::string& err)
{
    if (!check_dfg_res(dfgRes, err)) return false;
    if (!dfg || (count && (!terms || !irradiance || !reflection || !out))) { err = "terms / irradiance / reflection / dfg / out == NULL"; return false; }
    for (uint64_t i = 0; i < count; ++i) {
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!is_miss(terms[i])) {
            float A, B;
            dfg_lookup(dfgRes, terms[i].nDotV, terms[i].rho, [&](uint32_t e, float ab[2]) { ab[0] = dfg[e].a; ab[1] = dfg[e].b; }, A, B);
            compose(terms[i], irradiance[i].rgb, reflection[i].rgb, A, B, o);
        }
        for (uint32_t c = 0; c < 4u; ++c) out[4u * i + c] = o[c];
    }
    return true;
}

} // namespace ptshade
