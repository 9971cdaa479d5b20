// direct_host.cpp — the host twins of the direct-light kernels (include/ptmi_plugin.h Part 24): the rule of
// direct_rule.h in plain loops, and the argument checks the context's entry points share with them.  No GPU involved.
#include "direct_rule.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ptdirect {

bool check_params(const PTDirectParams* p, std::string& err)
{
    if (!p) { err = "params == NULL"; return false; }
    if (p->structSize == 0u) { err = "PTDirectParams.structSize is not set (must be sizeof(PTDirectParams) of the host's header)"; return false; }
    if (p->structSize < sizeof(PTDirectParams) || p->structSize > 4096u) {
        err = "PTDirectParams.structSize = " + std::to_string(p->structSize) + " is not a size of this struct";
        return false;
    }
    if (!strata_ok(p->strata)) { err = "strata = " + std::to_string(p->strata) + " (1 ... " + std::to_string(PT_DIRECT_MAX_STRATA) + ")"; return false; }
    if (p->flags & ~PT_DIRECT_CENTERED) { err = "unknown flag bits " + std::to_string(p->flags); return false; }
    for (uint32_t r : p->reserved) if (r) { err = "PTDirectParams.reserved != 0"; return false; }
    if (!std::isfinite(p->minAlpha) || p->minAlpha < 0.0f) { err = "minAlpha = " + std::to_string(p->minAlpha) + " is not finite and >= 0"; return false; }
    return true;
}

namespace {

Light light_of(const void* lights, uint32_t l)
{
    PTLight r;
    memcpy(&r, (const char*)lights + (size_t)l * sizeof(PTLight), sizeof(r));
    Light o;
    for (uint32_t a = 0; a < 3u; ++a) { o.position[a] = r.position[a]; o.emission[a] = r.emission[a]; o.u[a] = r.u[a]; o.v[a] = r.v[a]; }
    o.type = r.type; o.range = r.range; o.area = r.area;
    derive_rows(o);
    return o;
}

} // namespace

bool pair_count_host(const void* lights, uint32_t lightCount, uint32_t strata, uint32_t* outPairsPerEntry, std::string& err)
{
    if (!outPairsPerEntry) { err = "outPairsPerEntry == NULL"; return false; }
    *outPairsPerEntry = 0u;
    if (!strata_ok(strata)) { err = "strata = " + std::to_string(strata) + " (1 ... " + std::to_string(PT_DIRECT_MAX_STRATA) + ")"; return false; }
    if (lightCount && !lights) { err = "lights == NULL"; return false; }
    uint64_t pairs = 0;
    for (uint32_t l = 0; l < lightCount; ++l) pairs += pairs_of(light_of(lights, l).type, strata);
    if (pairs > 0xFFFFFFFFull) { err = "more than 2^32 - 1 pairs per entry"; return false; }
    *outPairsPerEntry = (uint32_t)pairs;
    return true;
}

bool rays_host(const PTDirectParams* p, const void* lights, uint32_t lightCount, const PTRay* rays, const PTShadeTerms* terms, const PTReceiver* receivers,
               uint64_t count, PTRay* outRays, float* outContrib, std::string& err)
{
    if (!check_params(p, err)) return false;
    uint32_t pairsPerEntry = 0;
    if (!pair_count_host(lights, lightCount, p->strata, &pairsPerEntry, err)) return false;
    if (count && (!rays || !terms || !receivers)) { err = "rays / terms / receivers == NULL"; return false; }
    if (count && pairsPerEntry && (!outRays || !outContrib)) { err = "outRays / outContrib == NULL"; return false; }
    std::vector<Light> L(lightCount);
    for (uint32_t l = 0; l < lightCount; ++l) L[l] = light_of(lights, l);
    const bool centred = (p->flags & PT_DIRECT_CENTERED) != 0u;
    for (uint64_t i = 0; i < count; ++i) {
        const bool miss = ptshade::is_miss(terms[i]);
        Entry e;
        if (!miss) entry_begin(terms[i], rays[i].direction, receivers[i].position, receivers[i].normal, p->minAlpha, e);
        uint32_t s = entry_state(p->seed, i);
        uint64_t pair = i * pairsPerEntry;
        for (uint32_t l = 0; l < lightCount; ++l) {
            const uint32_t n = pairs_of(L[l].type, p->strata);
            for (uint32_t k = 0; k < n; ++k, ++pair) {
                float x1 = 0.5f, x2 = 0.5f;
                if (!centred && L[l].type == PT_LIGHT_TYPE_RECTANGLE) {
                    x1 = pt_random_float(&s);
                    x2 = pt_random_float(&s);
                }
                float dir[3] = {0.0f, 0.0f, 0.0f}, c[3] = {0.0f, 0.0f, 0.0f};
                const bool counts = !miss && pair_eval(e, L[l], p->strata, k, x1, x2, dir, c);
                PTRay& r = outRays[pair];
                for (uint32_t a = 0; a < 3u; ++a) {
                    r.origin[a] = counts ? e.O[a] : 0.0f;
                    r.direction[a] = dir[a];
                    outContrib[4u * pair + a] = c[a];
                }
                r.tmax = counts ? PT_FAR_PLANE : 0.0f;
                r.reserved = 0u;
                outContrib[4u * pair + 3u] = 0.0f;
            }
        }
    }
    return true;
}

bool accumulate_host(const PTShadeTerms* terms, const float* contrib, const PTRayHit* pairHits, uint64_t count, uint32_t pairsPerEntry, float* out,
                     std::string& err)
{
    if (count && (!terms || !out)) { err = "terms / out == NULL"; return false; }
    if (count && pairsPerEntry && (!contrib || !pairHits)) { err = "contrib / pairHits == NULL"; return false; }
    for (uint64_t i = 0; i < count; ++i) {
        float* o = out + 4u * i;
        if (ptshade::is_miss(terms[i])) {
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            continue;
        }
        float d[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t k = 0; k < pairsPerEntry; ++k) {
            const uint64_t pair = i * pairsPerEntry + k;
            const float* c = contrib + 4u * pair;
            // a pair that does not count has zero contribution: adding it would leave the bits, but it is not added
            if (pairHits[pair].prim != 0xFFFFFFFFu || !(c[0] > 0.0f || c[1] > 0.0f || c[2] > 0.0f)) continue;
            for (uint32_t ch = 0; ch < 3u; ++ch) d[ch] = d[ch] + c[ch];
        }
        o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; o[3] = 1.0f;
    }
    return true;
}

} // namespace ptdirect
