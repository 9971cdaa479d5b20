// lightmap_lookup_host.cpp — the host twin of the lightmap lookup (include/ptmi_plugin.h Part 22): the rule of
// lightmap_lookup_rule.h in a plain loop, and the check of a binding table that PTBindLightmaps shares with it.  No GPU involved.
#include "lightmap_lookup_rule.h"

#include <cstring>

namespace ptlm {

bool check_bindings(const PTLightmapBinding* bindings, uint32_t count, uint64_t attrCount, uint32_t instanceCount, std::string& err)
{
    if (count > PT_LIGHTMAP_MAX_BINDINGS) { err = "count = " + std::to_string(count) + " bindings (at most " + std::to_string(PT_LIGHTMAP_MAX_BINDINGS) + ")"; return false; }
    if (count && !bindings) { err = "bindings == NULL"; return false; }
    for (uint32_t k = 0; k < count; ++k) {
        const PTLightmapBinding& b = bindings[k];
        const std::string who = "binding " + std::to_string(k) + ": ";
        if (!b.dImage || ((uintptr_t)b.dImage & 15u)) { err = who + "image == NULL or not 16-byte aligned"; return false; }
        if ((uintptr_t)b.dUvs & 7u) { err = who + "uvs is not 8-byte aligned"; return false; }
        if (b.width == 0u || b.width > PT_CHART_MAX_SIZE || b.height == 0u || b.height > PT_CHART_MAX_SIZE) {
            err = who + "size " + std::to_string(b.width) + " x " + std::to_string(b.height) + " (1 ... " + std::to_string(PT_CHART_MAX_SIZE) + ")";
            return false;
        }
        if (b.primCount == 0u || (uint64_t)b.firstPrim + b.primCount > attrCount) {
            err = who + "span " + std::to_string(b.firstPrim) + " + " + std::to_string(b.primCount) + " is empty or past the scene's " + std::to_string(attrCount) + " attribute records";
            return false;
        }
        if (instanceCount != 0xFFFFFFFFu && b.instance != 0xFFFFFFFFu && b.instance >= instanceCount) {
            err = who + "instance " + std::to_string(b.instance) + " (the scene has " + std::to_string(instanceCount) + ")";
            return false;
        }
        if (b.flags & ~PT_LIGHTMAP_TWO_SIDED) { err = who + "unknown flag bits"; return false; }
        if (b.reserved[0] || b.reserved[1]) { err = who + "reserved words must be 0"; return false; }
    }
    return true;
}

bool lookup_host(const PTLightmapBinding* bindings, uint32_t bindingCount, const PTTriangleAttributes* attrs, uint64_t attrCount, uint32_t materialCount,
                 const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces, uint64_t count, PTIrradiance* out, uint32_t* outBinding,
                 std::string& err)
{
    if (!check_bindings(bindings, bindingCount, attrCount, 0xFFFFFFFFu, err)) return false;
    for (uint32_t k = 0; k < bindingCount; ++k)
        if (!bindings[k].dUvs && !attrs) { err = "binding " + std::to_string(k) + ": no uvs and attrs == NULL"; return false; }
    if (count && (!rays || !hits || !surfaces || !out)) { err = "rays / hits / surfaces / out == NULL"; return false; }
    for (uint64_t i = 0; i < count; ++i) {
        const PTRayHit& h = hits[i];
        // the surface record is written only where a hit was found
        const bool miss = h.prim == 0xFFFFFFFFu || (uint32_t)surfaces[i].materialIndex >= materialCount;
        const bool back = !miss && seen_from_behind(rays[i].direction, surfaces[i].normal);
        float E[4];
        const uint32_t k = lookup(miss, back, h.prim, h.u, h.v, miss ? 0u : surfaces[i].instance, bindingCount,
                                  [&](uint32_t b) { return bindings[b]; }, [](bool done) { return done; },
                                  [&](const Chosen& c, uint32_t prim, float uv[6]) {
                                      if (c.uvs) {
                                          memcpy(uv, c.uvs + 6u * (size_t)(prim - c.firstPrim), 6 * sizeof(float));
                                      } else {
                                          const PTTriangleAttributes& a = attrs[prim];
                                          uv[0] = a.uv0[0]; uv[1] = a.uv0[1]; uv[2] = a.uv1[0]; uv[3] = a.uv1[1]; uv[4] = a.uv2[0]; uv[5] = a.uv2[1];
                                      }
                                  },
                                  [](const Chosen& c, const uint32_t index[4], float t[4][4]) {
                                      for (uint32_t k = 0; k < 4u; ++k) memcpy(t[k], (const float*)c.image + 4u * (size_t)index[k], 16);
                                  },
                                  E);
        memcpy(&out[i], E, sizeof(PTIrradiance));
        if (outBinding) outBinding[i] = k;
    }
    return true;
}

} // namespace ptlm
