// light_grid_sanitize_main.cpp — the host twin of the light-grid build (light_grid_host.cpp) under AddressSanitizer + UBSan,
// stand-alone: `make light-grid-sanitize` builds and runs it.  It builds grids of several shapes -- one cell, a flat slab, the largest
// dims on one axis -- over a lattice of lights of every type with a NaN position, an infinite range and a zero emission among them,
// with every array allocated at its exact size, so that a read or write past an end is reported; it checks that every list is
// ascending, that the overflow cell lists every light and that a count-only call agrees with the full one.  No GPU involved.
#include "light_grid_rule.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

int fail(const char* what, const std::string& err)
{
    std::fprintf(stderr, "light-grid-sanitize: %s: %s\n", what, err.c_str());
    return 1;
}

PTLight make_light(uint32_t type, float x, float y, float z, float range)
{
    PTLight l = {};
    l.position[0] = x; l.position[1] = y; l.position[2] = z;
    l.type = type;
    l.emission[0] = 10.0f; l.emission[1] = 8.0f; l.emission[2] = 6.0f;
    l.range = range;
    if (type == PT_LIGHT_TYPE_RECTANGLE) {
        l.u[0] = 0.4f; l.v[2] = 0.4f;                           // normal = cross(u, v) = (0, -1, 0): faces down
        l.area = 0.16f;
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
    const uint32_t types[4] = {PT_LIGHT_TYPE_POINT, PT_LIGHT_TYPE_SPOT, PT_LIGHT_TYPE_RECTANGLE, PT_LIGHT_TYPE_DIRECTIONAL};
    std::vector<PTLight> lights;
    for (uint32_t k = 0; k < 40u; ++k) lights.push_back(make_light(types[k % 4u], (float)(k % 8u) + 0.5f, 1.2f, (float)(k / 8u) + 0.5f, 1.5f));
    lights[3].emission[0] = lights[3].emission[1] = lights[3].emission[2] = 0.0f;
    lights[4].position[0] = NAN;
    lights[5].range = INFINITY;
    lights.push_back(make_light(77u, 1.0f, 1.0f, 1.0f, 1.5f));                         // an unknown type
    const uint32_t shapes[][3] = {{1u, 1u, 1u}, {8u, 2u, 8u}, {256u, 1u, 3u}, {3u, 5u, 7u}};
    for (const auto& dims : shapes)
        for (uint32_t count : {0u, 1u, (uint32_t)lights.size()}) {
            PTLightGridParams p = {};
            p.structSize = sizeof(p);
            p.origin[0] = -0.25f; p.origin[1] = 0.0f; p.origin[2] = 0.125f;
            p.cellSize = dims[0] == 256u ? 0.03125f : 1.0f;
            for (int a = 0; a < 3; ++a) p.dims[a] = dims[a];
            const uint32_t cells = dims[0] * dims[1] * dims[2];
            std::vector<uint32_t> offsets((size_t)cells + 2u), rectBefore((size_t)count + 1u), counted((size_t)cells + 2u), rb2((size_t)count + 1u);
            uint64_t total = 0, total2 = 0;
            if (!ptlgrid::build_host(&p, count ? lights.data() : nullptr, count, counted.data(), nullptr, 0u, rb2.data(), &total, err)) return fail("count", err);
            std::vector<uint32_t> indices((size_t)total);
            if (!ptlgrid::build_host(&p, count ? lights.data() : nullptr, count, offsets.data(), indices.data(), total, rectBefore.data(), &total2, err))
                return fail("build", err);
            if (total != total2 || offsets != counted || rectBefore != rb2 || offsets[cells + 1u] != total) return fail("build", "the count-only call disagrees");
            for (uint32_t c = 0; c <= cells; ++c) {
                if (offsets[c] > offsets[c + 1u]) return fail("build", "offsets descend");
                for (uint32_t k = offsets[c]; k < offsets[c + 1u]; ++k) {
                    if (indices[k] >= count) return fail("build", "a light index past the lights");
                    if (k > offsets[c] && indices[k] <= indices[k - 1u]) return fail("build", "a list that does not ascend");
                }
            }
            if (offsets[cells + 1u] - offsets[cells] != count) return fail("build", "the overflow cell does not list every light");
            if (count > 5u) {
                bool nanListed = false, infListed = false;
                for (uint32_t k = offsets[0]; k < offsets[1]; ++k) {
                    nanListed = nanListed || indices[k] == 4u;
                    infListed = infListed || indices[k] == 5u;
                    if (indices[k] == 3u) return fail("build", "a light without emission is listed");
                }
                if (!nanListed) return fail("build", "the light with a NaN position is not listed");
                (void)infListed;                                // the spot with an infinite range may fall to its half-space
            }
            // a capacity below the total: the offsets and the total come back, the indices are left alone
            if (total > 1u) {
                std::vector<uint32_t> few((size_t)total - 1u, 0xABCDu);
                if (!ptlgrid::build_host(&p, lights.data(), count, counted.data(), few.data(), total - 1u, rb2.data(), &total2, err)) return fail("short", err);
                for (uint32_t v : few) if (v != 0xABCDu) return fail("short", "indices written although they do not fit");
                if (total2 != total) return fail("short", "the total differs");
            }
            // the cell rule: a point inside, on the far face (outside), a NaN
            ptlgrid::Grid g;
            for (int a = 0; a < 3; ++a) { g.origin[a] = p.origin[a]; g.dims[a] = p.dims[a]; }
            g.cellSize = p.cellSize;
            const float in[3] = {p.origin[0] + 0.5f * p.cellSize, p.origin[1] + 0.5f * p.cellSize, p.origin[2] + 0.5f * p.cellSize};
            const float face[3] = {p.origin[0] + p.cellSize * (float)dims[0], in[1], in[2]};
            const float bad[3] = {in[0], NAN, in[2]};
            if (ptlgrid::cell_of(g, in) != 0u || ptlgrid::cell_of(g, face) != cells || ptlgrid::cell_of(g, bad) != cells) return fail("cell_of", "wrong cell");
        }
    // refusals
    PTLightGridParams ok = {};
    ok.structSize = sizeof(ok); ok.cellSize = 1.0f; ok.dims[0] = ok.dims[1] = ok.dims[2] = 2u;
    if (!ptlgrid::check_params(&ok, err)) return fail("check_params", err);
    PTLightGridParams q = ok; q.dims[1] = 0u;
    if (ptlgrid::check_params(&q, err)) return fail("check_params", "accepted a dim of 0");
    q = ok; q.dims[2] = 257u;
    if (ptlgrid::check_params(&q, err)) return fail("check_params", "accepted a dim of 257");
    q = ok; q.dims[0] = q.dims[1] = q.dims[2] = 128u;
    if (ptlgrid::check_params(&q, err)) return fail("check_params", "accepted 2^21 cells");
    q = ok; q.cellSize = 0.0f;
    if (ptlgrid::check_params(&q, err)) return fail("check_params", "accepted a cell size of 0");
    q = ok; q.cellSize = INFINITY;
    if (ptlgrid::check_params(&q, err)) return fail("check_params", "accepted an infinite cell size");
    q = ok; q.cellSize = NAN;
    if (ptlgrid::check_params(&q, err)) return fail("check_params", "accepted a NaN cell size");
    q = ok; q.reserved = 1u;
    if (ptlgrid::check_params(&q, err)) return fail("check_params", "accepted a reserved word");
    q = ok; q.structSize = 0u;
    if (ptlgrid::check_params(&q, err) || ptlgrid::check_params(nullptr, err)) return fail("check_params", "accepted no structSize / NULL");
    uint32_t o[10], r[2];
    if (ptlgrid::build_host(&ok, nullptr, 1u, o, nullptr, 0u, r, nullptr, err) || ptlgrid::build_host(&ok, lights.data(), 1u, nullptr, nullptr, 0u, r, nullptr, err) ||
        ptlgrid::build_host(&ok, lights.data(), 1u, o, nullptr, 4u, r, nullptr, err))
        return fail("build_host", "accepted bad arguments");
    std::printf("light grid ok\n");
    return 0;
}
