// skin_host.cpp — the host twin of the skinning kernels (include/ptmi_plugin.h Part 11): PTSetSkin's checks and
// the rule of skin_rule.h in plain loops.  No GPU involved.
#include "skin_rule.h"

#include <cmath>

namespace ptskin {

bool skin_check(const PTSkinDesc& d, uint32_t triCount, uint32_t materialCount, std::string& err)
{
    if (!d.restVertices || !d.joints || !d.weights) { err = "PTSkinDesc: restVertices / joints / weights == NULL"; return false; }
    if (d.jointCount < 1u || d.jointCount > PT_SKIN_MAX_JOINTS) {
        err = "PTSkinDesc.jointCount (" + std::to_string(d.jointCount) + ") is not in 1 ... " + std::to_string(PT_SKIN_MAX_JOINTS);
        return false;
    }
    const size_t n = (size_t)triCount * 3u;
    for (size_t i = 0; i < n; ++i) {
        const PTFloat4& v = d.restVertices[i];
        if (!std::isfinite(v.x) || !std::isfinite(v.y) || !std::isfinite(v.z)) { err = "rest vertex " + std::to_string(i) + " is not finite"; return false; }
        for (int k = 0; k < 4; ++k) {
            if (d.joints[4 * i + k] >= d.jointCount) {
                err = "vertex " + std::to_string(i) + ": joint index " + std::to_string(d.joints[4 * i + k]) + " >= jointCount (" + std::to_string(d.jointCount) + ")";
                return false;
            }
            if (!std::isfinite(d.weights[4 * i + k])) { err = "vertex " + std::to_string(i) + ": weight " + std::to_string(k) + " is not finite"; return false; }
        }
    }
    for (uint32_t t = 0; d.restAttrs && materialCount != 0xFFFFFFFFu && t < triCount; ++t)
        if (d.restAttrs[t].materialIndex >= materialCount) {
            err = "triangle " + std::to_string(t) + ": materialIndex " + std::to_string(d.restAttrs[t].materialIndex) + " >= materialCount";
            return false;
        }
    return true;
}

bool skin_check_palette(const float* matrices, uint32_t jointCount, std::string& err)
{
    for (size_t i = 0; i < (size_t)jointCount * 12u; ++i)
        if (!std::isfinite(matrices[i])) { err = "joint matrix " + std::to_string(i / 12u) + " is not finite"; return false; }
    return true;
}

namespace {

void blend(const PTSkinDesc& d, const float* M, size_t i, float B[12])
{
    const uint16_t* j = d.joints + 4 * i;
    const float* w = d.weights + 4 * i;
    const float *m0 = M + 12u * j[0], *m1 = M + 12u * j[1], *m2 = M + 12u * j[2], *m3 = M + 12u * j[3];
    for (int e = 0; e < 12; ++e) B[e] = skin_blend(w[0], m0[e], w[1], m1[e], w[2], m2[e], w[3], m3[e]);
}

} // namespace

void skin_host(const PTSkinDesc& d, uint32_t triCount, const float* M, PTFloat4* outVerts, PTTriangleAttributes* outAttrs, float* outBounds)
{
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < (size_t)triCount * 3u; ++i) {
        float B[12], p[3];
        blend(d, M, i, B);
        const PTFloat4& v = d.restVertices[i];
        skin_point(B, v.x, v.y, v.z, p);
        outVerts[i] = PTFloat4{p[0], p[1], p[2], 0.0f};
        for (int a = 0; a < 3; ++a) { mn[a] = skin_min(mn[a], p[a]); mx[a] = skin_max(mx[a], p[a]); }
        if (outAttrs && d.restAttrs) {
            const size_t t = i / 3u, corner = i % 3u;
            if (corner == 0) outAttrs[t] = d.restAttrs[t];               // pads, uvs and materialIndex are the rest record's
            // a record as 8 rows of 4 floats: the corner's normal is row `corner`, its tangent row 3 + corner
            const float* rest = reinterpret_cast<const float*>(d.restAttrs + t);
            float* out = reinterpret_cast<float*>(outAttrs + t);
            const float *rn = rest + 4 * corner, *rt = rest + 12 + 4 * corner;
            skin_direction(B, rn[0], rn[1], rn[2], out + 4 * corner);
            skin_direction(B, rt[0], rt[1], rt[2], out + 12 + 4 * corner);
        }
    }
    if (outBounds)
        for (int a = 0; a < 3; ++a) { outBounds[a] = mn[a]; outBounds[3 + a] = mx[a]; }
}

} // namespace ptskin
