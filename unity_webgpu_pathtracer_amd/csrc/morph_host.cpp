// morph_host.cpp — the host twin of the morph kernels (include/ptmi_plugin.h Part 12): PTSetMorph's checks, the
// rule of morph_rule.h in plain loops, and the conversion of a CSR stream into the layout the kernels read.  No GPU involved.
#include "morph_rule.h"

#include <cmath>

namespace ptmorph {

namespace {

bool check_stream(const char* name, const uint32_t* off, const PTMorphEntry* ent, size_t corners, uint32_t targetCount, std::string& err)
{
    const std::string s = std::string(name) + " stream: ";
    if (off[0] != 0u) { err = s + "offsets[0] != 0"; return false; }
    for (size_t c = 0; c < corners; ++c)
        if (off[c + 1] < off[c]) { err = s + "offsets decrease at corner " + std::to_string(c); return false; }
    if (off[corners] && !ent) { err = s + "entries == NULL"; return false; }
    for (size_t c = 0; c < corners; ++c)
        for (uint32_t e = off[c]; e < off[c + 1]; ++e) {
            const PTMorphEntry& x = ent[e];
            if (x.target >= targetCount) {
                err = s + "corner " + std::to_string(c) + ": target " + std::to_string(x.target) + " >= targetCount (" + std::to_string(targetCount) + ")";
                return false;
            }
            if (e > off[c] && x.target <= ent[e - 1].target) { err = s + "corner " + std::to_string(c) + ": targets are not strictly ascending"; return false; }
            if (!std::isfinite(x.dx) || !std::isfinite(x.dy) || !std::isfinite(x.dz)) { err = s + "the delta of entry " + std::to_string(e) + " is not finite"; return false; }
        }
    return true;
}

// acc folded with the corner's listed entries, in order
void fold(const uint32_t* off, const PTMorphEntry* ent, size_t corner, const float* w, float acc[3])
{
    for (uint32_t e = off[corner]; e < off[corner + 1]; ++e) {
        const float wt = w[ent[e].target];
        acc[0] = morph_step(acc[0], wt, ent[e].dx);
        acc[1] = morph_step(acc[1], wt, ent[e].dy);
        acc[2] = morph_step(acc[2], wt, ent[e].dz);
    }
}

void blend(const PTSkinDesc& d, const float* M, size_t i, float B[12])
{
    const uint16_t* j = d.joints + 4 * i;
    const float* w = d.weights + 4 * i;
    const float *m0 = M + 12u * j[0], *m1 = M + 12u * j[1], *m2 = M + 12u * j[2], *m3 = M + 12u * j[3];
    for (int e = 0; e < 12; ++e) B[e] = ptskin::skin_blend(w[0], m0[e], w[1], m1[e], w[2], m2[e], w[3], m3[e]);
}

// one normal or tangent row: rest (4 floats, the record's) -> out (the first 3 floats)
void direction(const uint32_t* off, const PTMorphEntry* ent, size_t corner, const float* w, const float* B, const float* rest, float* out)
{
    float m[3] = {rest[0], rest[1], rest[2]};
    const bool listed = off && off[corner + 1] > off[corner];
    if (listed) fold(off, ent, corner, w, m);
    if (B) morph_skin_direction(B, m, rest, out);
    else if (listed) morph_direction(m, rest, out);             // no entry and no palette: the copy of the rest record stands
}

} // namespace

bool morph_check(const PTMorphDesc& d, uint32_t triCount, uint32_t materialCount, std::string& err)
{
    if (!d.restVertices || !d.positionOffsets) { err = "PTMorphDesc: restVertices / positionOffsets == NULL"; return false; }
    if (d.targetCount < 1u || d.targetCount > PT_MORPH_MAX_TARGETS) {
        err = "PTMorphDesc.targetCount (" + std::to_string(d.targetCount) + ") is not in 1 ... " + std::to_string(PT_MORPH_MAX_TARGETS);
        return false;
    }
    if ((!d.normalOffsets && d.normalEntries) || (!d.tangentOffsets && d.tangentEntries)) { err = "PTMorphDesc: a stream has entries but no offsets"; return false; }
    if ((d.normalOffsets || d.tangentOffsets) && !d.restAttrs) { err = "PTMorphDesc: a normal or tangent stream needs restAttrs"; return false; }
    const size_t n = (size_t)triCount * 3u;
    for (size_t i = 0; i < n; ++i) {
        const PTFloat4& v = d.restVertices[i];
        if (!std::isfinite(v.x) || !std::isfinite(v.y) || !std::isfinite(v.z)) { err = "rest vertex " + std::to_string(i) + " is not finite"; return false; }
    }
    if (!check_stream("position", d.positionOffsets, d.positionEntries, n, d.targetCount, err)) return false;
    if (d.normalOffsets && !check_stream("normal", d.normalOffsets, d.normalEntries, n, d.targetCount, err)) return false;
    if (d.tangentOffsets && !check_stream("tangent", d.tangentOffsets, d.tangentEntries, n, d.targetCount, err)) return false;
    for (uint32_t t = 0; d.restAttrs && materialCount != 0xFFFFFFFFu && t < triCount; ++t)
        if (d.restAttrs[t].materialIndex >= materialCount) {
            err = "triangle " + std::to_string(t) + ": materialIndex " + std::to_string(d.restAttrs[t].materialIndex) + " >= materialCount";
            return false;
        }
    return true;
}

bool morph_check_weights(const float* weights, uint32_t targetCount, std::string& err)
{
    for (uint32_t i = 0; i < targetCount; ++i)
        if (!std::isfinite(weights[i])) { err = "morph weight " + std::to_string(i) + " is not finite"; return false; }
    return true;
}

void morph_host(const PTMorphDesc& d, const PTSkinDesc* skin, uint32_t triCount, const float* w, const float* M, PTFloat4* outVerts,
                PTTriangleAttributes* outAttrs, float* outBounds)
{
    using ptskin::skin_max;
    using ptskin::skin_min;
    const bool skinned = skin && M;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < (size_t)triCount * 3u; ++i) {
        float B[12], p[3];
        const PTFloat4& v = d.restVertices[i];
        float acc[3] = {v.x, v.y, v.z};
        fold(d.positionOffsets, d.positionEntries, i, w, acc);
        if (skinned) {
            blend(*skin, M, i, B);
            ptskin::skin_point(B, acc[0], acc[1], acc[2], p);
        } else {
            p[0] = acc[0]; p[1] = acc[1]; p[2] = acc[2];
        }
        outVerts[i] = PTFloat4{p[0], p[1], p[2], 0.0f};
        for (int a = 0; a < 3; ++a) { mn[a] = skin_min(mn[a], p[a]); mx[a] = skin_max(mx[a], p[a]); }
        if (outAttrs && d.restAttrs) {
            const size_t t = i / 3u, corner = i % 3u;
            if (corner == 0) outAttrs[t] = d.restAttrs[t];               // tangent w, pads, uvs and materialIndex are the rest record's
            // a record as 8 rows of 4 floats: the corner's normal is row `corner`, its tangent row 3 + corner
            const float* rest = reinterpret_cast<const float*>(d.restAttrs + t);
            float* out = reinterpret_cast<float*>(outAttrs + t);
            direction(d.normalOffsets, d.normalEntries, i, w, skinned ? B : nullptr, rest + 4 * corner, out + 4 * corner);
            direction(d.tangentOffsets, d.tangentEntries, i, w, skinned ? B : nullptr, rest + 12 + 4 * corner, out + 12 + 4 * corner);
        }
    }
    if (outBounds)
        for (int a = 0; a < 3; ++a) { outBounds[a] = mn[a]; outBounds[3 + a] = mx[a]; }
}

uint64_t morph_layout_size(const uint32_t* off, uint32_t corners)
{
    uint64_t stored = 0;
    for (uint32_t c0 = 0; c0 < corners; c0 += 64u) {
        uint32_t longest = 0;
        for (uint32_t c = c0; c < corners && c < c0 + 64u; ++c) longest = off[c + 1] - off[c] > longest ? off[c + 1] - off[c] : longest;
        stored += (uint64_t)longest * 64u;
    }
    return stored;
}

bool morph_layout(const uint32_t* off, const PTMorphEntry* ent, uint32_t corners, MorphLayout& out)
{
    const uint64_t stored = morph_layout_size(off, corners);
    if (stored > 0xFFFFFFFFull) return false;
    const uint32_t slices = (corners + 63u) / 64u;
    out.count.assign(corners, 0u);
    out.sliceBase.assign((size_t)slices + 1u, 0u);
    out.entries.assign((size_t)stored, PTMorphEntry{0.0f, 0.0f, 0.0f, 0u});
    uint32_t base = 0;
    for (uint32_t k = 0; k < slices; ++k) {
        out.sliceBase[k] = base;
        uint32_t longest = 0;
        for (uint32_t c = k * 64u; c < corners && c < k * 64u + 64u; ++c) {
            const uint32_t n = off[c + 1] - off[c];
            out.count[c] = n;
            longest = n > longest ? n : longest;
            for (uint32_t s = 0; s < n; ++s) out.entries[(size_t)base + (size_t)s * 64u + (c & 63u)] = ent[off[c] + s];
        }
        base += longest * 64u;
    }
    out.sliceBase[slices] = base;
    return true;
}

} // namespace ptmorph
