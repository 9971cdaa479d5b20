// morph_sanitize_main.cpp — the host twin of the morph kernels (morph_host.cpp) in a stand-alone program for `make morph-sanitize`
// (AddressSanitizer + UBSan, host code only, no GPU): morphs and skins a generated mesh with exactly sized heap arrays, checks the
// result against the rule applied by hand and the device layout against the stream it came from, and makes the refusals.
// Prints "morph ok" and returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "morph_rule.h"

namespace {

uint32_t g_state = 54321u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("morph-sanitize: %s\n", what); return 1; }

// a random stream: corner c lists every target with probability `density`; corner `full` lists all of them, corner `none` none
void stream(uint32_t corners, uint32_t K, float density, uint32_t full, uint32_t none, std::vector<uint32_t>& off, std::vector<PTMorphEntry>& ent)
{
    off.assign(1, 0u);
    ent.clear();
    for (uint32_t c = 0; c < corners; ++c) {
        for (uint32_t k = 0; k < K; ++k)
            if (c != none && (c == full || rnd() < density)) ent.push_back(PTMorphEntry{rnd() - 0.5f, rnd() - 0.5f, rnd() - 0.5f, k});
        off.push_back((uint32_t)ent.size());
    }
}

} // namespace

int main()
{
    const uint32_t T = 301, K = 37, J = 16, N = T * 3;
    std::vector<PTFloat4> rest(N), out(N), plain(N);
    std::vector<PTTriangleAttributes> restAttrs(T), outAttrs(T);
    std::vector<float> w(K), M((size_t)J * 12), sw((size_t)N * 4);
    std::vector<uint16_t> joints((size_t)N * 4);
    for (uint32_t i = 0; i < N; ++i) rest[i] = PTFloat4{rnd() * 4 - 2, rnd() * 4 - 2, rnd() * 4 - 2, 1.0f};
    for (uint32_t k = 0; k < K; ++k) w[k] = rnd() * 2 - 0.5f;
    for (uint32_t t = 0; t < T; ++t) {
        float* r = reinterpret_cast<float*>(&restAttrs[t]);
        for (int k = 0; k < 32; ++k) r[k] = rnd() - 0.5f;
        restAttrs[t].materialIndex = t % 7;
    }
    for (uint32_t j = 0; j < J; ++j) {                   // a rotation about z, a uniform scale, a translation
        const float a = 6.28f * rnd(), s = 0.5f + rnd(), c = std::cos(a) * s, n = std::sin(a) * s;
        const float m[12] = {c, -n, 0, rnd() - 0.5f, n, c, 0, rnd() - 0.5f, 0, 0, s, rnd() - 0.5f};
        std::memcpy(&M[(size_t)j * 12], m, sizeof(m));
    }
    for (uint32_t i = 0; i < N; ++i)
        for (int k = 0; k < 4; ++k) { joints[4 * i + k] = (uint16_t)(rnd() * J) % J; sw[4 * i + k] = 0.25f; }
    std::vector<uint32_t> po, no, to;
    std::vector<PTMorphEntry> pe, ne, te;
    stream(N, K, 0.1f, 5, 6, po, pe);
    stream(N, K, 0.05f, 7, 0, no, ne);
    stream(N, K, 0.0f, N, N, to, te);                    // a tangent stream that is present and empty
    pe.shrink_to_fit(); ne.shrink_to_fit();

    PTMorphDesc d = {};
    d.structSize = sizeof(d); d.targetCount = K;
    d.restVertices = rest.data(); d.restAttrs = restAttrs.data();
    d.positionOffsets = po.data(); d.positionEntries = pe.data();
    d.normalOffsets = no.data(); d.normalEntries = ne.data();
    d.tangentOffsets = to.data(); d.tangentEntries = nullptr;
    PTSkinDesc s = {};
    s.structSize = sizeof(s); s.jointCount = J;
    s.restVertices = rest.data(); s.joints = joints.data(); s.weights = sw.data();
    std::string err;
    if (!ptmorph::morph_check(d, T, 7, err) || !ptmorph::morph_check_weights(w.data(), K, err)) return bad(err.c_str());
    float box[6];
    ptmorph::morph_host(d, nullptr, T, w.data(), nullptr, plain.data(), outAttrs.data(), box);

    // corner 5 lists every target: the rule by hand
    float acc[3] = {rest[5].x, rest[5].y, rest[5].z};
    for (uint32_t e = po[5]; e < po[6]; ++e) {
        acc[0] = acc[0] + w[pe[e].target] * pe[e].dx; acc[1] = acc[1] + w[pe[e].target] * pe[e].dy; acc[2] = acc[2] + w[pe[e].target] * pe[e].dz;
    }
    if (po[6] - po[5] != K || plain[5].x != acc[0] || plain[5].y != acc[1] || plain[5].z != acc[2] || plain[5].w != 0.0f) return bad("the dense corner is not the rule");
    if (plain[6].x != rest[6].x || plain[6].y != rest[6].y || plain[6].z != rest[6].z) return bad("a corner without entries moved");
    for (uint32_t i = 0; i < N; ++i) {
        const float p[3] = {plain[i].x, plain[i].y, plain[i].z};
        for (int a = 0; a < 3; ++a)
            if (!(p[a] >= box[a] && p[a] <= box[3 + a])) return bad("a vertex lies outside the bounds");
    }
    if (std::memcmp(outAttrs[0].normal0, restAttrs[0].normal0, 16) != 0) return bad("a normal without entries is not the rest bytes");
    const float* n7 = outAttrs[2].normal1;                // corner 7: triangle 2, corner 1
    if (std::fabs(n7[0] * n7[0] + n7[1] * n7[1] + n7[2] * n7[2] - 1.0f) > 1e-5f) return bad("a morphed normal is not unit length");
    for (uint32_t t = 0; t < T; ++t)
        if (std::memcmp(outAttrs[t].tangent0, restAttrs[t].tangent0, 48) != 0 || std::memcmp(outAttrs[t].uv0, restAttrs[t].uv0, 32) != 0)
            return bad("tangents of an empty stream / uvs / materialIndex were not copied");

    // morph, then skin: the skin's point of the morphed position
    ptmorph::morph_host(d, &s, T, w.data(), M.data(), out.data(), outAttrs.data(), box);
    float B[12], want[3];
    for (int e = 0; e < 12; ++e)
        B[e] = ptskin::skin_blend(0.25f, M[12u * joints[20] + e], 0.25f, M[12u * joints[21] + e], 0.25f, M[12u * joints[22] + e], 0.25f, M[12u * joints[23] + e]);
    ptskin::skin_point(B, acc[0], acc[1], acc[2], want);
    if (out[5].x != want[0] || out[5].y != want[1] || out[5].z != want[2]) return bad("morph + skin is not skin_point of the morphed position");

    // the device layout holds the stream's entries where the kernels look for them, and zeroes elsewhere
    ptmorph::MorphLayout L;
    if (!ptmorph::morph_layout(po.data(), pe.data(), N, L)) return bad("the layout was refused");
    if (L.entries.size() != ptmorph::morph_layout_size(po.data(), N) || L.sliceBase.size() != (N + 63) / 64 + 1) return bad("the layout's sizes");
    size_t listed = 0;
    for (uint32_t c = 0; c < N; ++c) {
        if (L.count[c] != po[c + 1] - po[c]) return bad("a corner's count");
        const uint32_t slots = (L.sliceBase[c / 64 + 1] - L.sliceBase[c / 64]) / 64;
        for (uint32_t k = 0; k < slots; ++k) {
            const PTMorphEntry& e = L.entries[(size_t)L.sliceBase[c / 64] + 64u * k + c % 64];
            const PTMorphEntry zero = {0.0f, 0.0f, 0.0f, 0u};
            if (std::memcmp(&e, k < L.count[c] ? &pe[po[c] + k] : &zero, 16) != 0) return bad("a slot of the layout");
            listed += k < L.count[c];
        }
    }
    if (listed != pe.size()) return bad("the layout lost entries");

    // the refusals: each on an exactly sized copy
    PTMorphDesc e = d;
    e.targetCount = 0;
    if (ptmorph::morph_check(e, T, 7, err)) return bad("targetCount 0 was accepted");
    e.targetCount = PT_MORPH_MAX_TARGETS + 1;
    if (ptmorph::morph_check(e, T, 7, err)) return bad("targetCount 1025 was accepted");
    std::vector<PTMorphEntry> be(pe);
    be[be.size() - 1].target = K;
    e = d; e.positionEntries = be.data();
    if (ptmorph::morph_check(e, T, 7, err)) return bad("a target >= targetCount was accepted");
    be = pe;
    be[po[5] + 1].target = be[po[5]].target;
    e.positionEntries = be.data();
    if (ptmorph::morph_check(e, T, 7, err)) return bad("targets that do not ascend were accepted");
    be = pe;
    be[3].dy = std::numeric_limits<float>::infinity();
    e.positionEntries = be.data();
    if (ptmorph::morph_check(e, T, 7, err)) return bad("an infinite delta was accepted");
    std::vector<uint32_t> bo(po);
    bo[0] = 1;
    e = d; e.positionOffsets = bo.data();
    if (ptmorph::morph_check(e, T, 7, err)) return bad("offsets[0] != 0 was accepted");
    bo = po;
    bo[9] = bo[10] + 1;
    e.positionOffsets = bo.data();
    if (ptmorph::morph_check(e, T, 7, err)) return bad("decreasing offsets were accepted");
    e = d; e.restAttrs = nullptr;
    if (ptmorph::morph_check(e, T, 7, err)) return bad("a normal stream without restAttrs was accepted");
    std::vector<float> bw(w);
    bw[K - 1] = std::numeric_limits<float>::quiet_NaN();
    if (ptmorph::morph_check_weights(bw.data(), K, err)) return bad("a NaN weight was accepted");
    if (ptmorph::morph_check(d, T, 6, err)) return bad("a materialIndex >= materialCount was accepted");
    std::printf("morph ok\n");
    return 0;
}
