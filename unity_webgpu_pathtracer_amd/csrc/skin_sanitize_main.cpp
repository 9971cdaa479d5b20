// skin_sanitize_main.cpp — the host twin of the skinning kernels (skin_host.cpp) in a stand-alone program for `make skin-sanitize`
// (AddressSanitizer + UBSan, host code only, no GPU): skins a generated mesh with exactly sized heap arrays, checks the result
// against the rule applied by hand, and makes the three refusals.  Prints "skin ok" and returns 0, or says what went wrong.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "skin_rule.h"

namespace {

uint32_t g_state = 12345u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

int bad(const char* what) { std::printf("skin-sanitize: %s\n", what); return 1; }

} // namespace

int main()
{
    const uint32_t T = 301, J = 64, N = T * 3;
    std::vector<PTFloat4> rest(N), out(N);
    std::vector<uint16_t> joints((size_t)N * 4);
    std::vector<float> weights((size_t)N * 4), M((size_t)J * 12);
    std::vector<PTTriangleAttributes> restAttrs(T), outAttrs(T);
    for (uint32_t j = 0; j < J; ++j) {                   // a rotation about z, a uniform scale, a translation
        const float a = 6.28f * rnd(), s = 0.5f + rnd(), c = std::cos(a) * s, n = std::sin(a) * s;
        const float m[12] = {c, -n, 0, rnd() - 0.5f, n, c, 0, rnd() - 0.5f, 0, 0, s, rnd() - 0.5f};
        std::memcpy(&M[(size_t)j * 12], m, sizeof(m));
    }
    for (uint32_t i = 0; i < N; ++i) {
        rest[i] = PTFloat4{rnd() * 4 - 2, rnd() * 4 - 2, rnd() * 4 - 2, 1.0f};
        float sum = 0;
        for (int k = 0; k < 4; ++k) {
            joints[4 * i + k] = (uint16_t)(rnd() * J) % J;
            weights[4 * i + k] = (i % 5 == (uint32_t)k) ? 0.0f : rnd();
            sum += weights[4 * i + k];
        }
        for (int k = 0; k < 4; ++k) weights[4 * i + k] /= sum;
    }
    for (int k = 0; k < 4; ++k) weights[k] = k == 2 ? 1.0f : 0.0f;         // vertex 0: one-hot on its third joint
    for (uint32_t t = 0; t < T; ++t) {
        float* r = reinterpret_cast<float*>(&restAttrs[t]);
        for (int k = 0; k < 32; ++k) r[k] = rnd() - 0.5f;
        restAttrs[t].materialIndex = t % 7;
    }
    std::memset(restAttrs[1].normal1, 0, sizeof(restAttrs[1].normal1));     // a zero-length rest normal is kept

    PTSkinDesc d = {};
    d.structSize = sizeof(d); d.jointCount = J;
    d.restVertices = rest.data(); d.joints = joints.data(); d.weights = weights.data(); d.restAttrs = restAttrs.data();
    std::string err;
    if (!ptskin::skin_check(d, T, 7, err) || !ptskin::skin_check_palette(M.data(), J, err)) return bad(err.c_str());
    float box[6];
    ptskin::skin_host(d, T, M.data(), out.data(), outAttrs.data(), box);

    float want[3];
    ptskin::skin_point(&M[(size_t)joints[2] * 12], rest[0].x, rest[0].y, rest[0].z, want);
    // 1 * m + 0 * other terms: exact for finite matrices
    if (out[0].x != want[0] || out[0].y != want[1] || out[0].z != want[2] || out[0].w != 0.0f) return bad("one-hot weights are not the rigid transform");
    for (uint32_t i = 0; i < N; ++i) {
        const float p[3] = {out[i].x, out[i].y, out[i].z};
        for (int a = 0; a < 3; ++a)
            if (!(p[a] >= box[a] && p[a] <= box[3 + a])) return bad("a vertex lies outside the bounds");
    }
    if (std::memcmp(outAttrs[1].normal1, restAttrs[1].normal1, 12) != 0) return bad("a zero-length normal was not kept");
    for (uint32_t t = 0; t < T; ++t) {
        if (std::memcmp(outAttrs[t].uv0, restAttrs[t].uv0, 32) != 0 || outAttrs[t].pad3 != restAttrs[t].pad3) return bad("uvs / materialIndex / pads were not copied");
        const float* n = outAttrs[t].normal0;
        if (t != 1 && std::fabs(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] - 1.0f) > 1e-5f) return bad("a normal is not unit length");
    }

    // the refusals: each on an exactly sized copy
    std::vector<uint16_t> badJoints(joints);
    badJoints[badJoints.size() - 1] = (uint16_t)J;
    PTSkinDesc e = d;
    e.joints = badJoints.data();
    if (ptskin::skin_check(e, T, 7, err)) return bad("a joint index >= jointCount was accepted");
    std::vector<float> badWeights(weights);
    badWeights[7] = std::numeric_limits<float>::quiet_NaN();
    e = d;
    e.weights = badWeights.data();
    if (ptskin::skin_check(e, T, 7, err)) return bad("a NaN weight was accepted");
    std::vector<float> badM(M);
    badM[badM.size() - 1] = std::numeric_limits<float>::quiet_NaN();
    if (ptskin::skin_check_palette(badM.data(), J, err)) return bad("a NaN matrix was accepted");
    if (ptskin::skin_check(d, T, 6, err)) return bad("a materialIndex >= materialCount was accepted");
    std::printf("skin ok\n");
    return 0;
}
