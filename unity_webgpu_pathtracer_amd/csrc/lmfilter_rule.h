// lmfilter_rule.h — the lightmap denoiser (include/ptmi_plugin.h Part 17): the one definition of the rule, shared by
// the kernels (pt_lmfilter.hip) and the host twin (lmfilter_host.cpp).  Every fp32 operator is one IEEE binary32 operation, left
// to right as written, and both sides are compiled with -ffp-contract=off, so both give the same bits.  The rule uses only
// + - * /, sqrtf, fabsf, comparisons and max: the weights are rational and the normal lobe is built by squarings, so nothing
// depends on a library's exp or pow.  tests/lmfilter_ref.py restates it in numpy from this text.
//
// An edge-stopping a-trous filter over the texels of an atlas.  It works on images of width x height texels that the list fills:
//
//  1. Texel state.  A texel no list entry names is uncovered.  Entry i at texel t = texels[i]: e = irr[i].rgb;
//     l = (e.r * 0.299f + e.g * 0.587f) + e.b * 0.114f  (luminance3);  S = (float)samples;
//     v = max(((m2 - (S * l) * l) / (S - 1.0f)), 0.0f) / S : the variance of the mean of the luminance (max is fmaxf).
//     The entry is BAD when any of rgb, m2, position or normal is not finite, or v is NaN.  A bad entry's 16 input bytes are its
//     output and its texel is never a tap.  A texel that is covered and not bad is GOOD; it carries (e, v), P = position, N = normal.
//  2. Footprint.  h2_p = the smallest d2(p, q) that is > 0 over the good 4-neighbours q inside the image, looked at in the order
//     left, right, up, down; 0 when there is none.  d2(p, q): d = P_q - P_p per component, (d.x * d.x + d.y * d.y) + d.z * d.z.
//     A good texel with h2 == 0 is ISOLATED: it keeps (e, v) at every level, and still is a tap of others.
//  3. Position cut.  A tap q of p at the offset (ox, oy) is a good texel inside the image at (x + ox, y + oy).  It is admitted
//     when (ox, oy) == (0, 0), or d2(p, q) <= ((sigmaPosition * sigmaPosition) * h2_p) * (float)(ox * ox + oy * oy).
//  4. Level k = 0 ... iterations - 1, s = 2^k, for every good texel p that is not isolated, from the state of level k - 1:
//     g_p: over the offsets (dx, dy), dy = -1 ... 1 outer and dx = -1 ... 1 inner, the admitted ones: c = b[dx] * b[dy] with
//     b = {0.25f, 0.5f, 0.25f};  gw = gw + c;  gv = gv + c * v_q  (both from +0.0f);  g_p = gv / gw.
//     Then over the offsets (dx * s, dy * s), dy = -2 ... 2 outer and dx = -2 ... 2 inner, the admitted ones:
//       w_n = max((N_p.x * N_q.x + N_p.y * N_q.y) + N_p.z * N_q.z, 0.0f), then normalPower times w_n = w_n * w_n;
//       z = fabsf((N_p.x * d.x + N_p.y * d.y) + N_p.z * d.z) / ((sigmaPlane * sqrtf(h2_p)) * (float)s + 1e-12f)  with d = P_q - P_p;
//       r = 1.0f / (1.0f + z * z);  w_z = r * r;
//       x = fabsf(l_p - l_q) / (sigmaLuminance * sqrtf(g_p) + 1e-6f)  with l = luminance3 of the level's input e;
//       r = 1.0f / (1.0f + x * x);  w_l = r * r;
//       w = (((h[dx] * h[dy]) * w_n) * w_z) * w_l  with h = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
//       sw = sw + w;  se[c] = se[c] + w * e_q[c];  sv = sv + (w * w) * v_q  (all from +0.0f).
//     If sw > 0: e' = se[c] / sw per channel and v' = sv / (sw * sw); otherwise the texel keeps (e, v).
//  5. Output.  out[i].rgb = the final e of texels[i], out[i].m2 = its final v.  With iterations == 0 that is the input's rgb and
//     the v of step 1.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string>
#include "ptmi_math.h"
#include "ptmi_plugin.h"

#if defined(__HIPCC__)
#define PT_LMF_HD __host__ __device__ __forceinline__
#else
#define PT_LMF_HD inline
#endif

namespace ptlmf {

constexpr uint32_t kMaxSize = 8192u;
constexpr uint32_t kMaxIterations = 8u;
constexpr uint32_t kMaxNormalPower = 7u;
constexpr uint32_t kMinSamples = 2u, kMaxSamples = 1u << 24;
// the flags word of a texel (the normal guide's .w): 0 = uncovered
constexpr uint32_t kGood = 1u, kBad = 2u;

// the sigmas as the rule uses them
struct Sigmas {
    float luminance, position2, plane;       // position2 = sigmaPosition * sigmaPosition
    uint32_t normalPower;
};

// what a level reads of one texel
struct Texel {
    float e[3], v;
    float P[3], h2;
    float N[3];
};

PT_LMF_HD bool finite(float x) { return pt_abs(x) <= 3.402823466e38f; }

PT_LMF_HD float luminance(const float e[3]) { return (e[0] * 0.299f + e[1] * 0.587f) + e[2] * 0.114f; }

// step 1: the variance of the mean luminance behind an entry
PT_LMF_HD float entry_variance(const float e[3], float m2, uint32_t samples)
{
    const float l = luminance(e), S = (float)samples;
    return pt_max((m2 - (S * l) * l) / (S - 1.0f), 0.0f) / S;
}

PT_LMF_HD bool entry_bad(const PTReceiver& r, const PTIrradiance& i, float v)
{
    bool ok = finite(i.m2) && !pt_isnan(v);
    for (int a = 0; a < 3; ++a) ok = ok && finite(i.rgb[a]) && finite(r.position[a]) && finite(r.normal[a]);
    return !ok;
}

PT_LMF_HD float dist2(const float Pp[3], const float Pq[3])
{
    const float dx = Pq[0] - Pp[0], dy = Pq[1] - Pp[1], dz = Pq[2] - Pp[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// step 2: one neighbour into the running footprint
PT_LMF_HD float footprint_step(float h2, const float Pp[3], const float Pq[3])
{
    const float d2 = dist2(Pp, Pq);
    return (d2 > 0.0f && (h2 == 0.0f || d2 < h2)) ? d2 : h2;
}

// the filter kernels b and h of step 4 at the offset d (selects: an unrolled or a rolled loop reads no table)
PT_LMF_HD float kernel3(int32_t d) { return d == 0 ? 0.5f : 0.25f; }
PT_LMF_HD float kernel5(int32_t d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// step 3
PT_LMF_HD bool admitted(const Texel& p, const Texel& q, float position2, int32_t ox, int32_t oy)
{
    if (ox == 0 && oy == 0) return true;
    return dist2(p.P, q.P) <= (position2 * p.h2) * (float)(ox * ox + oy * oy);
}

// Step 4 for one good, not isolated texel p at (x, y).  fetch(x, y, q): false when (x, y) is no good texel (the caller has
// checked that it lies inside the image), else q is its texel from the level's input.
template <class Fetch>
PT_LMF_HD void filter_texel(const Sigmas& sg, const Texel& p, int32_t x, int32_t y, int32_t width, int32_t height, int32_t s, Fetch fetch, float out[4])
{
    float gw = 0.0f, gv = 0.0f;
    for (int32_t dy = -1; dy <= 1; ++dy)
        for (int32_t dx = -1; dx <= 1; ++dx) {
            const int32_t xx = x + dx, yy = y + dy;
            Texel q;
            if (xx < 0 || yy < 0 || xx >= width || yy >= height || !fetch(xx, yy, q) || !admitted(p, q, sg.position2, dx, dy)) continue;
            const float c = kernel3(dx) * kernel3(dy);
            gw = gw + c;
            gv = gv + c * q.v;
        }
    const float g = gv / gw;
    const float lp = luminance(p.e);
    const float zden = (sg.plane * pt_sqrt(p.h2)) * (float)s + 1e-12f;
    const float xden = sg.luminance * pt_sqrt(g) + 1e-6f;
    float sw = 0.0f, sv = 0.0f, se[3] = {0.0f, 0.0f, 0.0f};
    for (int32_t dy = -2; dy <= 2; ++dy)
        for (int32_t dx = -2; dx <= 2; ++dx) {
            const int32_t ox = dx * s, oy = dy * s, xx = x + ox, yy = y + oy;
            Texel q;
            if (xx < 0 || yy < 0 || xx >= width || yy >= height || !fetch(xx, yy, q) || !admitted(p, q, sg.position2, ox, oy)) continue;
            float wn = pt_max((p.N[0] * q.N[0] + p.N[1] * q.N[1]) + p.N[2] * q.N[2], 0.0f);
            for (uint32_t k = 0; k < sg.normalPower; ++k) wn = wn * wn;
            const float d[3] = {q.P[0] - p.P[0], q.P[1] - p.P[1], q.P[2] - p.P[2]};
            const float z = pt_abs((p.N[0] * d[0] + p.N[1] * d[1]) + p.N[2] * d[2]) / zden;
            const float rz = 1.0f / (1.0f + z * z);
            const float wz = rz * rz;
            const float xl = pt_abs(lp - luminance(q.e)) / xden;
            const float rl = 1.0f / (1.0f + xl * xl);
            const float wl = rl * rl;
            const float w = (((kernel5(dx) * kernel5(dy)) * wn) * wz) * wl;
            sw = sw + w;
            se[0] = se[0] + w * q.e[0];
            se[1] = se[1] + w * q.e[1];
            se[2] = se[2] + w * q.e[2];
            sv = sv + (w * w) * q.v;
        }
    if (sw > 0.0f) {
        out[0] = se[0] / sw; out[1] = se[1] / sw; out[2] = se[2] / sw;
        out[3] = sv / (sw * sw);
    } else {
        out[0] = p.e[0]; out[1] = p.e[1]; out[2] = p.e[2]; out[3] = p.v;
    }
}

// ---- host side (lmfilter_host.cpp) ----
// The checks the context's entry point shares with the twin.  false: err has the reason.
bool check_params(const PTLightmapDenoiseParams* params, std::string& err);
bool check_size(uint32_t width, uint32_t height, uint64_t count, std::string& err);
// The rule on the host.  false: err has the reason (the checks above, a NULL array, an index >= width * height, a duplicate).
bool denoise_host(const PTLightmapDenoiseParams* params, const uint32_t* texels, const PTReceiver* recv, const PTIrradiance* irr, uint64_t count,
                  uint32_t width, uint32_t height, PTIrradiance* out, std::string& err);

} // namespace ptlmf
