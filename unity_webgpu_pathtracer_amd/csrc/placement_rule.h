// placement_rule.h — probe placement (include/ptmi_plugin.h Part 18): the one definition of the rule -- how a stored
// offset is read, a sample's side, the per-lane selection keys and their merge, the inside test and the move -- shared by the
// kernels (pt_placement.hip) and the host twin (placement_host.cpp).  Every fp32 operator is one IEEE binary32 operation in the
// order written, and both sides are compiled with -ffp-contract=off, so both give the same bits.  The statistics are integer
// counts and min / max of 64-bit keys: exact in any order.  tests/placement_ref.py restates it.  Seeding and sphere direction are
// sh_rule.h's; the placed lookup is volume_rule.h's.
#pragma once
#include "volume_rule.h"

#define PT_PLACE_HD PT_SH_HD

namespace ptplace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kChunkSamples = 1ull << 20;      // PTProbePlace: a chunk holds floor(2^20 / samples) whole probes

// |o[a]| <= maxOffset * spacing[a] on every axis; a NaN fails
PT_PLACE_HD bool passes(const PTProbePlaceParams& p, const float o[3])
{
    bool ok = true;
    for (uint32_t a = 0; a < 3u; ++a) ok = ok && (pt_abs(o[a]) <= p.maxOffset * p.spacing[a]);
    return ok;
}

// a stored offset that does not pass is read as 0, whole
PT_PLACE_HD void read_offset(const PTProbePlaceParams& p, const float stored[3], float o[3])
{
    const bool ok = passes(p, stored);
    for (uint32_t a = 0; a < 3u; ++a) o[a] = ok ? stored[a] : 0.0f;
}

// What a lane, and after the merge a probe, knows of its samples.  The keys hold (bits(t) << 32) | j for the two minima and
// (bits(t) << 32) | (0xFFFFFFFF - j) for the maximum: the t of a hit is positive, so its bits order as the float does, and the low
// word settles equal t in favour of the lowest j.  A key means something only where its count is not 0.
struct Tally {
    uint32_t back, front;
    uint64_t nearestBack, nearestFront, farthestFront;
};

PT_PLACE_HD Tally empty()
{
    return Tally{0u, 0u, ~0ull, ~0ull, 0ull};
}

// one hit sample: w its direction, n the surface record's normal
PT_PLACE_HD void add_hit(Tally& T, uint32_t j, float t, const float w[3], const float n[3])
{
    const float c = (w[0] * n[0] + w[1] * n[1]) + w[2] * n[2];
    const uint64_t hi = (uint64_t)pt_asuint(t) << 32;
    if (c > 0.0f) {
        T.back += 1u;
        const uint64_t k = hi | j;
        T.nearestBack = k < T.nearestBack ? k : T.nearestBack;
    } else {                                                    // a NaN lands here
        T.front += 1u;
        const uint64_t k = hi | j, f = hi | (kNone - j);
        T.nearestFront = k < T.nearestFront ? k : T.nearestFront;
        T.farthestFront = f > T.farthestFront ? f : T.farthestFront;
    }
}

PT_PLACE_HD void merge(Tally& T, const Tally& o)
{
    T.back += o.back;
    T.front += o.front;
    T.nearestBack = o.nearestBack < T.nearestBack ? o.nearestBack : T.nearestBack;
    T.nearestFront = o.nearestFront < T.nearestFront ? o.nearestFront : T.nearestFront;
    T.farthestFront = o.farthestFront > T.farthestFront ? o.farthestFront : T.farthestFront;
}

PT_PLACE_HD PTProbePlaceStats stats_of(const Tally& T)
{
    PTProbePlaceStats s;
    s.back = T.back;
    s.front = T.front;
    s.nearestBack = T.back ? (uint32_t)T.nearestBack : kNone;
    s.nearestFront = T.front ? (uint32_t)T.nearestFront : kNone;
    s.farthestFront = T.front ? kNone - (uint32_t)T.farthestFront : kNone;
    s.tNearestBack = T.back ? pt_asfloat((uint32_t)(T.nearestBack >> 32)) : 0.0f;
    s.tNearestFront = T.front ? pt_asfloat((uint32_t)(T.nearestFront >> 32)) : 0.0f;
    s.tFarthestFront = T.front ? pt_asfloat((uint32_t)(T.farthestFront >> 32)) : 0.0f;
    return s;
}

PT_PLACE_HD bool inside(const PTProbePlaceParams& p, uint32_t back, uint32_t samples)
{
    return (float)back > p.backfaceShare * (float)samples;
}

// The end of a step for one probe: its state, and with move the new offset.  o is the offset as read (read_offset), replaced by
// an accepted candidate.  Only the direction the move goes along is made again from the seed.
PT_PLACE_HD uint32_t finish(const PTProbePlaceParams& p, uint32_t seed, uint32_t firstSample, uint32_t samples, const PTProbePlaceStats& s, bool move, float o[3])
{
    const bool in = inside(p, s.back, samples);
    if (move) {
        float cand[3] = {o[0], o[1], o[2]};
        if (in) {                                               // back > 0, so there is a nearest back sample
            uint32_t rng = ptsh::sample_rng(seed, firstSample, s.nearestBack);
            float w[3];
            ptsh::direction(rng, w);
            const float len = s.tNearestBack + p.minFrontDistance * 0.5f;
            for (uint32_t a = 0; a < 3u; ++a) cand[a] = o[a] + w[a] * len;
        } else if (s.front != 0u && s.tNearestFront < p.minFrontDistance) {
            uint32_t rng = ptsh::sample_rng(seed, firstSample, s.nearestFront);
            float w[3];
            ptsh::direction(rng, w);
            const float len = p.minFrontDistance - s.tNearestFront;
            for (uint32_t a = 0; a < 3u; ++a) cand[a] = o[a] - w[a] * len;
        }
        if (passes(p, cand))
            for (uint32_t a = 0; a < 3u; ++a) o[a] = cand[a];
    }
    return in ? PT_PROBE_INSIDE : 0u;
}

// ---- the host twins and the checks the entry points share (placement_host.cpp); false: err says why ----
bool check_params(const PTProbePlaceParams* params, std::string& err);
bool check_flags(uint32_t flags, std::string& err);
bool place_step_host(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const PTProbePlaceParams* params, const PTRayHit* hits,
                     const PTRaySurface* surfaces, int move, PTProbePlacement* inout, PTProbePlaceStats* stats, std::string& err);
bool grid_irradiance_placed_host(const PTProbeGrid* grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTProbePlacement* placement,
                                 const PTReceiver* queries, uint64_t count, PTIrradiance* out, std::string& err);

} // namespace ptplace
