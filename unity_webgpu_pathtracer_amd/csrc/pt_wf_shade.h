// pt_wf_shade.h — what the shade and cleanup kernels of a launch sequence are made of: the slot <-> pixel mappings, the path state
// of a slot, and the two bodies (shade_slot, cleanup_slots).  Shared by pt_wavefront.hip, whose kernels index a slot's own pixel,
// and pt_repack.hip, whose kernels take the pixel from PTWfBuffers.pixelOf because the sequence moves paths between slots.
#pragma once
#include "pt_device.h"
#include "pt_launch.h"
#include "pt_wf_state.h"
#include <type_traits>

namespace {

// float4 state array k of the set (pt_launch.h PT_F4_*), addressed from ONE base pointer
PT_DEV float4* f4_array(const PTWfBuffers& B, uint32_t k) { return B.f4base + (size_t)k * B.f4stride; }
// the ray of (slot, kind): bounce ray (ro, rd), environment NEE (neeO, envD) or light NEE (neeO, lightD)
PT_DEV void fetch_ray(const PTWfBuffers& B, uint32_t slot, uint32_t kind, v3& o, v3& d)
{
    const float4* rec = f4_array(B, 2u * kind) + 2u * (size_t)slot;          // PT_F4_RAY0 / 1 / 2: one 32-byte record, one sector
    o = xyz(rec[0]);
    d = xyz(rec[1]);
}

// pack_flags / store_path / flush_counters: pt_wf_state.h (shared with pt_gather.hip)

// ------------------------------------------------------------------------------------------
// init: every owned pixel starts its first sample (camera ray in the slot, state = TRACE)
// ------------------------------------------------------------------------------------------
// the pixel slot and the pass (of a batch) a slot belongs to
PT_DEV uint32_t pixel_slot_of(const PTWfBuffers& B, uint32_t slot, uint32_t& pass)
{
    pass = 0u;
    if (slot >= B.slotsPerPass) { pass = slot / B.slotsPerPass; slot -= pass * B.slotsPerPass; }
    return slot;
}

// The pixel and the pass of a slot under the two mappings a kernel can be instantiated with (MAP): PTTileMap, the frame's owned
// blocks in their fixed order (every PTRenderPass* path), and PTListMap, the blocks of a per-call table (PTRenderPassActive).
// wgSlot is the first slot of the lane's workgroup -- formed from blockIdx, hence wave-uniform: under the list mapping the
// table entry is ONE scalar load per wave (SGPRs, not VGPRs; the shade kernel sits on its 128-VGPR line).  A workgroup never
// straddles two entries or two passes (64 or 256 slots, entries of 256).  base = the block's sample count when the call began.
PT_DEV bool wf_pixel(const PTTileMap& tm, const PTWfBuffers& B, uint32_t slot, uint32_t wgSlot, uint32_t& px, uint32_t& py, uint32_t& pass, uint32_t& base)
{
    base = 0u;
    return pt_slot_to_pixel(tm, pixel_slot_of(B, slot, pass), px, py);
}
PT_DEV bool wf_pixel(const PTListMap& lm, const PTWfBuffers& B, uint32_t slot, uint32_t wgSlot, uint32_t& px, uint32_t& py, uint32_t& pass, uint32_t& base)
{
    pass = wgSlot / B.slotsPerPass;
    const uint2 entry = lm.table[(wgSlot - pass * B.slotsPerPass) >> 8];
    base = entry.y;
    return pt_list_slot_to_pixel(lm.frameBlocksX, lm.coverW, lm.coverH, entry.x, slot & 255u, px, py);
}
template <class MAP> constexpr bool kListMap = std::is_same<MAP, PTListMap>::value;

// PTRayMap (radiance queries, pt_launch.h): slot s is entry s of the caller's ray list; there is no pixel, one pass, no base.
PT_DEV bool wf_pixel(const PTRayMap& rm, const PTWfBuffers& B, uint32_t slot, uint32_t wgSlot, uint32_t& px, uint32_t& py, uint32_t& pass, uint32_t& base)
{
    px = 0u; py = 0u; pass = 0u; base = 0u;
    return slot < rm.count;
}
template <class MAP> constexpr bool kRayMap = std::is_same<MAP, PTRayMap>::value;
// How the ray of a list entry's sample starts (the Source of path_step): path_start_ray with the entry's ray in place of the
// camera's, and no RNG draw.  Like path_start_ray it leaves radiance, throughput and depth alone: with the next-sample overlap the
// previous sample's radiance is still live when it runs (pt_device.h).
// The entry is two 16-byte vector loads by slot: {origin.xyz, direction.x} {direction.yz, rng, reserved}.
struct RaySample {
    const PTRadianceRay* rays; uint32_t slot;
    PT_DEV void operator()(const PTFrameParams&, uint32_t, uint32_t, PathRegs& r, Counters& cn) const { start_ray(r, cn); }
    PT_DEV void start_ray(PathRegs& r, Counters& cn) const
    {
        const float4* e = (const float4*)(rays + slot);
        const float4 a = e[0], b = e[1];
        cn.paths++;
        r.scatterPdf = 0.0f;
        r.maxRoughness = 0.0f;
        r.ro = mk3(a.x, a.y, a.z);
        r.rd = mk3(a.w, b.x, b.y);
        r.state = PS_TRACE;
    }
};
// path_init for a list entry: the state path_init leaves, with the entry's RNG state and ray
PT_DEV void ray_path_init(const PTRayMap& rm, uint32_t slot, PathRegs& r, Counters& cn)
{
    r.rng = rm.rays[slot].rng;
    r.sampleIdx = 0u;
    r.color = mk3(0.0f);
    r.env.valid = 0u; r.light.valid = 0u;
    r.env.dir = mk3(0.0f); r.light.dir = mk3(0.0f);
    r.env.contribution = mk3(0.0f); r.light.contribution = mk3(0.0f);
    r.neeOrigin = mk3(0.0f); r.pendThroughput = mk3(0.0f);
    r.hasPending = false; r.green = false;
    path_reset_sample(r);
    RaySample{rm.rays, slot}.start_ray(r, cn);
}

#ifndef PT_WF_SHADE_MIN_WAVES
#define PT_WF_SHADE_MIN_WAVES 3
#endif

// The path state of one slot as the flags word f describes it (state != DONE).  Used by the cleanup kernel; the shade kernel
// requests the same words all at once (shade_slot).  PACKED: the layout of a repacked sequence (pt_wf_state.h) -- the RNG state
// and the pending throughput come from the fourth lanes of rad, envC, lightC and thr; B.rng and B.pthr are not touched.
template <bool PACKED = false>
PT_DEV void load_path(const PTWfBuffers& B, uint32_t slot, uint32_t f, PathRegs& r)
{
    r.state = fl_state(f);
    r.hasPending = fl_pending(f);
    r.env.valid = fl_env(f);
    r.light.valid = fl_light(f);
    r.green = (f >> 6) & 1u;
    r.sampleIdx = (f >> 7) & 0xFFFu;
    r.depth = f >> 19;
    if constexpr (!PACKED) r.rng = B.rng[slot];
    float4 q;
    q = B.ray[0][2u * slot]; r.ro = xyz(q); r.scatterPdf = q.w;
    q = B.ray[0][2u * slot + 1u]; r.rd = xyz(q); r.maxRoughness = q.w;
    q = B.rad[slot]; r.radiance = xyz(q);
    if constexpr (PACKED) r.rng = pt_asuint(q.w);
    const float4 qthr = B.thr[slot];
    r.throughput = xyz(qthr);
    r.color = xyz(B.color[slot]);
    r.env.dir = mk3(0.0f); r.light.dir = mk3(0.0f); r.neeOrigin = mk3(0.0f);
    r.env.contribution = mk3(0.0f); r.light.contribution = mk3(0.0f); r.pendThroughput = mk3(0.0f);
    if (r.hasPending) {
        const float4 qe = B.envC[slot], ql = B.lightC[slot];
        r.env.contribution = xyz(qe);
        r.light.contribution = xyz(ql);
        if constexpr (PACKED) r.pendThroughput = mk3(qe.w, ql.w, qthr.w);
        else r.pendThroughput = xyz(B.pthr[slot]);
    }
}

// non-zero iff a and b differ in a bit
PT_DEV uint32_t differing_bits(v3 a, v3 b) { return (pt_asuint(a.x) ^ pt_asuint(b.x)) | (pt_asuint(a.y) ^ pt_asuint(b.y)) | (pt_asuint(a.z) ^ pt_asuint(b.z)); }

// Everything the shade step does for one slot (flags word f already read, state != DONE).
// Every word of the slot's state is requested up front in ONE batch, whether the flags say it is meaningful or not (the pending
// NEE terms, the two occlusion bytes, the hit record): requested where they are used they formed a chain of four dependent
// round trips (state -> pending terms -> occlusion bytes -> hit record, ~870 cycles each at the shade kernel's 4 waves/SIMD)
// in front of the attribute / material / texture chain.  A value the flags do not cover is read and ignored.
// `slot` indexes the path-state arrays; `pixelSlot` is the pixel the state belongs to (the same number in schedules 1-3, where
// every pixel has its own slot; a context's current pixel in schedule 4, which also wants the finished pixel's sample sum in
// B.pixsum[pixelSlot]: PIXSUM).
// wgSlot: see wf_pixel (only read under the list mapping).
// PACKED (with PIXSUM; the shade kernel of a repacked sequence, pt_repack.hip): the slot's state is in the packed layout of
// pt_wf_state.h, and the step stores only what changes memory that somebody reads again --
//   - B.rng and B.pthr are neither read nor written: the RNG state rides in rad.w, the pending throughput in envC.w, lightC.w
//     (written by the sink with those arrays) and thr.w (every store of thr carries the current pendThroughput.z);
//   - color is loaded with the batch, but stored only by a step that changed one of its three words: a step that folds no
//     sample (about three in four) leaves the array alone;
//   - a slot that ends the step DONE stores its flags word and pixsum[pixel] only: nothing reads its ray record, rad, thr or
//     color again (the resolve reads pixsum, the cleanup skips DONE slots, a repack overwrites or marks them).
// Every arithmetic operation of the path is the one of the unpacked step, in the same order.
template <bool STATS, bool PIXSUM = false, class MAP = PTTileMap, bool PACKED = false>
PT_DEV bool shade_slot(const DScene& S, const PTFrameParams& P, const MAP& tm, const PTWfBuffers& B, uint32_t slot, uint32_t pixelSlot,
                       uint32_t f, Counters& cn, uint32_t wgSlot = 0u)
{
    uint32_t px, py, pass, base;
    wf_pixel(tm, B, pixelSlot, wgSlot, px, py, pass, base);
    static_assert(!PACKED || (PIXSUM && !kRayMap<MAP>), "the packed layout is a repacked sequence's: frames only, sums in pixsum");
    uint32_t rng = 0u;
    if constexpr (!PACKED) rng = B.rng[slot];
    float4 qro = B.ray[0][2u * slot], qrd = B.ray[0][2u * slot + 1u], qrad = B.rad[slot], qthr = B.thr[slot], qcol = B.color[slot];
    float4 qenvC = B.envC[slot], qlightC = B.lightC[slot], qpthr = PACKED ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : B.pthr[slot], qhit = B.hit[slot];
    uint32_t o0 = B.occl[slot], o1 = B.occl[(size_t)B.numSlots + slot];
    float4 qhit2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (S.hasTlas) qhit2 = B.hit2[slot];
    // pinned: left alone, the compiler sinks each load into the branch that uses it again
    if constexpr (PACKED)
        asm volatile("" : "+v"(qro.x), "+v"(qrd.x), "+v"(qrad.x), "+v"(qthr.x), "+v"(qcol.x), "+v"(qenvC.x), "+v"(qlightC.x),
                          "+v"(qhit.x), "+v"(o0), "+v"(o1), "+v"(qhit2.x));
    else
    asm volatile("" : "+v"(rng), "+v"(qro.x), "+v"(qrd.x), "+v"(qrad.x), "+v"(qthr.x), "+v"(qcol.x), "+v"(qenvC.x), "+v"(qlightC.x), "+v"(qpthr.x),
                      "+v"(qhit.x), "+v"(o0), "+v"(o1), "+v"(qhit2.x));
    if constexpr (PACKED) { rng = pt_asuint(qrad.w); qpthr = make_float4(qenvC.w, qlightC.w, qthr.w, 0.0f); }
    PathRegs r;
    r.state = fl_state(f);
    r.hasPending = fl_pending(f);
    r.env.valid = fl_env(f);
    r.light.valid = fl_light(f);
    r.green = (f >> 6) & 1u;
    r.sampleIdx = (f >> 7) & 0xFFFu;
    r.depth = f >> 19;
    r.rng = rng;
    r.ro = xyz(qro); r.scatterPdf = qro.w;
    r.rd = xyz(qrd); r.maxRoughness = qrd.w;
    r.radiance = xyz(qrad);
    r.throughput = xyz(qthr);
    r.color = xyz(qcol);
    r.env.dir = mk3(0.0f); r.light.dir = mk3(0.0f); r.neeOrigin = mk3(0.0f);
    r.env.contribution = r.hasPending ? xyz(qenvC) : mk3(0.0f);
    r.light.contribution = r.hasPending ? xyz(qlightC) : mk3(0.0f);
    r.pendThroughput = r.hasPending ? xyz(qpthr) : mk3(0.0f);
    const bool occEnv = r.hasPending && o0 != 0u, occLight = r.hasPending && o1 != 0u;
    HitRecord ch;
    ch.h.t = PT_FAR_PLANE; ch.h.u = 0.0f; ch.h.v = 0.0f; ch.h.triIndex = 0u;
    ch.pos = mk3(0.0f); ch.inst = 0u;
    if (r.state == PS_TRACE) {
        ch.h.t = qhit.x; ch.h.u = qhit.y; ch.h.v = qhit.z; ch.h.triIndex = pt_asuint(qhit.w);
        if (S.hasTlas) { ch.pos = xyz(qhit2); ch.inst = pt_asuint(qhit2.w); }
    }
    // the NEE rays of the bounce go to their arrays as soon as they are final (NeeSink): 15 registers free while the BSDF is sampled
    struct Sink {
        const PTWfBuffers& B; uint32_t slot;
        PT_DEV void operator()(PathRegs& q) const {
            uint32_t s2 = slot;
            asm volatile("" : "+v"(s2));
            B.ray[1][2u * s2] = f4(q.neeOrigin, 0.0f);
            B.ray[1][2u * s2 + 1u] = f4(q.env.dir, 0.0f);
            B.ray[2][2u * s2] = f4(q.neeOrigin, 0.0f);
            B.ray[2][2u * s2 + 1u] = f4(q.light.dir, 0.0f);
            B.envC[s2] = f4(q.env.contribution, PACKED ? q.pendThroughput.x : 0.0f);
            B.lightC[s2] = f4(q.light.contribution, PACKED ? q.pendThroughput.y : 0.0f);
            if constexpr (!PACKED) B.pthr[s2] = f4(q.pendThroughput, 0.0f);
        }
    };
    // PACKED: whether the step changes color.  Keeping the three loaded words to the end for that would cost three registers
    // across sample_brdf, and the kernel sits on its 128-VGPR line.  Only a fold changes color, and a step folds in two places:
    // in path_step's head (the deferred finish of an overlapped sample) and in its path_end_sample.  So the head is run HERE --
    // the same calls in the same order; path_step then finds nothing pending and no overlapped state, and its own head does
    // nothing -- and color is compared once after it and once at the end, each time against the value it had just before.
    // The result is ONE word, non-zero iff a word of color changed, pinned so that it is formed there and the old color dies.
    [[maybe_unused]] uint32_t colorDiff = 0u;
    [[maybe_unused]] v3 colorBefore = r.color;
    if constexpr (PACKED) {
        const bool deferred = path_overlapped(r);
        path_apply_pending(r, occEnv, occLight);
        if (deferred) {
            path_fold_sample(P, r);
            path_reset_sample(r);
        }
        colorDiff = differing_bits(r.color, colorBefore);
        asm volatile("" : "+v"(colorDiff));
        colorBefore = r.color;
    }
    // OVERLAP (pt_device.h): a sample that ends with its NEE pending starts its successor's ray in this step, so the slot's next
    // trace round carries the camera ray next to the two shadow rays instead of the shadow rays alone
    if constexpr (kRayMap<MAP>)
        path_step<STATS, false, Sink, RaySample, true>(S, P, r, ch, occEnv, occLight, 0u, 0u, 0u, nullptr, nullptr, cn, Sink{B, slot}, RaySample{tm.rays, pixelSlot});
    else
        path_step<STATS, false, Sink, CameraSample, true>(S, P, r, ch, occEnv, occLight, px, py, py * P.OutputWidth + px, nullptr, nullptr, cn, Sink{B, slot});
    // the store addresses are formed HERE from a slot the compiler cannot connect with the one the loads used: otherwise the
    // thirteen 64-bit load addresses stay in registers across the whole step to be reused by these stores
    uint32_t storeSlot = slot;
    asm volatile("" : "+v"(storeSlot));
    if constexpr (PACKED) {
        B.flags[storeSlot] = pack_flags(r);
        if (r.state != PS_DONE) {
            B.ray[0][2u * storeSlot] = f4(r.ro, r.scatterPdf);
            B.ray[0][2u * storeSlot + 1u] = f4(r.rd, r.maxRoughness);
            B.rad[storeSlot] = f4(r.radiance, pt_asfloat(r.rng));
            B.thr[storeSlot] = f4(r.throughput, r.pendThroughput.z);
            if ((colorDiff | differing_bits(r.color, colorBefore)) != 0u) B.color[storeSlot] = f4(r.color, 0.0f);
        }
    } else
    store_path(B, storeSlot, r, false);                             // the NEE arrays were written by the sink
    if (PIXSUM && r.state == PS_DONE) {
        uint32_t ps = pixelSlot;
        asm volatile("" : "+v"(ps));
        B.pixsum[ps] = f4(r.color, 0.0f);
    }
    return r.state != PS_DONE;
}

#ifndef PT_WF_SHADE_BLOCK
#define PT_WF_SHADE_BLOCK 64u          // one wave per workgroup: a finished wave frees its 128 VGPRs at once (256 -> 64: +4 %)
#endif
// The body of the cleanup kernels: pixels still alive after the fixed number of iterations are run to completion, one lane per
// slot with the megakernel's loop (trace <= 3 rays, path_step, repeat).  Normally a handful of lanes; correctness for any path length.
// REPACK: the pixel of a slot is B.pixelOf's, its sample sum goes to B.pixsum[that pixel slot], and its state is read from the
// packed layout of a repacked sequence (pt_repack.hip, pt_wf_state.h).
template <bool STATS, bool TLAS, bool REPACK, class MAP>
PT_DEV void cleanup_slots(const DScene& S, const PTFrameParams& P, const MAP& tm, const PTWfBuffers& B, uint2 (&s_stack)[PT_LDS_STACK][256])
{
    Counters cn = {};
    // a few resident workgroups stride over the slot blocks: almost every block is finished already, and scanning 256 flag
    // words is cheaper than scheduling a 24-KB-LDS workgroup for them
    for (uint32_t blk = blockIdx.x; blk < (B.numSlots >> 8); blk += gridDim.x) {
    const uint32_t slot = blk * 256u + threadIdx.x;
    const uint32_t f = B.flags[slot];
    if (__any(fl_state(f) != PS_DONE)) {
        if (fl_state(f) != PS_DONE) {
            uint32_t px, py, pass, base;
            const uint32_t pixelSlot = REPACK ? B.pixelOf[slot] : slot;
            wf_pixel(tm, B, pixelSlot, blk * 256u, px, py, pass, base);
            PathRegs r;
            load_path<REPACK>(B, slot, f, r);
            if (r.hasPending) {
                r.neeOrigin = xyz(B.ray[1][2u * slot]);
                r.env.dir = xyz(B.ray[1][2u * slot + 1u]);
                r.light.dir = xyz(B.ray[2][2u * slot + 1u]);
            }
            TravStack st;
            st.lds = PT_LDS_U2(&s_stack[0][threadIdx.x]);
            st.stride = 256u;
            while (r.state != PS_DONE) {
                HitRecord ch;
                ch.h.t = PT_FAR_PLANE; ch.h.u = 0.0f; ch.h.v = 0.0f; ch.h.triIndex = 0u;
                ch.pos = mk3(0.0f); ch.inst = 0u;
                bool occEnv = false, occLight = false;
                if (r.hasPending && r.env.valid != 0u) {
                    HitRecord h = ch;
                    if (TLAS) occEnv = traverse_tlas<STATS>(S, r.neeOrigin, r.env.dir, true, h, st, cn);
                    else { traverse_cwbvh<STATS>(S, r.neeOrigin, r.env.dir, true, h.h, st, cn); occEnv = h.h.t < PT_FAR_PLANE; }
                    cn.shadowRays++;
                }
                if (r.hasPending && r.light.valid != 0u) {
                    HitRecord h = ch;
                    if (TLAS) occLight = traverse_tlas<STATS>(S, r.neeOrigin, r.light.dir, true, h, st, cn);
                    else { traverse_cwbvh<STATS>(S, r.neeOrigin, r.light.dir, true, h.h, st, cn); occLight = h.h.t < PT_FAR_PLANE; }
                    cn.shadowRays++;
                }
                if (r.state == PS_TRACE) {
                    if (TLAS) traverse_tlas<STATS>(S, r.ro, r.rd, false, ch, st, cn);
                    else traverse_cwbvh<STATS>(S, r.ro, r.rd, false, ch.h, st, cn);
                    cn.closestRays++;
                }
                // OVERLAP: a slot can arrive with the previous sample's finish pending (all three rays above exist for it), and
                // the loop may as well go on the way the shade kernel would have
                if constexpr (kRayMap<MAP>)
                    path_step<STATS, false, NoNeeSink, RaySample, true>(S, P, r, ch, occEnv, occLight, 0u, 0u, 0u, nullptr, nullptr, cn, NoNeeSink(), RaySample{tm.rays, slot});
                else
                    path_step<STATS, false, NoNeeSink, CameraSample, true>(S, P, r, ch, occEnv, occLight, px, py, py * P.OutputWidth + px, nullptr, nullptr, cn);
            }
            B.flags[slot] = pack_flags(r);
            if (REPACK) B.pixsum[pixelSlot] = f4(r.color, 0.0f); else
            B.color[slot] = f4(r.color, 0.0f);
            if constexpr (kRayMap<MAP>) B.rng[slot] = r.rng;           // a query returns the RNG state; a frame's resolve never reads it
        }
    }
    }
    flush_counters<STATS>(cn, B.statRows, blockIdx.x * 4u + (threadIdx.x >> 6), threadIdx.x & 63u);
}

} // namespace
