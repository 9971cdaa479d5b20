// pt_wavefront.hip — schedules 1-4: the same per-pixel program as the megakernel, cut at the traversal calls.
//
// Why: in one fused kernel the Disney-BSDF shading code sets the register budget (185 VGPRs -> 2 waves/SIMD, or
// 128 with spills -> 4), and lanes that shade wait for lanes that traverse and vice versa (measured VALU lane
// utilisation 19 %).  Here every pixel owns a SLOT of path state in HBM and a pass is
//     init                     camera ray of the first sample into every slot
//     N x [ trace ; shade ]    trace: lean CWBVH traversal only, 8 waves/SIMD, rays compacted into lanes per wave;
//                              shade: path_step() of pt_device.h (apply NEE, shade, roulette, next sample)
//     cleanup                  lanes whose pixel is still alive after N iterations run it to completion megakernel-style
//     resolve                  out = (sum + accumulated * CurrentSample) / (CurrentSample + spp)   (PathTracer.compute:89-98)
// Samples of a pixel stay sequential (one RNG chain per pixel per pass, PathTracer.compute:60,66), so a slot carries one
// path at a time and a pass needs about SamplesPerPass x (bounces + 2) iterations.  N is that bound; pixels that need
// more (alpha-skips add iterations without adding depth) are finished by the cleanup kernel, so a pass is a fixed,
// HOST-SYNC-FREE sequence of launches.  Because the pixel write is decoupled (resolve), pass k+1 can start tracing on a
// second state set and stream while pass k is still draining; only the tiny resolve kernels are ordered.
//
// There are NO queues and NO global atomics in schedule 1: rays are found by scanning the slot-indexed flag words,
// results go to slot-indexed arrays, work counters accumulate in per-wave rows (plain read-modify-write: one wave owns
// a row) and are folded once per pass.  Every fp32 value and RNG draw is produced by the same device functions in the
// same per-path order as in schedule 0, so frames and counters are bit-identical between schedules and to the oracle.
#include "pt_device.h"
#include "pt_launch.h"
#include "pt_wf_state.h"
#include "pt_wf_shade.h"
#include "pt_compact.h"                        // rank_below
#include "repack_rule.h"
#include <type_traits>

namespace {

#define PT_WF_CHUNK 64u         // slots per work chunk of the persistent trace kernel (= one scan window per ray kind)

template <class MAP = PTTileMap>
__global__ __launch_bounds__(256) void pt_wf_init(PTFrameParams P, PTBatch batch, MAP tm, PTWfBuffers B)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0u && threadIdx.x < PT_WF_SHARDS) B.chunkHeads[threadIdx.x * 32u] = 0u;
    if (slot >= B.numSlots) return;
    if constexpr (!kListMap<MAP> && !kRayMap<MAP>) B.pixelOf[slot] = slot;      // a repack moves a path away from its pixel's slot (pt_repack.hip)
    uint32_t px, py, pass, base;
    Counters cn = {};
    if (!wf_pixel(tm, B, slot, blockIdx.x * 256u, px, py, pass, base)) B.flags[slot] = PS_DONE;
    else {
        PathRegs r;
        if constexpr (kRayMap<MAP>) ray_path_init(tm, slot, r, cn);
        else {
            uint32_t seedRoot, currentSample;
            pt_batch_pick(batch, pass, seedRoot, currentSample);
            if (kListMap<MAP>) currentSample = base + pass * (P.SamplesPerPass > 1 ? (uint32_t)P.SamplesPerPass : 1u);
            path_init(P, seedRoot, currentSample, px, py, py * P.OutputWidth + px, r, cn);
        }
        // over the frame's own blocks the sequence may be a repacked one, which keeps the RNG state in rad.w (pt_wf_state.h)
        store_path(B, slot, r, false, !kListMap<MAP> && !kRayMap<MAP> ? pt_asfloat(r.rng) : 0.0f);
    }
    // every lane of the wave takes part in the reduction (a lane that had returned would be read as garbage)
    flush_counters<false>(cn, B.statRows, blockIdx.x * 4u + (threadIdx.x >> 6), threadIdx.x & 63u);
}

// ------------------------------------------------------------------------------------------
// trace: one lane per (slot, kind).  kind 0 = closest hit of the bounce ray, 1 = environment NEE, 2 = light NEE
// ------------------------------------------------------------------------------------------
#ifndef PT_WF_TRACE_MIN_WAVES
#define PT_WF_TRACE_MIN_WAVES 8
#endif

template <bool STATS, bool TLAS>
__global__ __launch_bounds__(256, 4) void pt_wf_trace(DScene S, PTWfBuffers B, uint32_t iteration)
{
    __shared__ uint2 s_stack[PT_LDS_STACK][256];
    const uint32_t nb = B.numSlots >> 8;
    const uint32_t vb = blockIdx.x;
    const uint32_t kind = vb / nb;
    const uint32_t slot = (vb % nb) * 256u + threadIdx.x;
    const uint32_t f = B.flags[slot];
    bool valid;
    if (kind == 0u) valid = fl_state(f) == PS_TRACE;
    else if (kind == 1u) valid = fl_pending(f) && fl_env(f) != 0u;
    else valid = fl_pending(f) && fl_light(f) != 0u;
    Counters cn = {};
    if (valid) {
        v3 o, d;
        fetch_ray(B, slot, kind, o, d);
        TravStack st;
        st.lds = PT_LDS_U2(&s_stack[0][threadIdx.x]);
        st.stride = 256u;
        HitRecord h;
        h.h.t = PT_FAR_PLANE; h.h.u = 0.0f; h.h.v = 0.0f; h.h.triIndex = 0u;
        h.pos = mk3(0.0f); h.inst = 0u;
        bool occluded;
        if (TLAS) occluded = traverse_tlas<STATS>(S, o, d, kind != 0u, h, st, cn);
        else { traverse_cwbvh<STATS>(S, o, d, kind != 0u, h.h, st, cn); occluded = h.h.t < PT_FAR_PLANE; }
        if (kind == 0u) {
            B.hit[slot] = make_float4(h.h.t, h.h.u, h.h.v, pt_asfloat(h.h.triIndex));
            if (TLAS) B.hit2[slot] = make_float4(h.pos.x, h.pos.y, h.pos.z, pt_asfloat(h.inst));
            cn.closestRays++;
        } else { B.occl[(size_t)(kind - 1u) * B.numSlots + slot] = occluded ? 1 : 0; cn.shadowRays++; }
    }
    flush_counters<STATS>(cn, B.statRows, (B.numSlots >> 6) + vb * 4u + (threadIdx.x >> 6), threadIdx.x & 63u);
}

// ------------------------------------------------------------------------------------------
// trace with refill (schedule 1): persistent-threads ray scheduling inside each wave, no atomics.
//
// A wave owns PT_WF_RANGE consecutive slots = 3 * PT_WF_RANGE potential rays, enumerated kind-major (all bounce
// rays of the range, then the environment shadow rays, then the light shadow rays: neighbours in the enumeration are
// neighbours on screen and of one kind, i.e. as coherent as this path tracer gets).  The wave keeps 64 resumable
// traversals in flight.  The main launch reads its range's flag words once, when the wave starts (one or two coalesced
// loads per lane, requested together), ballots which rays exist kind by kind and writes them, in enumeration order, into
// a list of 16-bit items in LDS (3 * RANGE entries: 768 bytes, 4,868 per workgroup, under the 5,120 that 32 workgroups
// per CU allow).  Whenever PT_WF_REFILL or more lanes have retired their ray, the idle lane of rank r takes
// list[cursor + r]: a refill round is one ballot, one rank and one LDS read in front of the ray fetch, no flag load.
// (Before the list every round scanned the next 64 candidates' flag words and compacted them through a 64-entry LDS
// exchange -- compact_candidates, which the HAS_TLAS, persistent and fused kernels still use -- and a steady-phase
// range of ~340 rays was scanned about 19 times; profiles/trace_candidate_list_ab.md.)  Rays of very different length
// never hold a wave hostage, and the enumeration order -- hence every result -- is independent of timing.
// ------------------------------------------------------------------------------------------
#ifndef PT_WF_RANGE
#define PT_WF_RANGE 128u        // largest slots-per-wave the launcher may pick (power of two): two 8x8 tiles x 3 kinds = 384 candidate rays.
                                // Full 1080p frame, 64 / 128 / 256: 4,590 / 4,700 / 4,690 Mrays/s; small launches use 64 (pt_launch_wavefront)
#endif
#define PT_WF_STAT_ROW_SETS 4u   // statRows holds this many x numSlots/64 counter rows (pt_wf_arena_layout)
static_assert(PT_WF_RANGE >= 64u && (PT_WF_RANGE & (PT_WF_RANGE - 1u)) == 0u && PT_WF_STAT_ROW_SETS >= 3u,
              "one counter row per trace wave: the main trace launch uses rows numSlots/64 + wave, the tail launch rows 2 x numSlots/64 + wave");
static_assert(3u * PT_WF_RANGE <= 65535u, "an item of the main launch's candidate list (kind * RANGE + offset) is a uint16_t");
#ifndef PT_WF_REFILL
#define PT_WF_REFILL 16u        // refill when at least this many lanes are idle (with the candidate list: 8 / 12 / 16 / 24 read 5,907 / 5,948 / 5,914-5,953 / 5,859 Mrays/s)
#endif
#ifndef PT_WF_TRI_PARK
#define PT_WF_TRI_PARK 4u       // two-phase wave iteration (ray_tri_one / ray_node_one): lanes with triangles pending wait until that many lanes
                                // do.  2 ... 12 measure the same (+6 % over ray_step's nested loops), 16: +3 %, 24: -2 %
#endif

// LDS words the lanes of a wave exchange through, as LDS-address-space pointers: through a generic `volatile uint32_t*` every
// access is a FLAT instruction (the compiler does not infer the address space of a volatile access) -- it travels the
// texture-address path and counts against both memory counters.
typedef volatile __attribute__((address_space(3))) uint32_t* pt_lds_u32;
typedef volatile __attribute__((address_space(3))) uint16_t* pt_lds_u16;

// Result stores of the trace kernels.  The empty asm pins the address arithmetic (and the constant miss record) to the
// store instead of letting it be hoisted into registers that live across the whole traversal loop (64-VGPR budget).
PT_DEV void store_miss(const PTWfBuffers& B, uint32_t slot)
{
    float far = PT_FAR_PLANE;
    asm volatile("" : "+v"(far), "+v"(slot));
    f4_array(B, PT_F4_HIT)[slot] = make_float4(far, 0.0f, 0.0f, 0.0f);
}
// (the pin matters for the hit record as well: with its address hoisted out of the loop that finishes slab rays, the statistics
// instantiations of the refill kernel spilled it -- 12 bytes of scratch)
PT_DEV void store_hit(const PTWfBuffers& B, uint32_t slot, const TraceHit& hit)
{
    asm volatile("" : "+v"(slot));
    f4_array(B, PT_F4_HIT)[slot] = make_float4(hit.t, hit.u, hit.v, pt_asfloat(hit.triIndex));
}
PT_DEV void store_occlusion(const PTWfBuffers& B, uint32_t kind, uint32_t slot, bool occluded)
{
    asm volatile("" : "+v"(kind), "+v"(slot));
    B.occl[(size_t)(kind - 1u) * B.numSlots + slot] = occluded ? 1 : 0;
}

PT_DEV bool ray_exists(uint32_t f, uint32_t kind)
{
    if (kind == 0u) return fl_state(f) == PS_TRACE;
    if (kind == 1u) return fl_pending(f) && fl_env(f) != 0u;
    return fl_pending(f) && fl_light(f) != 0u;
}

// ---- the wave scheduler ------------------------------------------------------------------------------------------------
// What the trace kernels that keep 64 resumable traversals in flight per wave share (pt_wf_trace_refill, pt_wf_trace_refill_tlas,
// pt_wf_trace_persist, the trace phase of pt_wf_fused).  Each kernel enumerates its own candidates (slot range, chunk, context
// group, pend mask) and owns its loop; the steps of the loop are written once, here and under "suspension" below.

// Compaction of up to 64 candidates into the idle lanes: the lanes whose candidate exists (`valid`) put its `word` into xchg in
// enumeration order, as many as there are idle lanes; afterwards an idle lane with rankI < take owns xchg[rankI].  consumed: how far
// the caller's cursor moves (up to the first ray NOT taken).  The caller puts a wave barrier behind its reads of xchg.
struct Compaction { uint32_t take, consumed, rankI; };
PT_DEV Compaction compact_candidates(pt_lds_u32 xchg, bool idle, uint32_t nIdle, bool valid, uint32_t word)
{
    Compaction c;
    c.rankI = rank_below(__ballot(idle));
    const unsigned long long V = __ballot(valid);
    const uint32_t nV = (uint32_t)__popcll(V);
    c.take = nIdle < nV ? nIdle : nV;
    const uint32_t rankV = rank_below(V);
    c.consumed = 64u;
    if (c.take < nV) c.consumed = (uint32_t)__ffsll((long long)__ballot(valid && rankV == c.take)) - 1u;   // first ray NOT taken
    if (valid && rankV < c.take) xchg[rankV] = word;
    __builtin_amdgcn_wave_barrier();
    return c;
}

// The result of a finished ray.  Closest hit (kind 0): the miss record or (t, u, v, triIndex); shadow ray: the occlusion byte.
// recordStored: the hit record is in memory already (kernels that write it at every improvement), so only a miss is stored.
PT_DEV void store_result(const PTWfBuffers& B, uint32_t slot, uint32_t kind, bool hitAny, const TraceHit& hit, bool recordStored)
{
    if (kind == 0u) {
        if (!hitAny) store_miss(B, slot);
        else if (!recordStored) store_hit(B, slot, hit);
    } else store_occlusion(B, kind, slot, hitAny);
}

// A lane takes the ray (slot, kind) of a flat scene.  false: a NaN ray, a certain miss -- its result is stored and the lane stays idle.
PT_DEV bool start_ray(const PTWfBuffers& B, uint32_t slot, uint32_t kind, RayState& rs, Counters& cn)
{
    v3 o, d;
    fetch_ray(B, slot, kind, o, d);
    if (kind == 0u) cn.closestRays++; else cn.shadowRays++;
    rs.hit = TraceHit{PT_FAR_PLANE, 0.0f, 0.0f, 0u};
    if (!ray_begin(rs, o, d, kind != 0u)) return true;
    store_result(B, slot, kind, false, rs.hit, true);
    return false;
}

// Two phases per wave iteration instead of ray_step's nested loops: (1) every lane with a triangle pending tests ONE
// (the block runs when PT_WF_TRI_PARK lanes want it, or when nobody can do anything else), (2) every lane without a
// triangle pending -- including those that have just tested their last one -- pops and visits its next node.  A lane
// with k triangles spends k - 1 extra iterations in phase 1 while its neighbours keep visiting nodes; the triangle
// block runs once per iteration at ~3x the lane utilisation of the nested loop (2.1 executions at 8 %).
// Returns true when the lane's ray is complete.
template <bool STATS, class ST>
PT_DEV bool wave_step(const DScene& S, bool have, RayState& rs, ST& st, Counters& cn)
{
    const bool wantTri = have && rs.tg.y != 0u;
    const uint32_t nT = (uint32_t)__popcll(__ballot(wantTri));
    const uint32_t nN = (uint32_t)__popcll(__ballot(have && !wantTri));
    bool fin = false;
    if ((nT >= PT_WF_TRI_PARK || nN == 0u) && wantTri) fin = ray_tri_one<STATS>(S, rs, cn);
    if (have && !fin && rs.tg.y == 0u) fin = ray_node_one<STATS>(S, rs, st, cn);
    return fin;
}

// Before a wave parks its rays: a ray whose stack reaches into the HBM slab stays (a record only holds the LDS entries), so those
// are finished first.  Returns the lane's `have`.
template <bool STATS, class ST>
PT_DEV bool finish_slab_rays(const DScene& S, const PTWfBuffers& B, bool have, uint32_t slot, uint32_t kind, RayState& rs, ST& st, Counters& cn)
{
    if (__ballot(have && rs.sp > PT_WF_LDS_STACK) != 0ull)                  // (spelled out: without it the main refill kernel comes to 63 VGPRs and 1,558 instructions instead of 58 and 1,507)
    while (__ballot(have && rs.sp > PT_WF_LDS_STACK) != 0ull) {
        if (have) {
            // a lane may arrive with triangles pending: one triangle OR one node visit, whichever is next for it
            const bool fin = rs.tg.y != 0u ? ray_tri_one<STATS>(S, rs, cn) : ray_node_one<STATS>(S, rs, st, cn);
            if (fin) {
                store_result(B, slot, kind, rs.hit.t < PT_FAR_PLANE, rs.hit, false);
                have = false;
            }
        }
    }
    return have;
}

// ---- suspension (PT_WF_SUSPEND > 0) -----------------------------------------------------------------------------------
// A launch only holds 5-6 rays per lane of the chip, and ray lengths spread over an order of magnitude, so a wave spends
// most of its iterations DRAINING: measured on the Sponza-class pass, 54 % of all wave iterations ran after the wave's
// range was exhausted and 32 % with <= 16 active lanes, each costing the same ~450 VALU instructions and memory round
// trips as a full one.  So a wave whose range is exhausted stops as soon as PT_WF_SUSPEND or fewer rays are left: it
// writes those rays' traversal state (node group, triangle group, stack, t: 96 bytes) to a record array and exits, and a
// TAIL launch of the same kernel packs the records of PT_WF_TAIL_GROUP consecutive waves into full waves and resumes
// them.  A ray resumes exactly where it stopped, so results and counters are unchanged; late, sparse iterations (a
// handful of rays per 64-slot range) become a cheap scan + an 8:1 compacted tail.
// PT_WF_SUSPEND (pt_launch.h, default 16; 0 = off)
#ifndef PT_WF_TAIL_GROUP
#define PT_WF_TAIL_GROUP 8u     // source waves per tail wave
#endif
#define PT_WF_SUSP_STACK_ROWS ((PT_WF_LDS_STACK + 1u) / 2u)       // two stack entries per uint4 row
#define PT_WF_SUSP_ROWS (2u + PT_WF_SUSP_STACK_ROWS)             // uint4 rows per record (6 = 96 bytes with the default 8-entry LDS stack)
#define PT_WF_SUSP_RECORD_ROWS 6u                                // uint4 rows a record has room for (pt_wf_arena_layout)
static_assert(PT_WF_SUSP_ROWS <= PT_WF_SUSP_RECORD_ROWS, "a suspended ray's record does not fit its slot of the record array");

// The record p of a suspended ray, in the record array of the refill kernel (B.susp) or in the LDS of the fused kernel.
// ref: kind << 30 | the ray's slot (refill) or its context index within the wave (fused).
// A record holds the LDS part of the stack; a ray whose stack reaches into the HBM slab is not suspended (it is finished first).
template <class ST>
PT_DEV void suspend_ray(uint4* p, uint32_t ref, const RayState& r, ST& st)
{
    p[0] = make_uint4(ref, r.sp | (r.overflow ? 0x100u : 0u), r.ng.x, r.ng.y);
    p[1] = make_uint4(r.tg.x, r.tg.y, pt_asuint(r.hit.t), 0u);
#pragma unroll
    for (uint32_t e = 0; e < PT_WF_SUSP_STACK_ROWS; ++e) {
        const pt_u2 x = st.lds[(2u * e) * st.stride];
        const pt_u2 y = (2u * e + 1u < PT_WF_LDS_STACK) ? (pt_u2)st.lds[(2u * e + 1u) * st.stride] : pt_u2{0u, 0u};
        p[2u + e] = make_uint4(x.x, x.y, y.x, y.y);
    }
}
// The lane resumes the ray of record p and returns its ref; slotBase + (ref & 0x3FFFFFFF) is the ray's slot.  Only t of the hit is
// in a record: the best hit so far was left in the hit array.
template <class ST>
PT_DEV uint32_t resume_ray(const PTWfBuffers& B, const uint4* p, uint32_t slotBase, RayState& rs, ST& st)
{
    const uint4 a = p[0], b = p[1];
    uint4 er[PT_WF_SUSP_STACK_ROWS];
#pragma unroll
    for (uint32_t e = 0; e < PT_WF_SUSP_STACK_ROWS; ++e) er[e] = p[2u + e];
    const uint32_t kind = a.x >> 30;
    v3 o, d;
    fetch_ray(B, slotBase + (a.x & 0x3FFFFFFFu), kind, o, d);
    ray_begin(rs, o, d, kind != 0u);                                  // same invDir / octinv4 as when the ray started
    rs.sp = a.y & 0xFFu;
    rs.overflow = (a.y & 0x100u) != 0u;
    rs.ng = make_uint2(a.z, a.w);
    rs.tg = make_uint2(b.x, b.y);
    rs.hit = TraceHit{pt_asfloat(b.z), 0.0f, 0.0f, 0u};
#pragma unroll
    for (uint32_t e = 0; e < PT_WF_SUSP_STACK_ROWS; ++e) {
        st.lds[(2u * e) * st.stride] = pt_u2{er[e].x, er[e].y};
        if (2u * e + 1u < PT_WF_LDS_STACK) st.lds[(2u * e + 1u) * st.stride] = pt_u2{er[e].z, er[e].w};
    }
    return a.x;
}

// RANGE: slots per wave (64 or 128; pt_launch_wavefront picks by the size of the launch)
template <bool STATS, bool TAIL, uint32_t RANGE>
__global__ __launch_bounds__(64, PT_WF_TRACE_MIN_WAVES) void pt_wf_trace_refill(DScene S, PTWfBuffers B, uint32_t iteration)
{
    __shared__ uint2 s_stack[PT_WF_LDS_STACK][64];
    // tail launch: the packed record indices (32 bits each); main launch: the candidate list, 3 * RANGE items of 16 bits
    __shared__ uint32_t s_xchg[TAIL ? PT_WF_TAIL_GROUP * (PT_WF_SUSPEND ? PT_WF_SUSPEND : 1u) : 3u * RANGE / 2u];
    static_assert(TAIL || sizeof(s_stack) + sizeof(s_xchg) + sizeof(uint32_t) <= 5120u, "32 one-wave workgroups per CU must fit 160 KB of LDS: 5,120 bytes each");
    // the wave's counter row is parked in LDS until the end: kept in a register it is the one value the compiler spilled to
    // scratch, and ANY scratch costs this kernel its occupancy (see TravStackT)
    __shared__ uint32_t s_gw;
    const uint32_t lane = threadIdx.x;
    const uint32_t gw = blockIdx.x;
    const uint32_t numWaves = (B.numSlots + RANGE - 1u) / RANGE;
    const uint32_t slotBase = gw * RANGE;
    pt_lds_u32 xchg = (pt_lds_u32)&s_xchg[0];
    if (lane == 0u) s_gw = gw;

    // candidates: the main launch reads the flag words of its slot range ONCE and lists the rays that exist, kind-major, in s_xchg
    // (16-bit items, kind * RANGE + offset); the tail launch walks the records that its PT_WF_TAIL_GROUP source waves left behind
    // (their indices, packed, in s_xchg).  Either way a refill round hands list[cursor ...] to the idle lanes in order.
    uint32_t nItems = 0u;
    if (!TAIL) {
        const pt_lds_u16 list = (pt_lds_u16)&s_xchg[0];
        constexpr uint32_t kWords = RANGE / 64u;                      // flag words per lane: both loads are requested together
        uint32_t f[kWords];
        bool in[kWords];
#pragma unroll
        for (uint32_t w = 0; w < kWords; ++w) {
            const uint32_t slot = slotBase + w * 64u + lane;
            in[w] = slot < B.numSlots;
            f[w] = in[w] ? B.flags[slot] : 0u;
        }
#pragma unroll
        for (uint32_t kind = 0; kind < 3u; ++kind) {
#pragma unroll
            for (uint32_t w = 0; w < kWords; ++w) {
                const bool valid = in[w] && ray_exists(f[w], kind);
                const unsigned long long V = __ballot(valid);
                if (valid) list[nItems + rank_below(V)] = (uint16_t)(kind * RANGE + w * 64u + lane);
                nItems += (uint32_t)__popcll(V);                      // wave-uniform: the number of rays so far
            }
        }
        __builtin_amdgcn_wave_barrier();                              // no ray of the range: the loop below falls through to the zero report
    } else {
        const uint32_t s0 = gw * PT_WF_TAIL_GROUP;
        uint32_t c = 0u;
        if (lane < PT_WF_TAIL_GROUP && s0 + lane < numWaves) c = B.suspCount[s0 + lane];
        uint32_t incl = c;                                            // inclusive prefix over lanes 0..PT_WF_TAIL_GROUP-1
#pragma unroll
        for (uint32_t off = 1u; off < PT_WF_TAIL_GROUP; off <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64); if (lane >= off) incl += o; }
        nItems = (uint32_t)__shfl((int)incl, (int)PT_WF_TAIL_GROUP - 1, 64);
        constexpr uint32_t kT = PT_WF_SUSPEND ? PT_WF_SUSPEND : 1u;
#pragma unroll
        for (uint32_t r = 0; r < (PT_WF_TAIL_GROUP * kT + 63u) / 64u; ++r) {
            const uint32_t q = r * 64u + lane, i = q / kT, k = q % kT;
            const uint32_t ci = (uint32_t)__shfl((int)c, (int)(i & 63u), 64), pi = (uint32_t)__shfl((int)(incl - c), (int)(i & 63u), 64);
            if (i < PT_WF_TAIL_GROUP && k < ci) xchg[pi + k] = (s0 + i) * kT + k;
        }
        __builtin_amdgcn_wave_barrier();
        if (nItems == 0u) return;                                     // wave-uniform; nothing was counted
    }

    Counters cn = {};
    TravStackT<PT_WF_LDS_STACK, true> st;
    st.lds = PT_LDS_U2(&s_stack[0][lane]);
    st.stride = 64u;
    st.gbase = B.stackSpill;
    st.gwave = PT_LDS_WORD(s_gw);                                                 // slab row = wave * 64 + lane < numSlots
    RayState rs;
    rs.sp = 0u; rs.anyHit = false; rs.overflow = false;
    bool have = false;
    uint32_t mySlot = 0u, myKind = 0u;
    uint32_t cursor = 0u, nSuspended = 0u;

    while (true) {
        uint32_t nIdle = (uint32_t)__popcll(__ballot(!have));
        // ---- refill: compact the next candidates into the idle lanes
        while (cursor < nItems && (nIdle >= PT_WF_REFILL || nIdle == 64u)) {
            if (!TAIL) {
                const uint32_t rankI = rank_below(__ballot(!have));
                const uint32_t left = nItems - cursor;
                const uint32_t take = nIdle < left ? nIdle : left;
                if (!have && rankI < take) {
                    const uint32_t it = ((pt_lds_u16)&s_xchg[0])[cursor + rankI];
                    myKind = it / RANGE;
                    mySlot = slotBase + (it & (RANGE - 1u));
                    have = start_ray(B, mySlot, myKind, rs, cn);
                }
                cursor += take;
            } else {
                const uint32_t rankI = rank_below(__ballot(!have));
                const uint32_t left = nItems - cursor;
                const uint32_t take = nIdle < left ? nIdle : left;
                if (!have && rankI < take) {
                    mySlot = resume_ray(B, B.susp + (size_t)xchg[cursor + rankI] * PT_WF_SUSP_ROWS, 0u, rs, st);
                    myKind = mySlot >> 30;
                    mySlot &= 0x3FFFFFFFu;
                    have = true;
                }
                cursor += take;
            }
            nIdle = (uint32_t)__popcll(__ballot(!have));
        }
        if (nIdle == 64u) break;                                      // candidates exhausted and nothing in flight
        // ---- traverse until enough lanes have retired; once the candidates are exhausted, until PT_WF_SUSPEND or fewer rays
        //      are left (main launch) or all have finished (tail launch)
        const bool exhausted = cursor >= nItems;
        const uint32_t stopAt = !exhausted ? PT_WF_REFILL : ((!TAIL && PT_WF_SUSPEND > 0u) ? 64u - PT_WF_SUSPEND : 64u);
        while (nIdle < stopAt) {
            const float tBefore = rs.hit.t;
            const bool fin = wave_step<STATS>(S, have, rs, st, cn);
            // TAIL: the hit record goes to memory when a test improved it (a resumed ray has only t in registers).
            // main launch: (u, v, triIndex) stay in registers and are written once, when the ray finishes or is suspended
            if (TAIL && myKind == 0u && rs.hit.t < tBefore) f4_array(B, PT_F4_HIT)[mySlot] = make_float4(rs.hit.t, rs.hit.u, rs.hit.v, pt_asfloat(rs.hit.triIndex));
            if (fin) {
                store_result(B, mySlot, myKind, rs.hit.t < PT_FAR_PLANE, rs.hit, TAIL);
                have = false;
            }
            nIdle = (uint32_t)__popcll(__ballot(!have));
        }
        if (!TAIL && PT_WF_SUSPEND > 0u && exhausted && nIdle < 64u) {
            have = finish_slab_rays<STATS>(S, B, have, mySlot, myKind, rs, st, cn);
            const unsigned long long act = __ballot(have);
            // a suspended bounce ray leaves its best hit so far in the hit array (the tail launch writes there only when it improves it)
            if (have && myKind == 0u && rs.hit.t < PT_FAR_PLANE) store_hit(B, mySlot, rs.hit);
            if (have) suspend_ray(B.susp + (size_t)(*PT_LDS_WORD(s_gw) * PT_WF_SUSPEND + rank_below(act)) * PT_WF_SUSP_ROWS, mySlot | (myKind << 30), rs, st);
            have = false;
            nSuspended = (uint32_t)__popcll(act);
            break;
        }
    }
    if (!TAIL && PT_WF_SUSPEND > 0u && lane == 0u) B.suspCount[*PT_LDS_WORD(s_gw)] = nSuspended;     // every main wave reports, zero included
    __builtin_amdgcn_wave_barrier();
    flush_counters<STATS>(cn, B.statRows, (TAIL ? 2u : 1u) * (B.numSlots >> 6) + *PT_LDS_WORD(s_gw), lane);
}

// ------------------------------------------------------------------------------------------
// HAS_TLAS through the refill scheduler: traverse_tlas (pt_device.h) cut so that the hot loop of the wave contains ONE kind
// of step, the cwbvh_iteration<INST> of the instance a lane is inside.  Whenever a lane's instance is finished it runs
// instance_exit and walks the 2-wide TLAS -- tlas_node_step, a short, rarely taken loop -- to the next instance whose box it
// hits, which it enters with instance_enter.  The arithmetic and the decisions are those shared functions; what this kernel owns
// is where things live.  Per lane: the BLAS stack in LDS (8 entries, deeper ones in the HBM slab) plus a second, narrow LDS
// stack for TLAS node indices; the world-space ray is re-read from the slot arrays when an instance is entered.  Same per-ray
// operation order as traverse_tlas, so frames and all counters stay bit-identical.
// ------------------------------------------------------------------------------------------
#ifndef PT_WF_TLAS_LDS_STACK
#define PT_WF_TLAS_LDS_STACK 8u
#endif

#ifndef PT_WF_TLAS_CONT
#define PT_WF_TLAS_CONT 16u          // > 1: a lane keeps walking the TLAS within one wave iteration only while at least this many lanes walk with it
                                     // (0 / 4 / 8 / 16 / 24 / 32: 2,070 / 2,091 / 2,124 / 2,130 / 2,097 / 2,049 Mrays/s on the 200-instance scene)
#endif
#ifndef PT_WF_TLAS_MIN_WAVES
#define PT_WF_TLAS_MIN_WAVES 6      // 80 VGPRs, no scratch (without the SLP vectorizer); 5 waves: -3 %
#endif
// WAVES = 1: one-wave workgroups, TLAS nodes fetched from HBM / L2 (round 2).
// WAVES > 1 (round 3, the default for TLAS trees below 65,536 nodes): the WAVES waves of a workgroup share ONE copy of the top of
// the TLAS in LDS -- the first PT_WF_TLAS_CACHE_NODES nodes of S.tlasBfs, the breadth-first renumbering PTSetScene makes of the
// reference's node array (same nodes, same children, same visiting order: only the indices differ, and nothing observable
// depends on them).  The TLAS walk is a chain of ~13 dependent 64-byte fetches per ray at a quarter of the lanes (57 % of this
// kernel's time when they come from memory); from LDS a step costs a ds_read_b128 x 4 instead of a vector-memory round trip
// and takes 52 of the ray's ~145 sixteen-byte lane requests off the texture-address path.  To pay for the 25.6 KB copy at the same
// 24 waves per CU the per-wave LDS shrinks: PT_WF_TLAS_BLAS_LDS_STACK (4) CWBVH stack entries (deeper ones in the HBM slab, as
// before) and 16-bit TLAS stack entries.  Each wave still owns its own slot range and never waits for another after the
// one barrier that follows the copy.
template <bool STATS, uint32_t WAVES>
__global__ __launch_bounds__(64 * WAVES, PT_WF_TLAS_MIN_WAVES) void pt_wf_trace_refill_tlas(DScene S, PTWfBuffers B, uint32_t iteration)
{
    constexpr bool kCached = WAVES > 1u;
    constexpr uint32_t kBlasLds = kCached ? (uint32_t)PT_WF_TLAS_BLAS_LDS_STACK : (uint32_t)PT_WF_LDS_STACK;
    typedef typename std::conditional<kCached, uint16_t, uint32_t>::type tentry_t;
    __shared__ uint2 s_stack[WAVES][kBlasLds][64];
    __shared__ tentry_t s_tstack[WAVES][PT_WF_TLAS_LDS_STACK][64];
    __shared__ uint32_t s_xchg[WAVES][64];
    __shared__ uint32_t s_gw[WAVES];
    __shared__ float4 s_tcache[kCached ? PT_WF_TLAS_CACHE_NODES * 4u : 1u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = kCached ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0u;     // wave-uniform: LDS bases stay scalar
    const uint32_t gw = blockIdx.x * WAVES + wv;
    // WAVES = 1: the wave scans its own PT_WF_RANGE slots.  WAVES > 1: the workgroup's waves SHARE its WAVES x PT_WF_RANGE slots, in
    // chunks of PT_WF_TLAS_CHUNK slots handed out by an LDS counter -- a wave whose chunk is scanned takes the next one while its
    // rays are still in flight, so the waves of a workgroup run out of work together (with a fixed range per wave the workgroup
    // held its LDS and wave slots until its SLOWEST range was done: measured 2.9x slower, 8 waves without the LDS copy).
    constexpr uint32_t kChunk = kCached ? PT_WF_TLAS_CHUNK : PT_WF_RANGE;
    __shared__ uint32_t s_next;
    const uint32_t wgBase = blockIdx.x * WAVES * PT_WF_RANGE;
    uint32_t slotBase = gw * PT_WF_RANGE;
    pt_lds_u32 xchg = (pt_lds_u32)&s_xchg[wv][0];
    typedef typename std::conditional<kCached, pt_lds_u16, pt_lds_u32>::type tlds_t;
    tlds_t tlds = (tlds_t)&s_tstack[wv][0][lane];
    if (lane == 0u) s_gw[wv] = gw;
    const uint32_t nItems = 3u * kChunk;
    const float* T = S.tlasBfs;
    uint32_t cachedNodes = 0u;
    if (kCached) {
        cachedNodes = S.tlasNodeCount < PT_WF_TLAS_CACHE_NODES ? S.tlasNodeCount : PT_WF_TLAS_CACHE_NODES;
        for (uint32_t i = threadIdx.x; i < cachedNodes * 4u; i += 64u * WAVES) s_tcache[i] = ((const float4*)T)[i];
        if (threadIdx.x == 0u) s_next = 0u;
        __syncthreads();
    }

    Counters cn = {};
    TravStackT<kBlasLds, true> st;
    st.lds = PT_LDS_U2(&s_stack[wv][0][lane]);
    st.stride = 64u;
    st.gbase = B.stackSpill;
    st.gwave = PT_LDS_WORD(s_gw[wv]);
    RayState rs;
    rs.sp = 0u; rs.anyHit = false; rs.overflow = false; rs.hitFound = false;
    bool have = false, inBlas = false, needPop = false;
    bool toverflow = false;                                                   // STATS: the ray's TLAS walk dropped an entry
    uint32_t mySlot = 0u, myKind = 0u, cursor = kCached ? nItems : 0u;       // WAVES > 1: no chunk yet
    bool more = kCached;                                                      // chunks may remain (WAVES > 1)
    v3 O = mk3(0.0f), rD = mk3(0.0f);
    uint32_t nodeIndex = 0u, tsp = 0u, nextInst = 0u, instLeft = 0u;
    BlasOffsets off = {0u, 0u, 0u};
    uint32_t instIndex = 0u;

    // The empty asm statements keep the LDS access and the HBM-slab access of an entry in their own branches.  Without them the
    // compiler sinks the two into ONE access through a selected pointer -- a FLAT load / store (round 2's kernel had two of each in
    // its walk loop): a flat access counts against both the vector-memory and the LDS counter, and one that resolves to LDS
    // still travels the texture-address path.
    auto tpush = [&](uint32_t v) {
        if (tsp < PT_WF_TLAS_LDS_STACK) { tlds[tsp * 64u] = (tentry_t)v; asm volatile("" ::: "memory"); }
        else if (tsp < PT_BVH_STACK_SIZE) B.tlasSpill[spill_row(PT_LDS_WORD(s_gw[wv])) * PT_BVH_STACK_SIZE + tsp] = v;
        else if (STATS) toverflow = true;
        tsp++;
    };
    // The pop of the overflow rule (ptmi_plugin.h, Part 3; tlas_stack_pop in pt_device.h): entries at index >= 32 were never stored,
    // yield nothing and popping goes on, so the entry yielded is the one below min(tsp, 32).  false: nothing left, the ray is done.
    // The clamp sits on the slab branch: a pointer below PT_WF_TLAS_LDS_STACK needs none.
    auto tpop = [&]() -> bool {
        if (tsp == 0u) return false;
        --tsp;
        if (tsp < PT_WF_TLAS_LDS_STACK) { uint32_t v = tlds[tsp * 64u]; asm volatile("" : "+v"(v)); nodeIndex = v; return true; }
        tsp = tsp < PT_BVH_STACK_SIZE ? tsp : PT_BVH_STACK_SIZE - 1u;
        nodeIndex = B.tlasSpill[spill_row(PT_LDS_WORD(s_gw[wv])) * PT_BVH_STACK_SIZE + tsp];
        return true;
    };

    while (true) {
        uint32_t nIdle = (uint32_t)__popcll(__ballot(!have));
        while ((kCached || cursor < nItems) && (nIdle >= PT_WF_REFILL || nIdle == 64u)) {
            if (kCached && cursor >= nItems) {
                if (!more) break;
                uint32_t c = 0u;
                if (lane == 0u) c = atomicAdd(&s_next, 1u);
                c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
                if (c >= WAVES * PT_WF_RANGE / kChunk || wgBase + c * kChunk >= B.numSlots) { more = false; break; }
                slotBase = wgBase + c * kChunk;
                cursor = 0u;
            }
            const uint32_t item = cursor + lane;
            const uint32_t kind = item / kChunk;
            const uint32_t slot = slotBase + (item & (kChunk - 1u));
            bool valid = item < nItems && slot < B.numSlots;
            if (valid) valid = ray_exists(B.flags[slot], kind);
            const Compaction c = compact_candidates(xchg, !have, nIdle, valid, item);
            if (!have && c.rankI < c.take) {
                const uint32_t it = xchg[c.rankI];
                myKind = it / kChunk;
                mySlot = slotBase + (it & (kChunk - 1u));
                v3 d;
                fetch_ray(B, mySlot, myKind, O, d);
                if (myKind == 0u) cn.closestRays++; else cn.shadowRays++;
                if (ray_has_nan(O, d)) {
                    store_result(B, mySlot, myKind, false, rs.hit, true);     // a certain miss
                } else {
                    const v3 D = normalize3(d);                           // tlas.hlsl:238-240
                    rD = mk3(1.0f / D.x, 1.0f / D.y, 1.0f / D.z);
                    rs.hit.t = PT_FAR_PLANE;
                    rs.anyHit = myKind != 0u;
                    nodeIndex = 0u; tsp = 0u; instLeft = 0u; needPop = false; inBlas = false; toverflow = false;
                    have = true;
                }
            }
            __builtin_amdgcn_wave_barrier();
            cursor += c.consumed;
            nIdle = (uint32_t)__popcll(__ballot(!have));
        }
        if (nIdle == 64u) break;
        const uint32_t stopAt = (kCached ? more : cursor < nItems) ? PT_WF_REFILL : 64u;
        do {
            // ---- a lane that is between instances (its instance epilogue is done) walks the TLAS to the next instance whose box it hits.
            //      Per ray of the 200-instance scene: 13.0 TLAS nodes + 5.9 instance entries + 9.6 BLAS nodes + 3.0 triangles = 37
            //      steps against 18.6 for the same geometry baked flat.  Measured: this block is 57 % of the loop's
            //      time; it runs in 45 % of the wave iterations, 11 inner steps per execution (until its slowest lane is inside an
            //      instance) at 15.5 of 64 lanes, 80.8 M wave-steps per pass against 16.2 M executions of the CWBVH step below (37.8
            //      lanes).  Neither the chain's length (one fetch per instance entry instead of two, instByLeaf: no change) nor its
            //      scheduling (one TLAS step per wave iteration, a quorum for entering the block, triangle parking: all slower) is the
            //      lever; letting the last few walkers wait for company (PT_WF_TLAS_CONT) is worth 3 %.  What is left is the work
            //      itself: 19 TLAS steps per ray at a quarter of the lanes.
            //      The walk loop only visits TLAS nodes: lanes that reached a leaf (or still have instances of their leaf left) enter
            //      their instance together in ONE block after it.
            // enter the next instance of the current TLAS leaf
            // ONE fetch: the record PTSetScene laid out per TLAS index slot (worldToLocal, offsets, instance index) instead of
            // TLASData[TLASIndexOffset + k] -> instance record (two dependent fetches; same values)
            auto enter_instance = [&]() {
                const float4* ip = S.instByLeaf + (size_t)nextInst * 6;
                const float4 w0 = ip[0], w1 = ip[1], w2 = ip[2], w3 = ip[3], ints = ip[4];
                instIndex = pt_asuint(ip[5].x);
                nextInst++; instLeft--;
                if (STATS) cn.instanceVisits++;
                off = BlasOffsets{pt_asuint(ints.x), pt_asuint(ints.y), pt_asuint(ints.z)};
                const v3 wd = xyz(f4_array(B, 2u * myKind)[2u * (size_t)mySlot + 1u]);           // the direction row of the lane's ray record
                instance_enter(rs, w0, w1, w2, w3, O, wd, myKind != 0u);
                inBlas = true;
            };
            if (have && !inBlas && instLeft == 0u) {
                bool finished = false;
                for (uint32_t stepT = 0;; ++stepT) {                  // no step bound: until inside the next instance
                    // the lanes still walking are the wave's active lanes here; when only a few are left they wait for company (the
                    // lanes whose instance ends in this wave iteration) instead of stepping through the TLAS at 1-2 lanes per instruction
                    if (PT_WF_TLAS_CONT > 1u && stepT > 0u && (uint32_t)__popcll(__ballot(true)) < PT_WF_TLAS_CONT) break;
                    if (needPop) {
                        if (!tpop()) { finished = true; break; }
                        needPop = false;
                    }
                    // visit TLAS node nodeIndex
                    float4 a, b, c, e;
                    if (kCached && nodeIndex < cachedNodes) {
                        const float4* cp = &s_tcache[nodeIndex * 4u];
                        a = cp[0]; b = cp[1]; c = cp[2]; e = cp[3];
                        asm volatile("" : "+v"(a.x), "+v"(b.x), "+v"(c.x), "+v"(e.x));        // ds_read_b128 here, global_load below: never one flat load (see tpush)
                    } else {
                        const float4* np = (const float4*)(T + (size_t)nodeIndex * 16u);
                        a = np[0]; b = np[1]; c = np[2]; e = np[3];
                        // all four rows requested before the first use: left alone, the compiler fetches the instance count first, waits, and
                        // requests the boxes (or the leaf's first index) under the branch on it -- two dependent round trips per TLAS step
                        asm volatile("" : "+v"(a.x), "+v"(b.x), "+v"(c.x), "+v"(c.w), "+v"(e.x), "+v"(e.w));
                    }
                    if (STATS) cn.tlasNodeVisits++;
                    const TlasStep step = tlas_node_step(a, b, c, e, O, rD, rs.hit.t);
                    if (!step.leaf) {
                        if (step.nothingHit) needPop = true;
                        else {
                            nodeIndex = step.near;
                            if (step.pushFar) tpush(step.far);
                        }
                    } else {
                        nextInst = step.first;
                        instLeft = step.count;
                        needPop = true;                                    // after the leaf's instances
                        break;                                             // to the entry block below
                    }
                }
                if (finished) {
                    // the hit record was stored when it improved; a shadow ray that gets here found nothing (stopNow below ends the others)
                    store_result(B, mySlot, myKind, myKind == 0u && rs.hit.t < PT_FAR_PLANE, rs.hit, true);
                    if (STATS && toverflow) cn.overflows++;
                    have = false;
                }
            }
            if (have && !inBlas && instLeft > 0u) enter_instance();
            // ---- the hot step: one CWBVH iteration inside the current instance
            if (have && inBlas) {
                const float tBefore = rs.hit.t;
                const bool blasDone = cwbvh_iteration<STATS, true>(S, rs, off, st, cn);
                if (myKind == 0u && rs.hit.t < tBefore) f4_array(B, PT_F4_HIT)[mySlot] = make_float4(rs.hit.t, rs.hit.u, rs.hit.v, pt_asfloat(rs.hit.triIndex));
                if (blasDone) {
                    inBlas = false;
                    if (rs.anyHit) {
                        if (rs.hitFound) {                                                               // stopNow (tlas.hlsl:196-200)
                            store_result(B, mySlot, myKind, true, rs.hit, true);
                            if (STATS && toverflow) cn.overflows++;
                            have = false;
                        }
                    } else if (rs.hitFound) {
                        // world-space hit position and distance of the instance that improved the hit
                        const float4* ip = S.instances + (size_t)instIndex * 9;
                        const v3 pos = instance_exit<STATS>(rs, ip[0], ip[1], ip[2], ip[3], O, cn);
                        ((float*)&f4_array(B, PT_F4_HIT)[mySlot])[0] = rs.hit.t;
                        f4_array(B, PT_F4_HIT2)[mySlot] = make_float4(pos.x, pos.y, pos.z, pt_asfloat(instIndex));
                    }
                }
            }
            nIdle = (uint32_t)__popcll(__ballot(!have));
        } while (nIdle < stopAt);
    }
    __builtin_amdgcn_wave_barrier();
    flush_counters<STATS>(cn, B.statRows, (B.numSlots >> 6) + *PT_LDS_WORD(s_gw[wv]), lane);
}

// ------------------------------------------------------------------------------------------
// persistent trace (schedule 3): the refill kernel above, made persistent.  The grid is exactly the number of
// waves the chip holds; a wave that has scanned its 64-slot chunk pulls the NEXT chunk index from a device counter
// while its remaining rays are still in flight, so lanes are refilled continuously and nothing drains until the
// very end of the launch.  Chunk counters are sharded 8 ways (one per XCD under round-robin workgroup placement,
// blockIdx % 8) on separate 128-byte lines; a wave takes from its own shard first and steals from the others when
// it runs dry: ~numSlots/64 returning atomics per launch in total, i.e. one per 192 candidate rays.
// Which wave traces which ray depends on timing; what is computed for a ray does not.
// ------------------------------------------------------------------------------------------
PT_DEV bool next_chunk(uint32_t* heads, uint32_t numChunks, uint32_t shard, uint32_t& chunk)
{
    // lane 0 asks; everybody gets the answer.  Shard sh owns the chunks c with c % 8 == sh.
    uint32_t result = 0xFFFFFFFFu;
    if ((threadIdx.x & 63u) == 0u) {
        for (uint32_t t = 0; t < PT_WF_SHARDS; ++t) {
            const uint32_t sh = (shard + t) & (PT_WF_SHARDS - 1u);
            const uint32_t inShard = (numChunks + PT_WF_SHARDS - 1u - sh) / PT_WF_SHARDS;
            if (inShard == 0u) continue;
            const uint32_t k = atomicAdd(&heads[sh * 32u], 1u);
            if (k < inShard) { result = k * PT_WF_SHARDS + sh; break; }
        }
    }
    result = __shfl(result, 0, 64);
    chunk = result;
    return result != 0xFFFFFFFFu;
}

template <bool STATS>
__global__ __launch_bounds__(64, PT_WF_TRACE_MIN_WAVES) void pt_wf_trace_persist(DScene S, PTWfBuffers B, uint32_t iteration)
{
    __shared__ uint2 s_stack[PT_WF_LDS_STACK][64];
    __shared__ uint32_t s_xchg[64];
    const uint32_t lane = threadIdx.x;
    const uint32_t numChunks = (B.numSlots + PT_WF_CHUNK - 1u) / PT_WF_CHUNK;
    const uint32_t shard = blockIdx.x & (PT_WF_SHARDS - 1u);
    const uint32_t nItems = 3u * PT_WF_CHUNK;
    pt_lds_u32 xchg = (pt_lds_u32)&s_xchg[0];

    Counters cn = {};
    TravStackT<PT_WF_LDS_STACK, true> st;
    st.lds = PT_LDS_U2(&s_stack[0][lane]);
    st.stride = 64u;
    st.gbase = B.stackSpill;
    __shared__ uint32_t s_gw;
    if (lane == 0u) s_gw = blockIdx.x;
    st.gwave = PT_LDS_WORD(s_gw);                                                 // grid <= numSlots / 64 waves
    RayState rs;
    rs.sp = 0u; rs.anyHit = false; rs.overflow = false;
    bool have = false;
    uint32_t mySlot = 0u, myKind = 0u;
    uint32_t cursor = nItems, slotBase = 0u;        // no chunk yet
    bool more = true;                                // chunks may remain

    while (true) {
        uint32_t nIdle = (uint32_t)__popcll(__ballot(!have));
        // ---- refill from the current chunk, pulling new chunks as needed
        while (nIdle >= PT_WF_REFILL || nIdle == 64u) {
            if (cursor >= nItems) {
                uint32_t chunk;
                if (!more || !next_chunk(B.chunkHeads, numChunks, shard, chunk)) { more = false; break; }
                slotBase = chunk * PT_WF_CHUNK;
                cursor = 0u;
            }
            const uint32_t item = cursor + lane;
            const uint32_t kind = item / PT_WF_CHUNK;
            const uint32_t slot = slotBase + (item & (PT_WF_CHUNK - 1u));
            bool valid = item < nItems && slot < B.numSlots;
            if (valid) valid = ray_exists(B.flags[slot], kind);
            const Compaction c = compact_candidates(xchg, !have, nIdle, valid, item);
            if (!have && c.rankI < c.take) {
                const uint32_t it = xchg[c.rankI];
                myKind = it / PT_WF_CHUNK;
                mySlot = slotBase + (it & (PT_WF_CHUNK - 1u));
                have = start_ray(B, mySlot, myKind, rs, cn);
            }
            __builtin_amdgcn_wave_barrier();
            cursor += c.consumed;
            nIdle = (uint32_t)__popcll(__ballot(!have));
        }
        if (nIdle == 64u) break;                                      // no chunk left and nothing in flight
        const uint32_t stopAt = more ? PT_WF_REFILL : 64u;
        do {
            if (have) {
                const float tBefore = rs.hit.t;
                const bool fin = ray_step<STATS>(S, rs, st, cn);
                if (myKind == 0u && rs.hit.t < tBefore) f4_array(B, PT_F4_HIT)[mySlot] = make_float4(rs.hit.t, rs.hit.u, rs.hit.v, pt_asfloat(rs.hit.triIndex));
                if (fin) {
                    store_result(B, mySlot, myKind, rs.hit.t < PT_FAR_PLANE, rs.hit, true);
                    have = false;
                }
            }
            nIdle = (uint32_t)__popcll(__ballot(!have));
        } while (nIdle < stopAt);
    }
    flush_counters<STATS>(cn, B.statRows, (B.numSlots >> 6) + blockIdx.x, lane);
}

// ------------------------------------------------------------------------------------------
// shade: one lane per slot
// ------------------------------------------------------------------------------------------
// one lane per slot, in screen order: every regrouping of the slots that shade a hit was measured slower
template <bool STATS, class MAP = PTTileMap>
__global__ __launch_bounds__(PT_WF_SHADE_BLOCK, PT_WF_SHADE_MIN_WAVES) void pt_wf_shade(DScene S, PTFrameParams P, MAP tm, PTWfBuffers B,
                                                                         uint32_t iteration)
{
    const uint32_t vb = blockIdx.x;
    const uint32_t slot = vb * PT_WF_SHADE_BLOCK + threadIdx.x;
    if (vb == 0u && threadIdx.x < PT_WF_SHARDS) B.chunkHeads[threadIdx.x * 32u] = 0u;   // for the next trace launch (schedule 3)
    const uint32_t f = B.flags[slot];
    Counters cn = {};
    if (fl_state(f) != PS_DONE) shade_slot<STATS, false, MAP>(S, P, tm, B, slot, slot, f, cn, vb * PT_WF_SHADE_BLOCK);
    flush_counters<STATS>(cn, B.statRows, vb * (PT_WF_SHADE_BLOCK / 64u) + (threadIdx.x >> 6), threadIdx.x & 63u);
}

// ------------------------------------------------------------------------------------------
// Schedule 4: the FUSED PERSISTENT wavefront.  One launch per pass; no launch boundary anywhere inside it.
//
// Paths of different pixels never exchange anything (PathTracer.compute:60), so nothing in a pass needs a grid-wide barrier: the
// 52 x 3 launches of schedule 1 only exist because a launch is the unit in which that schedule alternates between the lean trace
// code and the register-hungry shading code.  Here a persistent wave does the alternating itself, over path CONTEXTS it owns:
//
//     a wave owns PT_WF_FUSED_GROUPS x 64 contexts (path state in HBM, indexed by context, not by pixel);
//     loop {  refill:  every context whose pixel has finished takes the next pixel of the frame from a device counter
//                      (one atomic per wave and round; the camera ray of its first sample is written);
//             trace:   the refill scheduler of pt_wf_trace_refill over the contexts' 3 x 64 x GROUPS candidate rays -- 64 resumable
//                      traversals in flight, idle lanes re-filled by ballot / rank compaction -- until the candidates are used up
//                      and <= PT_WF_SUSPEND rays are left; those are parked as records in LDS and resumed in the next round;
//             shade:   path_step() for every context whose rays have all returned; a pixel that finished its last sample
//                      leaves its sample sum in the per-pixel array the resolve kernel reads.  }
//
// Every context is busy until the frame runs out of pixels: there is no per-launch ramp-up and drain, no tail launch, no cleanup
// kernel, and ONE pass in flight fills the machine -- a host that synchronises after every pass (the reference presents every
// pass, PathTracer.cs:251-272) gets the pipelined throughput, with one path-state set of ~1 M contexts instead of twelve sets
// of one slot per pixel.  A wave only ever touches the state of its own contexts, so ordering is program order within the
// wave (workgroup-scope fences between phases).  Which context renders which pixel depends on timing; what is computed for a
// pixel does not: same device functions, same per-path order as every other schedule -> frames and counters are bit-identical.
// ------------------------------------------------------------------------------------------
#ifndef PT_WF_FUSED_WAVES
#define PT_WF_FUSED_WAVES 4         // waves per SIMD the fused kernel is compiled for (128 VGPRs)
#endif

#define PT_WF_NO_PIXEL 0xFFFFFFFFu

// add a phase's counters to the wave's LDS totals (one wave per workgroup; 16 words, PTStats order)
template <bool STATS>
PT_DEV void counters_to_lds(const Counters& cn, pt_lds_u32 tot, uint32_t lane)
{
    uint32_t vals[PT_NUM_COUNTERS];
    counters_to_array(cn, vals);
#pragma unroll
    for (int i = 0; i < PT_NUM_COUNTERS; ++i) {
        if (!STATS && (i >= 3 && i <= 9)) continue;
        if (!STATS && i >= 12) continue;
        if (i == 12) {
            const uint32_t m = wave_max_u32(vals[i]);
            if (lane == 0u && m > tot[i]) tot[i] = m;
        } else {
            const uint32_t v = wave_sum_u32(vals[i]);
            if (lane == 0u && v) tot[i] += v;
        }
    }
}

template <bool STATS>
__global__ __launch_bounds__(64, PT_WF_FUSED_WAVES) void pt_wf_fused(DScene S, PTFrameParams P, PTBatch batch, PTTileMap tm, PTWfBuffers B)
{
    constexpr uint32_t K = PT_WF_FUSED_GROUPS;
    constexpr uint32_t kSusp = PT_WF_SUSPEND ? PT_WF_SUSPEND : 1u;
    static_assert((K & (K - 1u)) == 0u && K >= 1u && K <= 16u, "context groups per wave: a power of two");
    __shared__ uint2 s_stack[PT_WF_LDS_STACK][64];
    __shared__ uint32_t s_xchg[64];
    __shared__ uint32_t s_pix[K][64];           // the pixel (slot of the frame's enumeration, pt_slot_to_pixel) a context renders, or PT_WF_NO_PIXEL
    __shared__ uint32_t s_pend[2][K][2];        // [buffer][group][low / high word]: contexts that have a ray parked in s_susp
    __shared__ uint4 s_susp[kSusp][PT_WF_SUSP_ROWS];
    __shared__ uint32_t s_cnt[PT_NUM_COUNTERS];
    __shared__ uint32_t s_gw;
    const uint32_t lane = threadIdx.x;
    const uint32_t ctxBase = blockIdx.x * (K * 64u);                 // context = ctxBase + group * 64 + lane
    pt_lds_u32 xchg = (pt_lds_u32)&s_xchg[0];
    pt_lds_u32 pix = (pt_lds_u32)&s_pix[0][0];
    pt_lds_u32 cnt = (pt_lds_u32)&s_cnt[0];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
        s_pix[k][lane] = PT_WF_NO_PIXEL;
        B.flags[ctxBase + k * 64u + lane] = PS_DONE;                 // a context without a pixel has no rays (the trace scan reads the flag words)
    }
    if (lane < PT_NUM_COUNTERS) s_cnt[lane] = 0u;
    if (lane < 4u * K) (&s_pend[0][0][0])[lane] = 0u;
    if (lane == 0u) s_gw = blockIdx.x;
    __builtin_amdgcn_wave_barrier();
    uint32_t nSusp = 0u, pb = 0u;
    bool more = true;

    while (true) {
        // ---- (0) refill: a context without a pixel takes the next pixel of the frame and starts its first sample
        bool any = false;
#pragma unroll 1
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t ctx = ctxBase + k * 64u + lane;
            uint32_t mine = pix[k * 64u + lane];
            const unsigned long long E = __ballot(mine == PT_WF_NO_PIXEL);
            if (more && E != 0ull) {                                 // wave-uniform
                const uint32_t n = (uint32_t)__popcll(E);
                uint32_t base = 0u;
                if (lane == 0u) base = atomicAdd(&B.chunkHeads[0], n);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base + n >= B.numSlots) more = false;
                Counters cn = {};
                if (mine == PT_WF_NO_PIXEL) {
                    const uint32_t slot = base + rank_below(E);
                    uint32_t px, py, pass;
                    if (slot < B.numSlots && pt_slot_to_pixel(tm, pixel_slot_of(B, slot, pass), px, py)) {      // (slots of partially covered edge tiles have no pixel)
                        PathRegs r;
                        uint32_t seedRoot, currentSample;
                        pt_batch_pick(batch, pass, seedRoot, currentSample);
                        path_init(P, seedRoot, currentSample, px, py, py * P.OutputWidth + px, r, cn);
                        store_path(B, ctx, r, false);
                        mine = slot;
                        pix[k * 64u + lane] = slot;
                    }
                }
                counters_to_lds<false>(cn, cnt, lane);
            }
            any = any || __ballot(mine != PT_WF_NO_PIXEL) != 0ull;
        }
        if (!any) { if (!more) break; else continue; }              // nothing to do: out of pixels -> done; else an edge tile gave none, pull again
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        __builtin_amdgcn_wave_barrier();

        // ---- (1) trace: resume what was parked, then scan the contexts' flag words kind-major and keep 64 traversals in flight
        {
            Counters cn = {};
            TravStackT<PT_WF_LDS_STACK, true> st;
            st.lds = PT_LDS_U2(&s_stack[0][lane]);
            st.stride = 64u;
            st.gbase = B.stackSpill;
            st.gwave = PT_LDS_WORD(s_gw);
            RayState rs;
            rs.sp = 0u; rs.anyHit = false; rs.overflow = false;
            rs.o = mk3(0.0f); rs.d = mk3(0.0f); rs.invDir = mk3(0.0f); rs.octinv4 = 0u;
            rs.ng = make_uint2(0u, 0u); rs.tg = make_uint2(0u, 0u);
            rs.hit.t = PT_FAR_PLANE; rs.hit.u = 0.0f; rs.hit.v = 0.0f; rs.hit.triIndex = 0u;
            bool have = false;
            uint32_t myRef = 0u;                                     // kind << 30 | context index within the wave (group * 64 + lane)
            const uint32_t po = pb, pn = pb ^ 1u;                    // pend masks: previous round (read), this round (written)
            if (lane < 2u * K) (&s_pend[pn][0][0])[lane] = 0u;
            // parked rays first: lane i takes record i (all lanes are idle here)
            if (PT_WF_SUSPEND > 0u && lane < nSusp) {
                myRef = resume_ray(B, s_susp[lane], ctxBase, rs, st);
                if ((myRef >> 30) == 0u && rs.hit.t < PT_FAR_PLANE) {   // the best hit so far was left in the hit array
                    const float4 h = f4_array(B, PT_F4_HIT)[ctxBase + (myRef & 0x3FFFFFFFu)];
                    rs.hit.u = h.y; rs.hit.v = h.z; rs.hit.triIndex = pt_asuint(h.w);
                }
                have = true;
            }
            nSusp = 0u;
            const uint32_t nItems = 3u * 64u * K;
            uint32_t cursor = 0u;
            bool startedNew = false;

            while (true) {
                uint32_t nIdle = (uint32_t)__popcll(__ballot(!have));
                while (cursor < nItems && (nIdle >= PT_WF_REFILL || nIdle == 64u)) {
                    const uint32_t item = cursor + lane;
                    const uint32_t kind = item / (64u * K);
                    const uint32_t local = item & (64u * K - 1u);    // group * 64 + lane of the context
                    bool valid = item < nItems;
                    if (valid) {
                        const uint32_t pw = s_pend[po][local >> 6][(local >> 5) & 1u];
                        // (a context with a parked ray got all its rays last round; one without a pixel is DONE)
                        valid = !((pw >> (local & 31u)) & 1u) && ray_exists(B.flags[ctxBase + local], kind);
                    }
                    const Compaction c = compact_candidates(xchg, !have, nIdle, valid, (kind << 30) | local);
                    if (!have && c.rankI < c.take) {
                        myRef = xchg[c.rankI];
                        have = start_ray(B, ctxBase + (myRef & 0x3FFFFFFFu), myRef >> 30, rs, cn);
                    }
                    __builtin_amdgcn_wave_barrier();
                    if (c.take > 0u) startedNew = true;
                    cursor += c.consumed;
                    nIdle = (uint32_t)__popcll(__ballot(!have));
                }
                if (nIdle == 64u) break;
                const bool exhausted = cursor >= nItems;
                // parking is allowed only in a round that started new rays: a round that merely resumed must finish them
                const bool mayPark = PT_WF_SUSPEND > 0u && exhausted && startedNew;
                const uint32_t stopAt = !exhausted ? PT_WF_REFILL : (mayPark ? 64u - PT_WF_SUSPEND : 64u);
                while (nIdle < stopAt) {
                    if (wave_step<STATS>(S, have, rs, st, cn)) {
                        store_result(B, ctxBase + (myRef & 0x3FFFFFFFu), myRef >> 30, rs.hit.t < PT_FAR_PLANE, rs.hit, false);
                        have = false;
                    }
                    nIdle = (uint32_t)__popcll(__ballot(!have));
                }
                if (mayPark && nIdle < 64u) {
                    have = finish_slab_rays<STATS>(S, B, have, ctxBase + (myRef & 0x3FFFFFFFu), myRef >> 30, rs, st, cn);
                    const unsigned long long act = __ballot(have);
                    if (have) {
                        const uint32_t kind = myRef >> 30, local = myRef & 0x3FFFFFFFu;
                        if (kind == 0u && rs.hit.t < PT_FAR_PLANE) store_hit(B, ctxBase + local, rs.hit);
                        suspend_ray(s_susp[rank_below(act)], myRef, rs, st);
                        atomicOr(&s_pend[pn][local >> 6][(local >> 5) & 1u], 1u << (local & 31u));
                        have = false;
                    }
                    nSusp = (uint32_t)__popcll(act);
                    break;
                }
            }
            pb = pn;
            counters_to_lds<STATS>(cn, cnt, lane);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        __builtin_amdgcn_wave_barrier();

        // ---- (2) shade: every context whose rays have all returned
#pragma unroll 1
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t ctx = ctxBase + k * 64u + lane;
            const uint32_t mine = pix[k * 64u + lane];
            const uint32_t pw = s_pend[pb][k][lane >> 5];
            const bool parked = (pw >> (lane & 31u)) & 1u;
            Counters cn = {};
            if (mine != PT_WF_NO_PIXEL && !parked) {
                const uint32_t f = B.flags[ctx];
                if (!shade_slot<STATS, true>(S, P, tm, B, ctx, mine, f, cn)) pix[k * 64u + lane] = PT_WF_NO_PIXEL;    // pixel finished: its sum is in B.pixsum
            }
            counters_to_lds<STATS>(cn, cnt, lane);                   // every lane of the wave takes part in the reductions
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    // the wave's totals -> its counter row (a wave owns row blockIdx.x for the whole launch)
    __builtin_amdgcn_wave_barrier();
    if (lane < PT_NUM_COUNTERS) {
        unsigned long long* p = B.statRows + (size_t)blockIdx.x * 16u + lane;
        const unsigned long long v = cnt[lane];
        if (lane == 12u) { if (v > *p) *p = v; } else if (v) *p += v;
    }
}

// cleanup: pixels still alive after the fixed number of iterations are run to completion here, one lane per slot with
// the megakernel's loop (trace <= 3 rays, path_step, repeat).  Normally a handful of lanes; correctness for any path length.
template <bool STATS, bool TLAS, class MAP = PTTileMap>
__global__ __launch_bounds__(256, 2) void pt_wf_cleanup(DScene S, PTFrameParams P, MAP tm, PTWfBuffers B)
{
    __shared__ uint2 s_stack[PT_LDS_STACK][256];
    cleanup_slots<STATS, TLAS, false, MAP>(S, P, tm, B, s_stack);                 // pt_wf_shade.h
}

// resolve: the pixel write of PathTracer.compute:89-98, applied to every pixel's sample sum -- for a batch, once per pass and in
// pass order, each pass reading what the previous one would have written (the intermediate frames are never stored; the running
// mean is the same chain of fp32 operations).
// MAP = PTListMap, the resolve of a pass over a block list: workgroup e writes the covered pixels of table entry e with the block's
// own sample count (CurrentSample = n_b + j * spp).  Every other pixel of `output` was copied from `accumulated` by the launcher.
template <class MAP = PTTileMap>
__global__ __launch_bounds__(256) void pt_wf_resolve(PTFrameParams P, PTBatch batch, MAP tm, PTWfBuffers B, const float4* __restrict__ sums,
                                                     const float4* __restrict__ accumulated, float4* __restrict__ output)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t px, py, pass, base;
    Counters cn = {};
    if (slot < B.slotsPerPass && wf_pixel(tm, B, slot, blockIdx.x * 256u, px, py, pass, base)) {
        const uint32_t pixelIndex = py * P.OutputWidth + px;
        const uint32_t numSamples = P.SamplesPerPass > 1 ? (uint32_t)P.SamplesPerPass : 1u;
        const float fSamples = (float)numSamples;
        v3 acc = mk3(0.0f);
        for (uint32_t j = 0; j < batch.count; ++j) {
            uint32_t seedRoot, currentSample;
            pt_batch_pick(batch, j, seedRoot, currentSample);
            if (kListMap<MAP>) currentSample = base + j * numSamples;
            const v3 color = xyz(sums[(size_t)j * B.slotsPerPass + slot]);      // per-pixel sample sum: B.color (schedules 1-3) or B.pixsum (schedule 4)
            if (currentSample > 0u) {
                if (j == 0u) {
                    const float4 a = accumulated[pixelIndex];
                    acc = mk3(a.x, a.y, a.z);
                }
                cn.pixelsRead++;
                const float cs = (float)currentSample;
                acc = (color + acc * cs) / (cs + fSamples);
            } else {
                acc = color / fSamples;
            }
            cn.pixelsWritten++;
        }
        output[pixelIndex] = make_float4(acc.x, acc.y, acc.z, 1.0f);
    }
    flush_counters<false>(cn, B.statRows, blockIdx.x * 4u + (threadIdx.x >> 6), threadIdx.x & 63u);
}

// resolve of a radiance query: entry s gets the mean of its samples -- the expression of pt_wf_resolve's CurrentSample == 0 branch --
// and the RNG state its path ended with.  Writes nothing past count; counts nothing (no pixel is written).
__global__ __launch_bounds__(256) void pt_wf_resolve_rays(PTFrameParams P, PTRayMap rm, PTWfBuffers B, PTRadiance* __restrict__ out)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= rm.count) return;
    const uint32_t numSamples = P.SamplesPerPass > 1 ? (uint32_t)P.SamplesPerPass : 1u;
    const float fSamples = (float)numSamples;
    const v3 acc = xyz(B.color[slot]) / fSamples;
    ((float4*)out)[slot] = make_float4(acc.x, acc.y, acc.z, pt_asfloat(B.rng[slot]));
}

// fold the per-wave rows into the context's 16 counters (PTStats order) and clear them
__global__ __launch_bounds__(256) void pt_wf_fold_rows(unsigned long long* rows, uint32_t numRows, unsigned long long* gstats)
{
    unsigned long long acc[PT_NUM_COUNTERS] = {};
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < numRows; r += gridDim.x * 256u) {
        unsigned long long* p = rows + (size_t)r * 16u;
#pragma unroll
        for (int i = 0; i < PT_NUM_COUNTERS; ++i) {
            unsigned long long v = p[i];
            if (i == 12) acc[i] = v > acc[i] ? v : acc[i]; else acc[i] += v;
            p[i] = 0ull;
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int i = 0; i < PT_NUM_COUNTERS; ++i) {
        unsigned long long v = acc[i];
        for (int off = 32; off > 0; off >>= 1) {
            unsigned long long o = __shfl_xor(v, off, 64);
            if (i == 12) v = o > v ? o : v; else v += o;
        }
        if (lane == 0 && v) { if (i == 12) atomicMax(&gstats[i], v); else atomicAdd(&gstats[i], v); }
    }
}

// Walks the arena of a state set in carving order and returns its size; with a base, fills B with the pointers.
size_t pt_wf_arena_layout(char* base, uint32_t numSlots, uint32_t residentWaves, bool needTlas, uint32_t maxIterations, PTWfBuffers& B)
{
    const size_t n = numSlots;
    const uint32_t numRows = PT_WF_STAT_ROW_SETS * (numSlots >> 6);
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // trace waves own 64 or 128 consecutive slots (pt_wf_wide_ranges); a wave addresses 64 slab rows and PT_WF_SUSPEND records.
    // The HAS_TLAS refill kernel always uses PT_WF_RANGE = 128 slots per wave; the plain one 64 or 128.
    const size_t traceWaves = pt_wf_max_trace_waves(numSlots, residentWaves);
    const size_t spillBytes = traceWaves * 64u * (size_t)(needTlas ? PT_WF_SPILL_ROW_ENTRIES : PT_BVH_STACK_SIZE - PT_WF_LDS_STACK) * sizeof(uint2);
    const size_t suspBytes = traceWaves * (size_t)(PT_WF_SUSPEND ? PT_WF_SUSPEND : 1u) * PT_WF_SUSP_RECORD_ROWS * sizeof(uint4);
    const size_t tlasSpillBytes = needTlas ? traceWaves * 64u * (size_t)PT_BVH_STACK_SIZE * sizeof(uint32_t) : 0;
    size_t total = 0;
    auto carve = [&](size_t bytes) { char* q = base ? base + total : nullptr; total += align(bytes); return q; };
    B.flags = (uint32_t*)carve(n * 4);
    B.rng = (uint32_t*)carve(n * 4);
    float4* dummy = nullptr;
    float4** arrs[PT_F4_COUNT] = {&B.ray[0], &dummy, &B.ray[1], &dummy, &B.ray[2], &dummy, &B.rad, &B.thr, &B.color, &B.envC, &B.lightC, &B.pthr, &B.hit, &B.hit2, &B.pixsum};   // PT_F4_* order; a ray-record array spans two strides
    for (auto a : arrs) *a = (float4*)carve(n * 16);
    B.f4base = B.ray[0];
    B.f4stride = (uint32_t)(align(n * 16) / 16);
    B.occl = (uint8_t*)carve(n * 2);
    B.statRows = (unsigned long long*)carve((size_t)numRows * 16 * 8);
    B.chunkHeads = (uint32_t*)carve(PT_WF_SHARDS * 32 * 4);
    B.stackSpill = (uint2*)carve(spillBytes);
    B.susp = (uint4*)carve(suspBytes);
    B.suspCount = (uint32_t*)carve(traceWaves * 4);
    B.tlasSpill = needTlas ? (uint32_t*)carve(tlasSpillBytes) : nullptr;
    // repack: the pixel index of a slot, the block counts, the decision, and the temporary region of numSlots / 2 slots.  Between a
    // shade and a trace launch stackSpill and susp hold nothing (a trace launch writes an entry or a record before it reads it),
    // and they were carved back to back: the region lies over them when they are large enough -- they are, for every set this
    // file sizes today (96 + 12 bytes per slot at 128 slots per trace wave against 92) --, in memory of its own otherwise.
    B.pixelOf = (uint32_t*)carve(n * 4);
    B.rpPrefix = (uint32_t*)carve((n >> 8) * 4 + 4);
    B.rpCtl = (uint32_t*)carve(ptrepack::PT_REPACK_CTL_WORDS * 4);
    B.rpCapacity = numSlots / 2u;
    const size_t tempBytes = (size_t)B.rpCapacity * PT_WF_REPACK_SLOT_BYTES;
    const bool aliased = base ? (char*)B.susp + suspBytes >= (char*)B.stackSpill + tempBytes : align(spillBytes) + suspBytes >= tempBytes;
    B.rpTemp = aliased ? (char*)B.stackSpill : carve(tempBytes);
    B.residentWaves = residentWaves;
    B.numSlots = numSlots;
    B.numStatRows = numRows;
    B.maxIterations = maxIterations;
    return total;
}

} // namespace

// One pass = a fixed sequence of launches on L.stream, no host synchronisation (see the file header).
// L.orderAfter (may be null) is the event of the previous pass's resolve: this pass's resolve reads that pass's output as
// AccumulatedOutput and, with ping-pong frames, overwrites the frame that resolve was still reading.
// MAP = PTListMap: the pass over a block list; nothing is zeroed and the frame is copied instead.
// MAP = PTRayMap: a radiance query: L.output is the PTRadiance array, nothing is ordered, zeroed or copied.  An irradiance gather
// (PT_WF_MAP_GATHER) runs the same instantiations between pt_gather.hip's init and resolve kernels, SH light probes (PT_WF_MAP_PROBE)
// between pt_probe.hip's.
// UNIT_A: this compilation of the file is the one without the post-RA scheduler (csrc/Makefile).  It is entered for the plain
// refill trace only, the other one for everything else -- each instantiates only the kernels it can launch.
namespace {

// what traces the rays of an iteration -- or, fused, renders the whole pass in one launch
enum class Trace { Refill, RefillTlas, Lane, Persist, Fused };
Trace pick_trace(int schedule, bool tlas)
{
    // HAS_TLAS: schedules 1 and 4 walk the two levels through the refill scheduler, 2 and 3 with one ray per lane
    if (tlas) return schedule == 1 || schedule == 4 ? Trace::RefillTlas : Trace::Lane;
    return schedule == 1 ? Trace::Refill : schedule == 2 ? Trace::Lane : schedule == 3 ? Trace::Persist : Trace::Fused;
}

// f(std::true_type / std::false_type): a run-time flag picks a template argument of the one launch statement f holds
template <class F> void with_flag(bool flag, F&& f) { if (flag) f(std::true_type{}); else f(std::false_type{}); }
#define PT_FLAG(x) (decltype(x)::value)

template <class MAP, bool UNIT_A>
hipError_t launch_sequence(const PTWfLaunch& L, const MAP& tm, uint32_t* launchesOut)
{
    constexpr bool kList = kListMap<MAP>, kRays = kRayMap<MAP>;
    const DScene& S = *L.scene;
    const PTFrameParams& P = *L.params;
    const PTBatch& batch = L.batch;
    const PTWfBuffers& B = *L.buffers;
    const bool fullStats = L.fullStats;
    const hipStream_t stream = L.stream;
    float4* const output = (float4*)L.output;
    const uint32_t nb = B.numSlots >> 8, nbPass = B.slotsPerPass >> 8;
    uint32_t launches = 0;
    hipError_t e;
    const bool tlas = S.hasTlas != 0u;
    const Trace trace = pick_trace(L.schedule, tlas);
    if (UNIT_A != (trace == Trace::Refill)) return hipErrorInvalidValue;       // pt_launch_wavefront picks the unit
    if (trace == Trace::Fused) {
        if constexpr (!UNIT_A && !kList && !kRays) {
            // schedule 4: one persistent launch renders the whole pass (pt_wf_fused); then the ordered pixel write and the counter fold
            if ((e = hipMemsetAsync(B.chunkHeads, 0, sizeof(uint32_t), stream)) != hipSuccess) return e;
            const uint32_t maxWaves = B.numSlots / (64u * PT_WF_FUSED_GROUPS);           // contexts never outnumber the frame's slots (array sizes)
            uint32_t waves = B.residentWaves / 8u * (uint32_t)PT_WF_FUSED_WAVES;          // CUs x 4 SIMDs x waves per SIMD
            if (waves > maxWaves) waves = maxWaves;
            if (waves == 0u) waves = 1u;
            with_flag(fullStats, [&](auto stats) {
                hipLaunchKernelGGL(pt_wf_fused<PT_FLAG(stats)>, dim3(waves), dim3(64), 0, stream, S, P, batch, tm, B);
            });
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if (L.orderAfter && (e = hipStreamWaitEvent(stream, L.orderAfter, 0)) != hipSuccess) return e;
            if (L.zeroOutputFirst &&
                (e = hipMemsetAsync(output, 0, (size_t)P.OutputWidth * P.OutputHeight * sizeof(float4), stream)) != hipSuccess) return e;
            hipLaunchKernelGGL(pt_wf_resolve<PTTileMap>, dim3(nbPass), dim3(256), 0, stream, P, batch, tm, B, (const float4*)B.pixsum, L.accumulated, output);
            hipLaunchKernelGGL(pt_wf_fold_rows, dim3(256), dim3(256), 0, stream, B.statRows, B.numStatRows, L.counters);
            if (launchesOut) *launchesOut = 3u;
            return hipGetLastError();
        } else {
            return hipErrorNotSupported;
        }
    }
    // an irradiance gather is the ray list's sequence with its own first and last kernel (pt_gather.hip)
    const bool gather = kRays && L.mapKind == PT_WF_MAP_GATHER;
    // ... and so are SH light probes (pt_probe.hip)
    const bool probe = kRays && L.mapKind == PT_WF_MAP_PROBE;
    if (gather) { if ((e = pt_launch_gather_init(S, P, L.gather, B, fullStats, stream)) != hipSuccess) return e; }
    else if (probe) { if ((e = pt_launch_probe_init(L.probe, B, stream)) != hipSuccess) return e; }
    else hipLaunchKernelGGL(pt_wf_init<MAP>, dim3(nb), dim3(256), 0, stream, P, batch, tm, B);
    launches++;
    const uint32_t spp = P.SamplesPerPass > 1 ? (uint32_t)P.SamplesPerPass : 1u;
    const uint32_t bounces = P.MaxRayBounces > 1u ? P.MaxRayBounces : 1u;
    // a sample needs at most (bounces + 1) closest-hit iterations + 1 to apply its last NEE; alpha-skips beyond that go to cleanup
    uint32_t iterations = L.iterationsOverride ? L.iterationsOverride : spp * (bounces + 2u) + 4u;
    if (iterations > B.maxIterations) iterations = B.maxIterations;
    // repack (pt_repack.hip): the default schedule over the frame's own blocks, large sets, long sequences
    const bool repack = !kList && !kRays && (trace == Trace::Refill || trace == Trace::RefillTlas) && B.rpTemp != nullptr &&
                        pt_wf_repack_slots(B.numSlots, B.residentWaves) && iterations >= PT_WF_REPACK_MIN_ITERATIONS;
    bool firstCandidate = true;
    for (uint32_t it = 0; it < iterations; ++it) {
        if constexpr (UNIT_A) {
            const bool wide = PT_WF_RANGE >= 128u && pt_wf_wide_ranges(B.numSlots, B.residentWaves);         // pt_launch.h
            const uint32_t blocks = wide ? (B.numSlots + 127u) / 128u : (B.numSlots + 63u) / 64u;
            // the main launch, then the tail launch over the rays the main one's waves left suspended
            auto refill = [&](auto tail, uint32_t grid) {
                with_flag(fullStats, [&](auto stats) { with_flag(wide, [&](auto w) {
                    hipLaunchKernelGGL((pt_wf_trace_refill<PT_FLAG(stats), PT_FLAG(tail), PT_FLAG(w) ? 128u : 64u>), dim3(grid), dim3(64), 0, stream, S, B, it);
                }); });
                launches++;
            };
            refill(std::false_type{}, blocks);
            if (PT_WF_SUSPEND > 0u) refill(std::true_type{}, (blocks + PT_WF_TAIL_GROUP - 1u) / PT_WF_TAIL_GROUP);
        } else {
            if (trace == Trace::Persist) {
                const uint32_t numChunks = (B.numSlots + PT_WF_CHUNK - 1u) / PT_WF_CHUNK;
                uint32_t waves = B.residentWaves;
                if (waves > numChunks) waves = numChunks;
                with_flag(fullStats, [&](auto stats) {
                    hipLaunchKernelGGL(pt_wf_trace_persist<PT_FLAG(stats)>, dim3(waves), dim3(64), 0, stream, S, B, it);
                });
            } else if (trace == Trace::RefillTlas) {
                const uint32_t refillBlocks = (B.numSlots + PT_WF_RANGE - 1u) / PT_WF_RANGE;                 // one wave per range
                const bool shared = PT_WF_TLAS_WG_WAVES > 1u && S.tlasNodeCount <= 0xFFFFu;     // several waves per workgroup: 16-bit TLAS stack entries
                with_flag(fullStats, [&](auto stats) { with_flag(shared, [&](auto sh) {
                    constexpr uint32_t WAVES = PT_FLAG(sh) ? PT_WF_TLAS_WG_WAVES : 1u;
                    hipLaunchKernelGGL((pt_wf_trace_refill_tlas<PT_FLAG(stats), WAVES>), dim3((refillBlocks + WAVES - 1u) / WAVES), dim3(64u * WAVES), 0, stream, S, B, it);
                }); });
            } else {
                with_flag(fullStats, [&](auto stats) { with_flag(tlas, [&](auto tl) {
                    hipLaunchKernelGGL((pt_wf_trace<PT_FLAG(stats), PT_FLAG(tl)>), dim3(nb * 3u), dim3(256), 0, stream, S, B, it);
                }); });
            }
            launches++;
        }
        if constexpr (!kList && !kRays) {
            if (repack) { if ((e = pt_launch_repack_shade(S, P, tm, B, fullStats, it, stream)) != hipSuccess) return e; }
        }
        if (!repack) with_flag(fullStats, [&](auto stats) {
            hipLaunchKernelGGL((pt_wf_shade<PT_FLAG(stats), MAP>), dim3(B.numSlots / PT_WF_SHADE_BLOCK), dim3(PT_WF_SHADE_BLOCK), 0, stream, S, P, tm, B, it);
        });
        launches++;
        if (repack && pt_wf_repack_candidate(it, iterations, spp)) {
            if ((e = pt_launch_repack(B, PT_WF_REPACK_FILL_NUM, PT_WF_REPACK_FILL_DEN, firstCandidate, L.repackStats, stream)) != hipSuccess) return e;
            firstCandidate = false;
            launches += 4;
        }
    }
    const uint32_t cleanupBlocks = nb < 1024u ? nb : 1024u;          // 256 CUs x 4 workgroups; each strides over the slot blocks
    if constexpr (!kList && !kRays) {
        if (repack) { if ((e = pt_launch_repack_cleanup(S, P, tm, B, fullStats, cleanupBlocks, stream)) != hipSuccess) return e; }
    }
    if (!repack) with_flag(fullStats, [&](auto stats) { with_flag(!UNIT_A && tlas, [&](auto tl) {
        constexpr bool TLAS = !UNIT_A && PT_FLAG(tl);                 // unit A renders flat scenes only
        hipLaunchKernelGGL((pt_wf_cleanup<PT_FLAG(stats), TLAS, MAP>), dim3(cleanupBlocks), dim3(256), 0, stream, S, P, tm, B);
    }); });
    if (L.orderAfter && (e = hipStreamWaitEvent(stream, L.orderAfter, 0)) != hipSuccess) return e;
    if (L.zeroOutputFirst &&
        (e = hipMemsetAsync(output, 0, (size_t)P.OutputWidth * P.OutputHeight * sizeof(float4), stream)) != hipSuccess) return e;
    if constexpr (kRays) {
        if (gather) { if ((e = pt_launch_gather_resolve(L.gather, B, (PTIrradiance*)L.output, stream)) != hipSuccess) return e; }
        else if (probe) { if ((e = pt_launch_probe_resolve(L.probe, B, (PTProbeCoeffs*)L.output, stream)) != hipSuccess) return e; }
        else hipLaunchKernelGGL(pt_wf_resolve_rays, dim3(nbPass), dim3(256), 0, stream, P, tm, B, (PTRadiance*)L.output);
    } else if constexpr (kList) {
        // pixels outside the list keep Accumulated, bit for bit: one copy of the frame, then the resolve overwrites the listed blocks
        if (L.accumulated &&
            (e = hipMemcpyAsync(output, L.accumulated, (size_t)P.OutputWidth * P.OutputHeight * sizeof(float4), hipMemcpyDeviceToDevice, stream)) != hipSuccess) return e;
    }
    if constexpr (!kRays)
        hipLaunchKernelGGL(pt_wf_resolve<MAP>, dim3(nbPass), dim3(256), 0, stream, P, batch, tm, B, (const float4*)(repack ? B.pixsum : B.color), L.accumulated, output);
    hipLaunchKernelGGL(pt_wf_fold_rows, dim3(256), dim3(256), 0, stream, B.statRows, B.numStatRows, L.counters);
    launches += 3;
    if (launchesOut) *launchesOut = launches;
    return hipGetLastError();
}
#undef PT_FLAG

// the slot mapping picks the instantiation; what a mapping never uses is cleared here, whatever the caller left in it
template <bool UNIT_A>
hipError_t launch_mapped(const PTWfLaunch& L, uint32_t* launchesOut)
{
    PTWfLaunch M = L;
    switch (L.mapKind) {
    case PT_WF_MAP_TILES:
        return launch_sequence<PTTileMap, UNIT_A>(M, M.tiles, launchesOut);
    case PT_WF_MAP_LIST:
        M.zeroOutputFirst = false;
        return launch_sequence<PTListMap, UNIT_A>(M, M.list, launchesOut);
    case PT_WF_MAP_RAYS:
        M.batch = PTBatch{};
        M.batch.count = 1u;
        M.accumulated = nullptr;
        M.orderAfter = nullptr;
        M.zeroOutputFirst = false;
        return launch_sequence<PTRayMap, UNIT_A>(M, M.rays, launchesOut);
    case PT_WF_MAP_GATHER:
    case PT_WF_MAP_PROBE: {
        // the ray map's kernels with one sample per slot: they never call its Source, so there is no list behind it
        const PTRayMap slots = {nullptr, L.mapKind == PT_WF_MAP_PROBE ? L.probe.entries * L.probe.samples : L.gather.entries * L.gather.samples};
        PTFrameParams P1 = *L.params;
        P1.SamplesPerPass = 1;
        M.params = &P1;
        M.batch = PTBatch{};
        M.batch.count = 1u;
        M.accumulated = nullptr;
        M.orderAfter = nullptr;
        M.zeroOutputFirst = false;
        return launch_sequence<PTRayMap, UNIT_A>(M, slots, launchesOut);
    }
    }
    return hipErrorInvalidValue;
}
} // namespace

#ifdef PT_WF_TU_B
// what every library links once: the arena layout and the launcher's entry point
size_t pt_wf_arena_bytes(uint32_t numSlots, uint32_t residentWaves, bool needTlas, uint32_t maxIterations)
{
    PTWfBuffers B = {};
    return pt_wf_arena_layout(nullptr, numSlots, residentWaves, needTlas, maxIterations, B);
}
PTWfBuffers pt_wf_arena_carve(void* base, uint32_t numSlots, uint32_t residentWaves, bool needTlas, uint32_t maxIterations)
{
    PTWfBuffers B = {};
    pt_wf_arena_layout((char*)base, numSlots, residentWaves, needTlas, maxIterations, B);
    return B;
}
hipError_t pt_wf_launch_unit_a(const PTWfLaunch& L, uint32_t* launchesOut);       // the other compilation of this file
hipError_t pt_launch_wavefront(const PTWfLaunch& L, uint32_t* launchesOut)
{
    if (L.schedule < 1 || L.schedule > 4) return hipErrorInvalidValue;
    if (L.schedule == 4 && L.mapKind != PT_WF_MAP_TILES) return hipErrorNotSupported;
    // the default schedule on a flat scene -- refill trace + shade -- runs the kernels built without the post-RA scheduler
    if (L.schedule == 1 && L.scene->hasTlas == 0u) return pt_wf_launch_unit_a(L, launchesOut);
    return launch_mapped<false>(L, launchesOut);
}
#else
hipError_t pt_wf_launch_unit_a(const PTWfLaunch& L, uint32_t* launchesOut) { return launch_mapped<true>(L, launchesOut); }
#endif
