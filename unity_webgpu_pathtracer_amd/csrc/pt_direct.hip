// pt_direct.hip — direct light at first hits (include/ptmi_plugin.h Part 24).
//
//     pt_direct_rays        one lane per entry: three 16-byte loads of terms, two each of the ray and the receiver; the lights
//                           walked through wave-uniform scalar loads; per pair two 16-byte stores of the ray and one of the
//                           contribution
//     pt_direct_accumulate  one lane per entry: row 1 of the terms, per pair a 16-byte load of the hit and one of the contribution
//     pt_direct_light[_tlas]  the hot path, shaped as pt_query.hip's kernels: one entry per lane, one 64-lane wave per workgroup,
//                           the grid capped at the resident waves and walking the list grid-stride.  pt_shade_hit.h's front
//                           (records, material fetch, terms), then a wave-uniform loop over (light, stratum): the light's record
//                           and derived rows arrive through scalar loads, every lane evaluates its pair, the wave walks towards
//                           that light together when any lane's pair counts (the others sit the walk out), the contribution is
//                           added when nothing was hit.  Terms, O, N, Vd and the running sum stay in registers; nothing per pair
//                           is stored.  What only a chunk's front reads of the kernel's arguments is read from the argument
//                           segment again per chunk, so neither kernel spills a scalar register.  The CWBVH stack is the ray
//                           queries' (pt_device.h's resident_wave_stack: PT_Q_LDS_STACK entries per lane in LDS, the rest in the
//                           context's slab); the HAS_TLAS kernel hands traverse_tlas a TLAS stack in LDS too (TlasStackLds, 32
//                           entries per lane), so neither kernel has scratch.
//     pt_direct_light_grid[_tlas]  the same body over a light grid (Part 25): after the front a lane takes the
//                           list of its O's cell; the wave visits the union of its lanes' lists in ascending light index -- a
//                           cross-lane minimum of the list heads per visited light -- and makes up the draws of the rectangle
//                           lights it jumps over.  The front, the pair, the walk, the sum and the output are written once
//                           (direct_light_body<TLAS, CULLED>), so are the bits.
//
// The arithmetic is direct_rule.h's, which the host twins evaluate too; the walks are the render's (pt_device.h), called, not copied.
#include "pt_device.h"
#include "pt_launch.h"
#include "pt_shade_hit.h"
#include "direct_rule.h"
#include "pt_direct.h"
#include "pt_light_grid.h"

namespace {

// light l of the scene as the rule reads it; l is the same in every lane of the wave: six scalar loads
PT_DEV ptdirect::Light uniform_light(const DScene& S, uint32_t l)
{
    const float4 a = pt_uniform_load(S.lights, (size_t)l * 4), b = pt_uniform_load(S.lights, (size_t)l * 4 + 1), c = pt_uniform_load(S.lights, (size_t)l * 4 + 2),
                 d = pt_uniform_load(S.lights, (size_t)l * 4 + 3);
    const float4 n = pt_uniform_load(S.lightConst, (size_t)l * 4), nn = pt_uniform_load(S.lightConst, (size_t)l * 4 + 3);
    ptdirect::Light L;
    L.position[0] = a.x; L.position[1] = a.y; L.position[2] = a.z; L.type = pt_asuint(a.w);
    L.emission[0] = b.x; L.emission[1] = b.y; L.emission[2] = b.z; L.range = b.w;
    L.u[0] = c.x; L.u[1] = c.y; L.u[2] = c.z; L.area = c.w;
    L.v[0] = d.x; L.v[1] = d.y; L.v[2] = d.z;
    L.N[0] = n.x; L.N[1] = n.y; L.N[2] = n.z;
    L.NN[0] = nn.x; L.NN[1] = nn.y; L.NN[2] = nn.z;
    return L;
}

PT_DEV uint32_t scene_lights(const DScene& S) { return S.hasLights && S.lightCount > 0 ? (uint32_t)S.lightCount : 0u; }

__global__ __launch_bounds__(256) void pt_direct_rays(DScene S, PTDirectParams P, uint32_t pairsPerEntry, const PTRay* __restrict__ rays,
                                                      const PTShadeTerms* __restrict__ terms, const PTReceiver* __restrict__ receivers, uint32_t count,
                                                      uint32_t first, float4* __restrict__ outRays, float4* __restrict__ outContrib)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const float4* tp = (const float4*)terms + (size_t)i * 3;
    const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
    const PTShadeTerms T = {{t0.x, t0.y, t0.z}, t0.w, {t1.x, t1.y, t1.z}, t1.w, {t2.x, t2.y, t2.z}, t2.w};
    const bool miss = ptshade::is_miss(T);
    ptdirect::Entry e = {};
    if (!miss) {
        const float4 r0 = ((const float4*)rays)[(size_t)i * 2], r1 = ((const float4*)rays)[(size_t)i * 2 + 1];
        const float4 c0 = ((const float4*)receivers)[(size_t)i * 2], c1 = ((const float4*)receivers)[(size_t)i * 2 + 1];
        const float D[3] = {r0.w, r1.x, r1.y}, Pp[3] = {c0.x, c0.y, c0.z}, N[3] = {c1.x, c1.y, c1.z};
        ptdirect::entry_begin(T, D, Pp, N, P.minAlpha, e);
    }
    const bool centred = (P.flags & PT_DIRECT_CENTERED) != 0u;
    uint32_t s = ptdirect::entry_state(P.seed, (uint64_t)first + i);
    size_t pair = (size_t)i * pairsPerEntry;
    const uint32_t lightCount = scene_lights(S);
    for (uint32_t l = 0; l < lightCount; ++l) {
        const ptdirect::Light Lt = uniform_light(S, l);
        const uint32_t n = ptdirect::pairs_of(Lt.type, P.strata);
        for (uint32_t k = 0; k < n; ++k, ++pair) {
            float x1 = 0.5f, x2 = 0.5f;
            if (!centred && Lt.type == PT_LIGHT_TYPE_RECTANGLE) {
                x1 = pt_random_float(&s);
                x2 = pt_random_float(&s);
            }
            float dir[3] = {0.0f, 0.0f, 0.0f}, c[3] = {0.0f, 0.0f, 0.0f};
            const bool counts = !miss && ptdirect::pair_eval(e, Lt, P.strata, k, x1, x2, dir, c);
            outRays[2u * pair] = make_float4(counts ? e.O[0] : 0.0f, counts ? e.O[1] : 0.0f, counts ? e.O[2] : 0.0f, dir[0]);
            outRays[2u * pair + 1u] = make_float4(dir[1], dir[2], counts ? PT_FAR_PLANE : 0.0f, pt_asfloat(0u));
            outContrib[pair] = make_float4(c[0], c[1], c[2], 0.0f);
        }
    }
}

__global__ __launch_bounds__(256) void pt_direct_accumulate(const PTShadeTerms* __restrict__ terms, const float4* __restrict__ contrib,
                                                            const PTRayHit* __restrict__ pairHits, uint32_t count, uint32_t pairsPerEntry,
                                                            float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const float4 t1 = ((const float4*)terms)[(size_t)i * 3 + 1];
    if (!(t1.w > 0.0f)) {                                               // ptshade::is_miss
        out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float d[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0; k < pairsPerEntry; ++k) {
        const size_t pair = (size_t)i * pairsPerEntry + k;
        const float4 h = ((const float4*)pairHits)[pair], c = contrib[pair];
        if (pt_asuint(h.w) != 0xFFFFFFFFu || !(c.x > 0.0f || c.y > 0.0f || c.z > 0.0f)) continue;
        d[0] = d[0] + c.x; d[1] = d[1] + c.y; d[2] = d[2] + c.z;
    }
    out[i] = make_float4(d[0], d[1], d[2], 1.0f);
}

// what the fused kernels read of PTDirectParams, in four scalar registers; add: PTShadeMixed's second launch
struct DirectArgs {
    uint32_t strata, seed, flags;       // flags: PTDirectParams.flags | kAddBit
    float minAlpha;
};
constexpr uint32_t kAddBit = 0x80000000u;

// The fused kernels' ONE argument.  What only a chunk's front reads -- the lists and the material fetch's tables -- is read from
// the kernel-argument segment again at the head of every chunk (front_args) and is dead once the front is done: held across the
// pair loop next to what the walks read, those 17 words do not fit the scalar register file (18 spilled in the HAS_TLAS kernel).
struct LightArgs {
    DScene S;
    DirectArgs P;
    const PTRay* rays;
    const PTRayHit* hits;
    const PTRaySurface* surfaces;
    float4* out;
    uint2* slab;
    uint32_t count, first;
};
typedef const __attribute__((address_space(4))) LightArgs* pt_light_kernargs;

struct FrontArgs {
    const float4* materials;
    const uint32_t* tex;
    const float4* attrs;
    uint32_t materialCount, hasTextures;
    const PTRay* rays;
    const PTRayHit* hits;
    const PTRaySurface* surfaces;
    uint32_t seed, first;
    float minAlpha;
};

// scalar loads of the kernel's own arguments (the struct is the kernel's only argument: it starts the segment).  The empty asm
// makes the pointer a new value at every call, so the loads stay in the chunk they are written in
PT_DEV FrontArgs front_args()
{
    pt_light_kernargs K = (pt_light_kernargs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    FrontArgs f;
    f.materials = K->S.materials; f.tex = K->S.tex; f.attrs = K->S.attrs;
    f.materialCount = K->S.materialCount; f.hasTextures = K->S.hasTextures;
    f.rays = K->rays; f.hits = K->hits; f.surfaces = K->surfaces;
    f.seed = K->P.seed; f.first = K->first; f.minAlpha = K->P.minAlpha;
    return f;
}

// likewise what a pair reads between two walks (the light arrays) and what a chunk's end reads (the output)
PT_DEV void light_arrays(const float4*& lights, const float4*& lightConst)
{
    pt_light_kernargs K = (pt_light_kernargs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    lights = K->S.lights;
    lightConst = K->S.lightConst;
}
PT_DEV float4* output_array()
{
    pt_light_kernargs K = (pt_light_kernargs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    return K->out;
}

// ---- what only the culled kernels read (Part 25): the pair loop over the union of the lanes' cell lists ----
// The culled kernels' ONE argument: LightArgs first, so that front_args, light_arrays and output_array read it as they are
struct GridLightArgs {
    LightArgs A;
    PTLightGridDevice G;
};
typedef const __attribute__((address_space(4))) GridLightArgs* pt_grid_kernargs;

// what a chunk's front reads of the grid, and what a step to the next light reads: from the argument segment again, as front_args
PT_DEV PTLightGridDevice grid_args()
{
    pt_grid_kernargs K = (pt_grid_kernargs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    PTLightGridDevice g;
    for (uint32_t a = 0; a < 3u; ++a) { g.g.origin[a] = K->G.g.origin[a]; g.g.dims[a] = K->G.g.dims[a]; }
    g.g.cellSize = K->G.g.cellSize;
    g.offsets = K->G.offsets;
    g.indices = K->G.indices;
    g.rectBefore = K->G.rectBefore;
    return g;
}
PT_DEV void grid_lists(const uint32_t*& indices, const uint32_t*& rectBefore)
{
    pt_grid_kernargs K = (pt_grid_kernargs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    indices = K->G.indices;
    rectBefore = K->G.rectBefore;
}

// ... and whether the chunk's end adds to the output (kAddBit): held across the pair loop, the flag spills in the HAS_TLAS kernel
PT_DEV bool add_to_output()
{
    pt_light_kernargs K = (pt_light_kernargs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    return (K->P.flags & kAddBit) != 0u;
}

// word `index` of p through a scalar load; p + index must be the same address in every lane of the wave
PT_DEV uint32_t uniform_word(const uint32_t* p, size_t index)
{
    const __attribute__((address_space(4))) uint32_t* q = (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)p;
    return q[index];
}

// the smallest v of the wave's 64 lanes, in a scalar register; every lane is active where this is called
PT_DEV uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = o < v ? o : v;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The next light of the union of the lanes' lists: the wave-wide minimum of the heads (kNoLight: every list is used up).  The
// lanes whose head it is advance their cursor.  Without `centred` every lane makes the draws PTDirectLight makes for the rectangle
// lights jumped over, drawn ... l - 1: two per pair, S * S pairs each -- integer-only, the trip count is the wave's
PT_DEV uint32_t next_light(uint32_t& head, uint32_t& cur, uint32_t end, uint32_t& s, uint32_t& drawn, bool centred, uint32_t strata)
{
    const uint32_t l = wave_min(head);
    if (l == ptlgrid::kNoLight) return l;
    const uint32_t *indices, *rectBefore;
    grid_lists(indices, rectBefore);
    if (head == l) {
        ++cur;
        head = cur < end ? indices[cur] : ptlgrid::kNoLight;
    }
    if (!centred) {
        const uint32_t* rb = (const uint32_t*)__builtin_assume_aligned(rectBefore, 4);
        const uint32_t skipped = uniform_word(rb, l) - uniform_word(rb, (uint32_t)__builtin_amdgcn_readfirstlane((int)drawn));
        for (uint32_t n = 2u * strata * strata * skipped; n != 0u; --n) pt_rng_next(&s);
    }
    drawn = l + 1u;
    asm volatile("" : "+v"(drawn));                                     // held in a vector register across the walk: the scalar file is full there
    return l;
}

// The four kernels' body.  CULLED: the pair loop steps through the union of the lanes' cell lists (next_light) where the others
// step through every light of the scene; a lane takes its list after the front.  Nothing else differs but two switches for
// scalar-register pressure, marked where they stand: the chunk loop's step (CULLED && TLAS) and the add flag (CULLED || TLAS).
template <bool TLAS, bool CULLED>
PT_DEV void direct_light_body(const LightArgs& A)
{
    const DScene& S = A.S;                                              // the walks' fields: live throughout
    const DirectArgs& P = A.P;
    const uint32_t count = A.count;
    __shared__ uint32_t s_tstack[TLAS ? PT_BVH_STACK_SIZE : 1][64];
    const uint32_t lane = threadIdx.x;
    Counters cn = {};
    TravStackT<PT_Q_LDS_STACK, true> st;
    resident_wave_stack(st, A.slab);
    const pt_lds_column tstack = (pt_lds_column)&s_tstack[0][lane];

    const bool centred = (P.flags & PT_DIRECT_CENTERED) != 0u;
    const uint32_t lightCount = scene_lights(S);
    // The chunk loop's step.  Left to the compiler, the pointer it is loaded through at every chunk's end is held in two scalar
    // registers across the pair loop; the culled HAS_TLAS kernel has none to spare (they spill) and holds the step itself, in one
    uint32_t step = 0u;
    if (CULLED && TLAS) {
        step = gridDim.x * 64u;
        asm volatile("" : "+s"(step));
    }
    for (uint32_t base = blockIdx.x * 64u; base < count; base += CULLED && TLAS ? step : gridDim.x * 64u) {     // base is wave-uniform: no lane leaves early
        const uint32_t i = base + lane;
        const bool active = i < count;
        bool hit = false;
        ptdirect::Entry e = {};
        uint32_t s;
        {
            const FrontArgs f = front_args();
            DScene Sf = {};                                             // the scene as the material fetch reads it
            Sf.materials = f.materials; Sf.tex = f.tex; Sf.attrs = f.attrs;
            Sf.materialCount = f.materialCount; Sf.hasTextures = f.hasTextures;
            if (active) {
                HitRecords h;
                hit_records(Sf, f.rays, f.hits, f.surfaces, i, nullptr, nullptr, 0u, h);
                hit = !ptshade::is_miss(h.T);
                if (hit) {
                    const float4 r0 = ((const float4*)f.rays)[(size_t)i * 2], r1 = ((const float4*)f.rays)[(size_t)i * 2 + 1];
                    const float D[3] = {r0.w, r1.x, r1.y};
                    ptdirect::entry_begin(h.T, D, h.P, h.N, f.minAlpha, e);
                }
            }
            s = ptdirect::entry_state(f.seed, (uint64_t)f.first + i);
        }
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
        const v3 o = mk3(e.O[0], e.O[1], e.O[2]);
        // CULLED: the lane's cursor into its cell's list and the light at it; a miss holds an empty list.  drawn: the lights below
        // it have had their draws
        uint32_t cur = 0u, end = 0u, head = ptlgrid::kNoLight, drawn = 0u;
        if (CULLED && hit) {                                            // the front's arguments are dead: the grid's fit the scalar file now
            const PTLightGridDevice G = grid_args();
            const uint32_t cell = ptlgrid::cell_of(G.g, e.O);
            cur = G.offsets[cell];
            end = G.offsets[cell + 1u];
            if (cur < end) head = G.indices[cur];
        }
        // one loop over the pairs (l, k), both wave-uniform.  The light's 24 words are loaded again for every pair (scalar-cache
        // hits) instead of being held in scalar registers across the walk, where the scene's pointers already fill the file
        for (uint32_t l = CULLED ? next_light(head, cur, end, s, drawn, centred, P.strata) : 0u, k = 0;
             CULLED ? l != ptlgrid::kNoLight : l < lightCount;) {
            DScene Sl = {};
            light_arrays(Sl.lights, Sl.lightConst);
            const ptdirect::Light Lt = uniform_light(Sl, l);
            if (k >= ptdirect::pairs_of(Lt.type, P.strata)) {
                l = CULLED ? next_light(head, cur, end, s, drawn, centred, P.strata) : l + 1u;
                k = 0;
                continue;
            }
            float x1 = 0.5f, x2 = 0.5f;
            if (!centred && Lt.type == PT_LIGHT_TYPE_RECTANGLE) {
                x1 = pt_random_float(&s);
                x2 = pt_random_float(&s);
            }
            float dir[3], c[3];
            const bool counts = hit && ptdirect::pair_eval(e, Lt, P.strata, k, x1, x2, dir, c);
            ++k;
            if (!__any(counts)) continue;                               // no lane's pair counts: no walk
            if (counts) {
                HitRecord rec = miss_record(PT_FAR_PLANE);
                const v3 d = mk3(dir[0], dir[1], dir[2]);
                if (TLAS) traverse_tlas<false, TlasStackLds>(S, o, d, /*isShadow*/ true, rec, st, cn, tstack);
                else traverse_cwbvh<false>(S, o, d, true, rec.h, st, cn, PT_FAR_PLANE);
                if (rec.h.triIndex == 0xFFFFFFFFu) { d0 = d0 + c[0]; d1 = d1 + c[1]; d2 = d2 + c[2]; }
            }
        }
        if (active) {
            float4* out = output_array();
            // held across the pair loop, the flag spills in the HAS_TLAS kernels and costs the flat culled one registers: only the
            // flat kernel over every light holds it, the others read it again (add_to_output)
            const bool add = CULLED || TLAS ? add_to_output() : (P.flags & kAddBit) != 0u;
            if (add) {
                if (hit) {
                    const float4 v = out[i];
                    out[i] = make_float4(v.x + d0, v.y + d1, v.z + d2, v.w);
                }
            } else {
                out[i] = hit ? make_float4(d0, d1, d2, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    }
}

} // namespace

// Stable, unmangled kernel names (rocprofv3 --kernel-trace lists them as they are written here).
extern "C" __global__ __launch_bounds__(64) void pt_direct_light(LightArgs A) { direct_light_body<false, false>(A); }
extern "C" __global__ __launch_bounds__(64) void pt_direct_light_tlas(LightArgs A) { direct_light_body<true, false>(A); }
extern "C" __global__ __launch_bounds__(64) void pt_direct_light_grid(GridLightArgs A) { direct_light_body<false, true>(A.A); }
extern "C" __global__ __launch_bounds__(64) void pt_direct_light_grid_tlas(GridLightArgs A) { direct_light_body<true, true>(A.A); }

hipError_t pt_direct_grid_caps(int device, uint32_t caps[2])
{
    void (*const kernels[2])(LightArgs) = {pt_direct_light, pt_direct_light_tlas};
    return pt_resident_wave_caps(device, kernels, 2, caps);
}

hipError_t pt_direct_culled_grid_caps(int device, uint32_t caps[2])
{
    void (*const kernels[2])(GridLightArgs) = {pt_direct_light_grid, pt_direct_light_grid_tlas};
    return pt_resident_wave_caps(device, kernels, 2, caps);
}

hipError_t pt_launch_direct_rays(const DScene& S, const PTDirectParams& P, uint32_t pairsPerEntry, const PTRay* rays, const PTShadeTerms* terms,
                                 const PTReceiver* receivers, uint32_t count, uint32_t first, PTRay* outRays, float4* outContrib, hipStream_t stream)
{
    if (count == 0u || pairsPerEntry == 0u) return hipSuccess;
    if (!ptdirect::strata_ok(P.strata) || (uint64_t)count * pairsPerEntry > (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_direct_rays, dim3((count + 255u) / 256u), dim3(256), 0, stream, S, P, pairsPerEntry, rays, terms, receivers, count, first,
                       (float4*)outRays, outContrib);
    return hipGetLastError();
}

hipError_t pt_launch_direct_accumulate(const PTShadeTerms* terms, const float4* contrib, const PTRayHit* pairHits, uint32_t count, uint32_t pairsPerEntry,
                                       float4* out, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    if ((uint64_t)count * pairsPerEntry > (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_direct_accumulate, dim3((count + 255u) / 256u), dim3(256), 0, stream, terms, contrib, pairHits, count, pairsPerEntry, out);
    return hipGetLastError();
}

hipError_t pt_launch_direct_light(const DScene& S, const PTDirectParams& P, const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces,
                                  uint32_t count, uint32_t first, float4* out, bool add, uint2* slab, uint32_t gridCap, hipStream_t stream,
                                  const PTLightGridDevice* lightGrid)
{
    if (count == 0u) return hipSuccess;
    if (!ptdirect::strata_ok(P.strata) || !slab || gridCap == 0u) return hipErrorInvalidValue;
#ifdef PT_D_GRID_CAP
    gridCap = gridCap < PT_D_GRID_CAP ? gridCap : PT_D_GRID_CAP;         // the stress build: every wave takes several chunks of a short list
#endif
    const uint32_t chunks = (count + 63u) / 64u;
    const uint32_t grid = chunks < gridCap ? chunks : gridCap;
    const LightArgs A = {S, {P.strata, P.seed, P.flags | (add ? kAddBit : 0u), P.minAlpha}, rays, hits, surfaces, out, slab, count, first};
    if (lightGrid) {
        if (!lightGrid->offsets || !lightGrid->indices || !lightGrid->rectBefore) return hipErrorInvalidValue;
        const GridLightArgs GA = {A, *lightGrid};
        if (S.hasTlas) hipLaunchKernelGGL(pt_direct_light_grid_tlas, dim3(grid), dim3(64), 0, stream, GA);
        else hipLaunchKernelGGL(pt_direct_light_grid, dim3(grid), dim3(64), 0, stream, GA);
        return hipGetLastError();
    }
    if (S.hasTlas) hipLaunchKernelGGL(pt_direct_light_tlas, dim3(grid), dim3(64), 0, stream, A);
    else hipLaunchKernelGGL(pt_direct_light, dim3(grid), dim3(64), 0, stream, A);
    return hipGetLastError();
}
