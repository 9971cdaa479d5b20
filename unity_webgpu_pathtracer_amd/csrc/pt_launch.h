// pt_launch.h — host-visible launcher declarations shared by the kernel files and the host API (pt_context.h, pt_api_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"

// Which 16x16-pixel blocks this context renders (PTSetTileOwnership) and how much of the frame the
// dispatch covers (PTFrameParams.DispatchGroupsX/Y, PathTracer.cs:203-208).
struct PTTileMap {
    uint32_t rank, world;
    uint32_t blocksX, blocksY;     // ceil(coverW/16), ceil(coverH/16)
    uint32_t coverW, coverH;       // pixels with x < coverW && y < coverH are rendered
};

// slot <-> pixel: owned 16x16 blocks in row-major order of (block row, k-th owned block of that row), 256 slots per block,
// one wave per 8x8 tile.  Shared by the megakernel, the wavefront schedules and the tile pack / unpack of the multi-GPU gather.
__host__ __device__ inline uint32_t pt_num_slots(const PTTileMap& tm)
{
    const uint32_t bpr = (tm.blocksX + tm.world - 1u) / tm.world;       // owned blocks per block-row (upper bound)
    return bpr * tm.blocksY * 256u;
}
__host__ __device__ inline bool pt_slot_to_pixel(const PTTileMap& tm, uint32_t slot, uint32_t& px, uint32_t& py)
{
    const uint32_t bpr = (tm.blocksX + tm.world - 1u) / tm.world;
    const uint32_t block = slot >> 8, tid = slot & 255u;
    const uint32_t by = block / bpr, k = block % bpr;
    const uint32_t first = (uint32_t)(((int)tm.rank - (int)(by % tm.world) + (int)tm.world) % (int)tm.world);
    const uint32_t bx = first + k * tm.world;
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    px = bx * 16u + (wave & 1u) * 8u + (lane & 7u);
    py = by * 16u + (wave >> 1) * 8u + (lane >> 3);
    return bx < tm.blocksX && by < tm.blocksY && px < tm.coverW && py < tm.coverH;
}
inline PTTileMap pt_make_tile_map(const PTFrameParams& p, int rank, int world)
{
    PTTileMap tm;
    tm.rank = (uint32_t)rank;
    tm.world = (uint32_t)world;
    uint32_t covW = p.OutputWidth, covH = p.OutputHeight;
    if (p.DispatchGroupsX && p.DispatchGroupsX * 8u < covW) covW = p.DispatchGroupsX * 8u;
    if (p.DispatchGroupsY && p.DispatchGroupsY * 8u < covH) covH = p.DispatchGroupsY * 8u;
    tm.coverW = covW; tm.coverH = covH;
    tm.blocksX = (covW + 15u) / 16u;
    tm.blocksY = (covH + 15u) / 16u;
    return tm;
}

// multi-GPU frame assembly (pt_tiles.hip): packed[slot] = frame[pixel(slot)] and back
hipError_t pt_launch_pack_tiles(const PTTileMap& tm, uint32_t frameWidth, const float4* frame, float4* packed, hipStream_t stream);
hipError_t pt_launch_unpack_tiles(const PTTileMap& tm, uint32_t frameWidth, const float4* packed, float4* frame, hipStream_t stream);

// per-light constants (pt_device.h derive_light_rows): S.lights / S.lightCount must be set; lightConst holds 64 bytes per light
hipError_t pt_launch_derive_lights(const DScene& S, float4* lightConst, hipStream_t stream);

hipError_t pt_launch_megakernel(const DScene& S, const PTFrameParams& P, const float4* accumulated, float4* output,
                                const PTTileMap& tm, unsigned long long* gstats, bool fullStats, hipStream_t stream);

hipError_t pt_launch_process_mesh(const PTMeshDesc& M, const void* dVertexBuffer, const void* dIndexBuffer, float4* dVertexPositions,
                                  float4* dTriangleAttributes, hipStream_t stream);
hipError_t pt_launch_copy_texture(const float4* dTexture, uint32_t width, uint32_t height, uint32_t dataOffset, uint32_t descriptorOffset,
                                  int hasAlpha, uint32_t* dTextureData, hipStream_t stream);
hipError_t pt_launch_present(const PTPresentParams& Q, const float4* src, float4* dst, hipStream_t stream);

// ---- the resident-wave kernels (pt_query.hip, pt_denoise.hip's guides, pt_direct.hip): one 64-lane wave per workgroup, walking
// with pt_device.h's resident_wave_stack ----
// caps[k] = resident workgroups per device of kernels[k] (occupancy x CUs): its grid cap, and the slab waves it needs
template <class Kernel>
inline hipError_t pt_resident_wave_caps(int device, const Kernel* kernels, int n, uint32_t* caps)
{
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return e;
    for (int k = 0; k < n; ++k) {
        int blocks = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, reinterpret_cast<const void*>(kernels[k]), 64, 0);
        if (e != hipSuccess) return e;
        caps[k] = (uint32_t)(blocks > 0 ? blocks : 1) * (uint32_t)prop.multiProcessorCount;
    }
    return hipSuccess;
}
// bytes of one wave's slab rows (64 lanes x PT_Q_SLAB_ENTRIES); defined in pt_query.hip, so the stress build's value is its kernels'
size_t pt_resident_wave_slab_bytes();

// ---- ray queries (pt_query.hip): mode PT_QUERY_CLOSEST / PT_QUERY_ANY_HIT / 2 = closest + surface ----
#define PT_QUERY_KERNELS 12
inline int pt_query_kernel_index(bool tlas, uint32_t mode, bool stats) { return ((tlas ? 3 : 0) + (int)mode) * 2 + (stats ? 1 : 0); }
hipError_t pt_query_grid_caps(int device, uint32_t caps[PT_QUERY_KERNELS]);
// count <= 2^31; rays: 2 float4 per ray, hits: 1 float4 per ray, surface (mode 2): 3 float4 per ray; slab holds >= gridCap waves
hipError_t pt_launch_query(const DScene& S, const float4* rays, uint32_t count, uint32_t mode, bool stats, float4* hits,
                           float4* surface, uint2* slab, uint32_t gridCap, unsigned long long* gstats, hipStream_t stream);

// ---- guides and denoising (pt_denoise.hip) ----
// the two guide kernels (flat, HAS_TLAS)
hipError_t pt_guide_grid_caps(int device, uint32_t caps[2]);
// n x n sub-pixel samples per pixel of P's OutputWidth x OutputHeight; albedo / normalDepth: one float4 per pixel each
hipError_t pt_launch_guides(const DScene& S, const PTFrameParams& P, uint32_t n, float4* albedo, float4* normalDepth, uint2* slab,
                            uint32_t gridCap, hipStream_t stream);
struct PTDenoiseArgs {
    uint32_t width, height;
    float sigmaL, sigmaN, sigmaZ;
    uint32_t flags;
};
// where the prepass takes v from: the moment planes of PTAccumulateMoments (Srr Sgg Sbb Sll | Srg Srb Sgb 0) and 1 / ((k - 1) W)
struct PTDenoiseVariance {
    const float4* plane0;
    const float4* plane1;
    float invDof;
    const float* blockInvDof = nullptr;      // NULL = invDof everywhere; else one value per 16x16 block (row-major, ceil(width/16) per row)
};
// iterations >= 1 levels: prepass, one launch per level, remodulation (iterations + 2 launches); every buffer width*height.
// variance == nullptr: the 3x3 spatial variance of PTDenoise; else the variance of the mean from the moments (PTDenoiseMoments)
hipError_t pt_launch_denoise(const PTDenoiseArgs& A, int iterations, const float4* src, float4* dst, const float4* albedo,
                             const float4* normalDepth, float4* state0, float4* state1, float2* gradz,
                             const PTDenoiseVariance* variance, hipStream_t stream);

// ---- per-pixel moments across passes and the noise metric (pt_moments.hip) ----
// plane0 / plane1 += the Welford term of (out - acc) times f, per pixel (include/ptmi_plugin.h Part 6)
hipError_t pt_launch_moments_accumulate(uint32_t pixels, float f, const float4* out, const float4* acc, float4* plane0,
                                        float4* plane1, hipStream_t stream);
// the same update over the listed 16x16 blocks only: entry e = {block id = by * ceil(width/16) + bx, the bits of the block's f}
hipError_t pt_launch_moments_accumulate_blocks(uint32_t entries, const uint2* table, uint32_t width, uint32_t height, const float4* out,
                                               const float4* acc, float4* plane0, float4* plane1, hipStream_t stream);
// words of the statistics buffer: 256 histogram bins, then the maximum's bits, pixelsBelow, the sum of eps (float bits)
enum : uint32_t { PT_NOISE_MAX = 256, PT_NOISE_BELOW, PT_NOISE_SUM, PT_NOISE_WORDS };
struct PTNoiseArgs {
    uint32_t width, height;
    uint32_t rank, world;           // block (bx, by) is counted when (bx + by) % world == rank
    float invDof, relFloor, threshold;
};
// stats: PT_NOISE_WORDS zeroed words; blockSums / tiles: ceil(width/16) * ceil(height/16) floats each.
// blockInvDof: NULL = A.invDof everywhere; else one value per 16x16 block of the tile map (adaptive sampling)
hipError_t pt_launch_noise(const PTNoiseArgs& A, const float4* frame, const float4* plane0, uint32_t* stats, float* blockSums,
                           float* tiles, hipStream_t stream, const float* blockInvDof = nullptr);

// ---- schedule 1 (wavefront): slot-indexed path state in HBM (see pt_wavefront.hip) ----
// float4 arrays of a state set, in carving order.  PT_F4_RAY0/1/2 are the RAY RECORDS of the three ray kinds a slot can have in
// flight (bounce ray, environment NEE, light NEE): 32 bytes per slot and kind, {origin.xyz, w0, direction.xyz, w1} at
// float4 index 2 * slot -- so each takes TWO strides.  A trace lane fetches its ray as one 32-byte read inside one 64-byte
// sector; round 2 kept origins and directions in separate 16-byte arrays and fetched two sectors per ray (12.2 GB of sectors
// per pass for 2.9 GB of rays).  w0 / w1 of the bounce record carry scatterPdf / maxRoughness.
enum : uint32_t { PT_F4_RAY0 = 0, PT_F4_RAY1 = 2, PT_F4_RAY2 = 4, PT_F4_RAD = 6, PT_F4_THR, PT_F4_COLOR, PT_F4_ENVC, PT_F4_LIGHTC,
                  PT_F4_PTHR, PT_F4_HIT, PT_F4_HIT2, PT_F4_PIXSUM, PT_F4_COUNT };
#ifndef PT_WF_LDS_STACK
#define PT_WF_LDS_STACK 8       // traversal-stack entries per lane kept in LDS by the refill / persistent trace kernels; deeper ones go to stackSpill
#endif
// HAS_TLAS refill kernel (pt_wf_trace_refill_tlas): waves per workgroup sharing one LDS copy of the top of the TLAS (1 = one-wave
// workgroups, nodes from memory), nodes in that copy (64 bytes each), CWBVH stack entries per lane kept in LDS by that variant.
// 8 waves x (4 x 512 B CWBVH stack + 8 x 128 B TLAS stack + 256 B exchange) + 400 x 64 B = 52.2 KB: three workgroups = 24 waves per CU.
// Measured (200-instance scene, 1080p / 8 spp, round 3): 1 wave 2,327 Mrays/s, 8 waves with all 399 nodes in LDS 2,155, 8 waves with
// one node in LDS 2,043 -- the copy is worth 6 %, the eight-wave workgroup costs 12 %: the TLAS walk is not bound by where its nodes
// come from.  Default 1; the stress build (csrc/Makefile) runs the 8-wave variant through the parity suite.
#ifndef PT_WF_TLAS_WG_WAVES
#define PT_WF_TLAS_WG_WAVES 1u
#endif
#ifndef PT_WF_TLAS_CACHE_NODES
#define PT_WF_TLAS_CACHE_NODES 400u
#endif
#ifndef PT_WF_TLAS_CHUNK
#define PT_WF_TLAS_CHUNK 64u     // slots per chunk the waves of such a workgroup take from their shared range (power of two <= 64 x ... <= PT_WF_RANGE)
#endif
#ifndef PT_WF_TLAS_BLAS_LDS_STACK
#define PT_WF_TLAS_BLAS_LDS_STACK (PT_WF_LDS_STACK < 4 ? PT_WF_LDS_STACK : 4)
#endif
// entries per slab row: the deepest overflow any trace kernel of the build can have
#define PT_WF_SPILL_ROW_ENTRIES (PT_BVH_STACK_SIZE - (PT_WF_TLAS_BLAS_LDS_STACK < PT_WF_LDS_STACK ? PT_WF_TLAS_BLAS_LDS_STACK : PT_WF_LDS_STACK))
struct PTWfBuffers {
    uint32_t* flags;            // [numSlots] packed state word
    uint32_t* rng;              // [numSlots]
    float4* ray[3];             // [2 * numSlots] each: ray records of kind 0 (bounce ray: origin, scatterPdf | direction, maxRoughness), 1 (environment NEE), 2 (light NEE)
    float4 *rad, *thr, *color;  // radiance, throughput, per-pixel sample sum
    float4 *envC, *lightC, *pthr;        // contributions of the two NEE rays and the throughput they apply to
    float4* hit;                // [numSlots] (t, u, v, triIndex bits) written by trace kind 0
    float4* hit2;               // [numSlots] HAS_TLAS only: (world hit position, instance index bits)
    float4* pixsum;             // [numSlots] schedule 4 only: a finished pixel's sample sum, indexed by PIXEL slot (the other arrays by context)
    // The float4 arrays above are carved back to back at a fixed stride: array k starts at f4base + k * f4stride
    // (order: PT_F4_*).  The trace kernels address them this way -- one base pointer instead of seven -- because at 8 waves/SIMD a
    // wave may hold 80 SGPRs, and every pointer costs two.
    float4* f4base;
    uint32_t f4stride;          // in float4 elements
    uint8_t* occl;              // [2][numSlots] written by trace kinds 1, 2
    uint2* stackSpill;          // [numSlots / 64 waves x 64 lanes][32 - PT_WF_LDS_STACK]: traversal-stack entries beyond the LDS part (refill / persistent trace kernels)
    uint32_t* tlasSpill;        // [numSlots][32]: HAS_TLAS refill kernel, TLAS-stack entries beyond its LDS part (allocated for HAS_TLAS scenes only)
    uint4* susp;                // [numSlots / 64][PT_WF_SUSPEND][6]: suspended rays of the refill trace kernel (pt_wavefront.hip)
    uint32_t* suspCount;        // [numSlots / 64]
    uint32_t* chunkHeads;       // [8 shards x 32 words]: work counters of the persistent trace kernel, one 128-B line each
    unsigned long long* statRows;   // [numStatRows][16]
    uint32_t numSlots, numStatRows, maxIterations;
    uint32_t slotsPerPass;      // numSlots = passes of the batch x slotsPerPass; slot s belongs to pass s / slotsPerPass, pixel slot s % slotsPerPass
    uint32_t residentWaves;     // waves the device holds at the trace kernel's occupancy (CUs x 4 SIMDs x 8)
    // ---- mid-pass slot repack (pt_repack.hip, repack_rule.h).  Appended: no kernel that does not read them moves ----
    uint32_t* pixelOf;          // [numSlots] the pixel slot whose path a slot carries: the identity until a repack moves the path
    uint32_t* rpPrefix;         // [numSlots / 256] live slots per block, then their exclusive prefix
    uint32_t* rpCtl;            // [ptrepack::PT_REPACK_CTL_WORDS] the decision of the last candidate: go, L, E
    char* rpTemp;               // the temporary SoA region of a repack: rpCapacity slots x PT_WF_REPACK_SLOT_BYTES
    uint32_t rpCapacity;        // numSlots / 2
};
#define PT_WF_REPACK_SLOT_BYTES 184u     // flags, pixelOf (4 each) + three 32-byte ray records + rad, thr, color, envC, lightC (16 each): rng and pthr ride in their .w lanes

// The arena of a state set: every array of PTWfBuffers carved from one allocation of pt_wf_arena_bytes() bytes.  Both are defined
// in pt_wavefront.hip, by the one of its two compilations that every library links (-DPT_WF_TU_B), so the layout is by
// construction the one its kernels index.  needTlas: the scene is HAS_TLAS (tlasSpill); slotsPerPass is left to the caller.
size_t pt_wf_arena_bytes(uint32_t numSlots, uint32_t residentWaves, bool needTlas, uint32_t maxIterations);
PTWfBuffers pt_wf_arena_carve(void* base, uint32_t numSlots, uint32_t residentWaves, bool needTlas, uint32_t maxIterations);

// Refill trace launches: 128 slots per wave while that still gives a quarter of the device's wave slots a wave (1080p: 16,320
// waves for 8,192 slots, +2.4 %; half and quarter frames: +2 %), 64 for smaller launches.  Shared by the launcher and by the
// arena sizing (a trace wave addresses 64 slab rows and PT_WF_SUSPEND records).
#ifndef PT_WF_WIDE_DIV
#define PT_WF_WIDE_DIV 4u       // with 12 sets in flight: 1/4 of a 1080p frame 5.09 vs 5.21 ms, 1/8 equal either way
#endif
inline bool pt_wf_wide_ranges(uint32_t numSlots, uint32_t residentWaves) { return (numSlots / 128u) >= residentWaves / PT_WF_WIDE_DIV; }
// most trace waves any schedule launches over a set of numSlots slots (refill: numSlots / 64 or / 128; persistent: <= residentWaves)
inline uint32_t pt_wf_max_trace_waves(uint32_t numSlots, uint32_t residentWaves)
{
    const uint32_t narrow = (numSlots + 63u) / 64u;
    if (!pt_wf_wide_ranges(numSlots, residentWaves)) return narrow;
    const uint32_t wide = (numSlots + 127u) / 128u, persist = residentWaves < narrow ? residentWaves : narrow;
    return wide > persist ? wide : persist;
}

// A BATCH of progressive passes rendered by ONE launch sequence (PTRenderPassBatchTo): the passes differ only in RngSeedRoot and
// CurrentSample, their paths are independent (the running mean of PathTracer.compute:89-98 only meets them in the resolve kernel,
// which applies the passes in order), so a launch covers count x slotsPerPass slots.
#define PT_MAX_BATCH 8
struct PTBatch {
    uint32_t count;
    uint32_t seedRoot[PT_MAX_BATCH];
    uint32_t currentSample[PT_MAX_BATCH];
};
__host__ __device__ inline void pt_batch_pick(const PTBatch& b, uint32_t j, uint32_t& seedRoot, uint32_t& currentSample)
{
    seedRoot = b.seedRoot[0]; currentSample = b.currentSample[0];
#pragma unroll
    for (uint32_t k = 1; k < PT_MAX_BATCH; ++k) if (j == k) { seedRoot = b.seedRoot[k]; currentSample = b.currentSample[k]; }
}

// ---- adaptive passes (include/ptmi_plugin.h Part 7): a pass over a LIST of 16x16 blocks, each with its own sample count ----
// Slot s of pass j is j * slotsPerPass + e * 256 + tid with slotsPerPass = entries * 256; entry e of the per-call table is
// {block id = by * frameBlocksX + bx, the block's sample count at the start of the call}.  Inside a block the lanes are laid
// out as by pt_slot_to_pixel (four 8x8 waves).  The kernels of one call read only this snapshot (uploaded on the set's stream
// before the init kernel): a later call's init may run while this call's resolve is still pending.
struct PTListMap {
    uint32_t frameBlocksX;         // ceil(OutputWidth / 16)
    uint32_t coverW, coverH;       // pixels with x < coverW && y < coverH are rendered (pt_make_tile_map)
    const uint2* table;
};
__host__ __device__ inline bool pt_list_slot_to_pixel(uint32_t frameBlocksX, uint32_t coverW, uint32_t coverH, uint32_t blockId, uint32_t tid,
                                                      uint32_t& px, uint32_t& py)
{
    const uint32_t by = blockId / frameBlocksX, bx = blockId - by * frameBlocksX;
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    px = bx * 16u + (wave & 1u) * 8u + (lane & 7u);
    py = by * 16u + (wave >> 1) * 8u + (lane >> 3);
    return px < coverW && py < coverH;
}
// The launch sequence over the list (PTWfLaunch, below): batch.currentSample is not read (pass j of entry e renders with
// CurrentSample = table[e].y + j * spp), the whole frame is copied from `accumulated` to `output` before the resolve (when
// accumulated != NULL), nothing is zeroed, schedule 4 is not available.

// ---- radiance queries (include/ptmi_plugin.h Part 8): a launch sequence over a caller's LIST OF RAYS ----
// Slot s is entry s of the list (one pass, slotsPerPass = numSlots = count rounded up to 256; the slots past count start as
// finished).  A path depends on its "pixel" only through how a sample starts: here sample 0 is the entry's ray and RNG state, and
// every later sample reloads the entry's ray (a 32-byte vector load by slot) and draws nothing.  px, py and pixelIndex carry nothing.
struct PTRayMap {
    const PTRadianceRay* rays;     // 16-byte aligned
    uint32_t count;
};
#define PT_RADIANCE_CHUNK (1u << 21)      // most entries of one launch sequence (a state set no larger than a 1080p frame's); <= 2^23
// The launch sequence over the ray list (PTWfLaunch, below): `output` is the PTRadiance array, the resolve writes
// out[s] = {colour / (float)spp, rng} for s < count and depends on nothing but this sequence; batch, accumulated, orderAfter and
// zeroOutputFirst are not read.  Schedule 4 is not available.
// PTCameraRays (pt_kernels.hip): entry i = path_init's ray and RNG state of pixel indices[i] (NULL: pixel i); count <= 2^31
hipError_t pt_launch_camera_rays(const PTFrameParams& P, const uint32_t* indices, uint32_t count, PTRadianceRay* rays, hipStream_t stream);

// ---- irradiance gathers (include/ptmi_plugin.h Part 13; pt_gather.hip): a launch sequence over RECEIVERS x SAMPLES ----
// Slot s carries sample s % samples of entry s / samples (entry-major: neighbouring lanes share a receiver).  The sequence is the
// ray list's with two kernels exchanged: pt_wf_gather_init does the receiver step where pt_wf_init would load a ray, and
// pt_wf_gather_resolve folds an entry's samples where pt_wf_resolve_rays would write one entry per slot.  Everything between them
// is the PTRayMap instantiations of trace, shade and cleanup with SamplesPerPass forced to 1, so the Source of the ray map is never
// called (rays == NULL) and no sample ever overlaps a successor.
struct PTGatherMap {
    const PTReceiver* recv;        // 16-byte aligned
    uint32_t entries, samples;     // entries * samples <= PT_RADIANCE_CHUNK
    uint32_t firstSample;
};
// the two kernels of a gather's launch sequence on state set B, and PTGatherRays (slots [0, entries * samples) of one launch)
hipError_t pt_launch_gather_init(const DScene& S, const PTFrameParams& P, const PTGatherMap& gm, const PTWfBuffers& B, bool fullStats, hipStream_t stream);
hipError_t pt_launch_gather_resolve(const PTGatherMap& gm, const PTWfBuffers& B, PTIrradiance* out, hipStream_t stream);
hipError_t pt_launch_gather_rays(const DScene& S, const PTFrameParams& P, const PTGatherMap& gm, PTRadianceRay* rays, hipStream_t stream);

// ---- SH light probes (include/ptmi_plugin.h Part 15; pt_probe.hip): a launch sequence over PROBES x SAMPLES ----
// The gather's arrangement with its own first and last kernel: pt_wf_probe_init leaves in slot s = entry * samples + j the state
// a radiance query starts the ray {P, w_j} with, and pt_wf_probe_resolve, one wave per probe, projects the slots' colours onto
// the nine basis functions (w_j is made again from the seed, never stored) and adds the delta lights.
struct PTProbeMap {
    const PTProbe* probes;         // 16-byte aligned
    uint32_t entries, samples;     // entries * samples <= PT_RADIANCE_CHUNK
    uint32_t firstSample;
    // PT_PROBE_DELTA_LIGHTS: pair p = entry * lightCount + light of THIS chunk's entries; lightCount == 0: no delta term
    uint32_t lightCount;
    const float4* deltaRays;       // 2 per pair: the any-hit ray {P, lsDirection.x} {lsDirection.yz, tmax, 0}; tmax == 0: skipped
    const float4* deltaLi;         // 1 per pair: Li
    const float4* deltaHits;       // 1 per pair: the any-hit record (prim == 0xFFFFFFFF: visible)
};
hipError_t pt_launch_probe_init(const PTProbeMap& pm, const PTWfBuffers& B, hipStream_t stream);
hipError_t pt_launch_probe_resolve(const PTProbeMap& pm, const PTWfBuffers& B, PTProbeCoeffs* out, hipStream_t stream);
hipError_t pt_launch_probe_rays(const PTProbeMap& pm, PTRadianceRay* rays, hipStream_t stream);
// pairs [0, entries * S.lightCount) of pm.probes: the any-hit rays and Li (<= 2^28 pairs per launch)
hipError_t pt_launch_probe_delta_rays(const DScene& S, const PTProbe* probes, uint32_t entries, float4* rays, float4* li, hipStream_t stream);
hipError_t pt_launch_probe_irradiance(const PTProbeCoeffs* sh, uint64_t probeCount, const PTProbeQuery* queries, uint32_t count, PTIrradiance* out,
                                      hipStream_t stream);
// ---- probe volumes (include/ptmi_plugin.h Part 16; pt_volume.hip) ----
// A depth bake of one chunk (entries * samples <= 2^21): the rays kernel writes 2 float4 per slot = entry * samples + j, the
// closest-hit query (pt_launch_query) writes 1 float4 per slot, the resolve turns them into one 512-byte record per probe.
hipError_t pt_launch_probe_depth_rays(const PTProbe* probes, uint32_t entries, uint32_t samples, uint32_t firstSample, float maxDistance, float4* rays,
                                      hipStream_t stream);
hipError_t pt_launch_probe_depth_resolve(const PTProbe* probes, uint32_t entries, uint32_t samples, uint32_t firstSample, float maxDistance,
                                         const float4* hits, PTProbeDepthMap* out, hipStream_t stream);
// the grid has passed ptvol::check_grid; depth may be null without PT_GRID_VISIBILITY
hipError_t pt_launch_probe_grid_irradiance(const PTProbeGrid& grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTReceiver* queries,
                                           uint32_t count, PTIrradiance* out, hipStream_t stream);
// ---- probe placement (include/ptmi_plugin.h Part 18; pt_placement.hip) ----
// One step of one chunk (entries * samples <= 2^20): the rays kernel writes 2 float4 per slot = entry * samples + j from the origin
// P + the offset as the rule reads it, the closest-hit query with surface records (pt_launch_query, mode 2) writes 1 and 3 float4
// per slot, the step kernel turns them into the probe's new 16 bytes (move) and state, and its statistics where stats != null.
hipError_t pt_launch_probe_place_rays(const PTProbe* probes, uint32_t entries, uint32_t samples, uint32_t firstSample, const PTProbePlaceParams& params,
                                      const PTProbePlacement* placement, float4* rays, hipStream_t stream);
hipError_t pt_launch_probe_place_step(const PTProbe* probes, uint32_t entries, uint32_t samples, uint32_t firstSample, const PTProbePlaceParams& params,
                                      const float4* hits, const float4* surfaces, bool move, PTProbePlacement* placement, PTProbePlaceStats* stats,
                                      hipStream_t stream);
// placement is not null; otherwise as pt_launch_probe_grid_irradiance
hipError_t pt_launch_probe_grid_irradiance_placed(const PTProbeGrid& grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTProbePlacement* placement,
                                                  const PTReceiver* queries, uint32_t count, PTIrradiance* out, hipStream_t stream);
// ---- reflection probes (include/ptmi_plugin.h Part 20; pt_reflection.hip) ----
// The list's texels [firstTexel, firstTexel + texels) -- texel g belongs to probe g / (res * res) --, texels * samples <= 2^30 slots:
// the rays kernel writes one PTRadianceRay per slot = (g - firstTexel) * samples + j; the fold turns texels * samples PTRadiance
// entries into `texels` base texels.
hipError_t pt_launch_refl_rays(const PTProbe* probes, uint64_t firstTexel, uint32_t texels, uint32_t res, uint32_t firstSample, uint32_t samples,
                               PTRadianceRay* rays, hipStream_t stream);
hipError_t pt_launch_refl_fold(const PTRadiance* radiance, uint32_t texels, uint32_t samples, PTReflectionTexel* out, hipStream_t stream);
// res and levels have passed ptrefl::check_layout; probes <= 65535 per launch
hipError_t pt_launch_refl_prefilter(const PTReflectionTexel* base, uint32_t probes, uint32_t res, uint32_t levels, PTReflectionTexel* out, hipStream_t stream);
// probes and boxes may be null (boxes only with probes)
hipError_t pt_launch_refl_lookup(const PTReflectionTexel* maps, uint64_t probeCount, uint32_t res, uint32_t levels, const PTProbe* probes,
                                 const PTReflectionBox* boxes, const PTReflectionQuery* queries, uint32_t count, PTReflectionTexel* out, hipStream_t stream);
// ---- shading from the bakes (include/ptmi_plugin.h Part 21; pt_shade_baked.hip) ----
// res is 16, 32 or 64
hipError_t pt_launch_shade_dfg(uint32_t res, PTShadeDFG* out, hipStream_t stream);
// rays, hits, surfaces: a closest-hit query's with surface records; probes and boxes may be null (boxes only with probes, probes
// only with probeCount == 0); every output may be null
hipError_t pt_launch_shade_surfaces(const DScene& S, const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces, uint32_t count, const PTProbe* probes,
                                    const PTReflectionBox* boxes, uint32_t probeCount, PTShadeMaterial* outMaterial, PTShadeTerms* outTerms,
                                    PTReceiver* outReceivers, PTReflectionQuery* outQueries, hipStream_t stream);
hipError_t pt_launch_shade_compose(const PTShadeTerms* terms, const PTIrradiance* irradiance, const PTReflectionTexel* reflection, uint32_t count,
                                   const PTShadeDFG* dfg, uint32_t dfgRes, float4* out, hipStream_t stream);
// the fused call: in.grid has passed ptvol::check_grid, in.res and in.levels ptrefl::check_layout; in.dPlacement picks the kernel
hipError_t pt_launch_shade_baked(const DScene& S, const PTShadeInputs& in, const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces, uint32_t count,
                                 float4* out, hipStream_t stream);
// pixels [first, first + count) of the frame P describes: the guides' ray at one sample per pixel, tmax PT_FAR_PLANE
hipError_t pt_launch_shade_frame_rays(const PTFrameParams& P, uint32_t first, uint32_t count, PTRay* rays, hipStream_t stream);
// ---- first hits shaded from baked lightmaps (include/ptmi_plugin.h Part 22; pt_shade_lightmap.hip) ----
// table: bindingCount (<= PT_LIGHTMAP_MAX_BINDINGS) records on the device that have passed ptlm::check_bindings, or null with 0;
// outBinding may be null
hipError_t pt_launch_lightmap_lookup(const DScene& S, const PTLightmapBinding* table, uint32_t bindingCount, const PTRay* rays, const PTRayHit* hits,
                                     const PTRaySurface* surfaces, uint32_t count, PTIrradiance* out, uint32_t* outBinding, hipStream_t stream);
// pt_launch_shade_baked with the lightmap lookup in front of the volume's
hipError_t pt_launch_shade_lightmapped(const DScene& S, const PTShadeInputs& in, const PTLightmapBinding* table, uint32_t bindingCount, const PTRay* rays,
                                       const PTRayHit* hits, const PTRaySurface* surfaces, uint32_t count, float4* out, hipStream_t stream);
#ifndef PT_WF_FUSED_GROUPS
#define PT_WF_FUSED_GROUPS 2u   // schedule 4: groups of 64 path contexts a persistent wave owns (power of two <= 4: numSlots is a multiple of 256).
                                // Sponza-class 1080p / 8 spp, one pass in flight: 1: 29.9 ms, 2: 25.2, 4: 27.9, 8: 31.4
#endif
#ifndef PT_WF_SUSPEND
#define PT_WF_SUSPEND 16u       // refill trace kernel: a wave whose range is exhausted stops when this many rays or fewer are left, and leaves them
                                // as records for the tail launch (pt_wavefront.hip); 0 = off.  Also the record slots per trace wave (pt_wf_arena_bytes)
#endif
// ---- mid-pass slot repack (schedule 1 over PTTileMap; pt_repack.hip, pt_wavefront.hip's launch sequence) ----
// After the shade launch of a CANDIDATE iteration the live slots of the set are counted, and when few enough are left
// (0 < L <= numSlots / 2 and L <= fill x E, E = end of the highest live block) their state is moved to slots [0, L): the
// shade waves that follow are full again and the trace ranges dense.  Candidates: iteration first = FIRST_SPP x spp + FIRST_ADD,
// then every STRIDE-th, at most MAX_CANDIDATES of them, none with fewer than MIN_LEFT iterations to go.  Measured on the
// Sponza-class pass (profiles/slot_repack_ab.md): every slot is alive through iteration spp - 1, half of them at iteration 2 spp.
// PT_WF_REPACK_MIN_SLOTS: sets of fewer slots keep their sequence; not defined = the pt_wf_wide_ranges boundary.
#ifndef PT_WF_REPACK_MIN_ITERATIONS
#define PT_WF_REPACK_MIN_ITERATIONS 12u
#endif
// Sweep on the Sponza-class benchmark, Mrays/s against the parent's 5,650 (profiles/slot_repack_ab.md): first spp + 2, stride 2, no
// limit: 5,787; stride 1: 5,647 (a candidate is four launches whether it repacks or not); first 2 spp: 5,820; first 2 spp with
// at most 7 / 6 / 5 candidates: 5,869 / 5,876 / 5,896 -- a repack of fewer than ~50 k slots costs more than the waves it saves.
#ifndef PT_WF_REPACK_FIRST_SPP
#define PT_WF_REPACK_FIRST_SPP 2u
#endif
#ifndef PT_WF_REPACK_FIRST_ADD
#define PT_WF_REPACK_FIRST_ADD 0u
#endif
#ifndef PT_WF_REPACK_STRIDE
#define PT_WF_REPACK_STRIDE 2u
#endif
#ifndef PT_WF_REPACK_MAX_CANDIDATES
#define PT_WF_REPACK_MAX_CANDIDATES 5u
#endif
#ifndef PT_WF_REPACK_MIN_LEFT
#define PT_WF_REPACK_MIN_LEFT 4u
#endif
#ifndef PT_WF_REPACK_FILL_NUM
#define PT_WF_REPACK_FILL_NUM 3u
#endif
#ifndef PT_WF_REPACK_FILL_DEN
#define PT_WF_REPACK_FILL_DEN 4u
#endif
inline bool pt_wf_repack_slots(uint32_t numSlots, uint32_t residentWaves)
{
#ifdef PT_WF_REPACK_MIN_SLOTS
    return numSlots >= PT_WF_REPACK_MIN_SLOTS;
#else
    return pt_wf_wide_ranges(numSlots, residentWaves);
#endif
}
// is the state after the shade launch of iteration `it` (of `iterations`) a candidate?
inline bool pt_wf_repack_candidate(uint32_t it, uint32_t iterations, uint32_t spp)
{
    const uint32_t first = PT_WF_REPACK_FIRST_SPP * spp + PT_WF_REPACK_FIRST_ADD;
    if (it < first || it + PT_WF_REPACK_MIN_LEFT >= iterations) return false;            // iterations after it: iterations - 1 - it
    return (it - first) % PT_WF_REPACK_STRIDE == 0u && (it - first) / PT_WF_REPACK_STRIDE < PT_WF_REPACK_MAX_CANDIDATES;
}
// pt_repack.hip: the four launches of a candidate (count, scan and decide, move out, move back) on set B; the shade launch and the
// cleanup launch of a sequence that repacks (the pixel of a slot from B.pixelOf, finished sums into B.pixsum).  stats may be null.
hipError_t pt_launch_repack(const PTWfBuffers& B, uint32_t fillNum, uint32_t fillDen, bool firstOfSequence, unsigned long long* stats, hipStream_t stream);
hipError_t pt_launch_repack_shade(const DScene& S, const PTFrameParams& P, const PTTileMap& tm, const PTWfBuffers& B, bool fullStats, uint32_t iteration,
                                  hipStream_t stream);
hipError_t pt_launch_repack_cleanup(const DScene& S, const PTFrameParams& P, const PTTileMap& tm, const PTWfBuffers& B, bool fullStats, uint32_t blocks,
                                    hipStream_t stream);
#ifndef PT_WF_SETS
#define PT_WF_SETS 12            // path-state sets = passes that can be in flight at once, each on its own stream (3 -> 6 sets with 8 hardware queues: +12 %;
                                 // 6 -> 12 sets with 16 queues: +2 % at 1080p, +7 % at 960x540, -14 % time for a 1/8 share of a 1080p frame; 16: no better, 24: worse)
#endif

// ---- ONE wavefront launch sequence: what to render (the slot mapping), from and into what, on which stream, by which schedule ----
enum PTWfMapKind : uint32_t { PT_WF_MAP_TILES, PT_WF_MAP_LIST, PT_WF_MAP_RAYS, PT_WF_MAP_GATHER, PT_WF_MAP_PROBE };
struct PTWfLaunch {
    const DScene* scene;
    const PTFrameParams* params;
    PTBatch batch;
    PTWfMapKind mapKind;                    // which member of the union below is set
    union {
        PTTileMap tiles;                    // a pass (or a sub-frame of one) over the context's 16x16 blocks
        PTListMap list;                     // a pass over a block list
        PTRayMap rays;                      // a radiance query
        PTGatherMap gather;                 // an irradiance gather
        PTProbeMap probe;                   // SH light probes
    };
    const float4* accumulated;
    void* output;                           // the frame (float4 per pixel); PT_WF_MAP_RAYS: the PTRadiance array; PT_WF_MAP_GATHER: the PTIrradiance array; PT_WF_MAP_PROBE: the PTProbeCoeffs array
    const PTWfBuffers* buffers;             // the state set the sequence runs on
    unsigned long long* counters;           // the context's 16 counters (PTStats order)
    bool fullStats;
    hipStream_t stream;
    hipEvent_t orderAfter;                  // may be null: the resolve -- and only it -- waits for this event
    bool zeroOutputFirst;                   // PT_WF_MAP_TILES only: clear the frame before the resolve (pixels of other ranks read as zeros)
    int schedule;                           // 1 ... 4 (PTSetSchedule)
    uint32_t iterationsOverride;            // 0 = spp * (bounces + 2) + 4, capped by buffers->maxIterations
    unsigned long long* repackStats;        // may be null: the context's four repack counters (PTRepackStats order), added to on the device
};
// Enqueues the sequence on L.stream without host synchronisation; launchesOut (may be null): kernel launches enqueued.
// hipErrorNotSupported for schedule 4 over a list, rays, a gather or probes.  pt_wavefront.hip is compiled twice with different scheduler flags
// (csrc/Makefile); which compilation's kernels run is decided behind this one entry point.
hipError_t pt_launch_wavefront(const PTWfLaunch& L, uint32_t* launchesOut);
