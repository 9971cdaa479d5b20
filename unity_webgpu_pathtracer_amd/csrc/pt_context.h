// pt_context.h — internal to the pt_api_*.hip files (the PT* entry points of include/ptmi_plugin.h, one file per part of that
// header): the context and the group, the types that own their HIP resources, and the error / import helpers every part uses.
#pragma once
#include "pt_launch.h"
#include "pt_tlas.h"
#include "pt_refit.h"
#include "pt_quality.h"
#include "pt_skin.h"
#include "pt_morph.h"
#include "pt_lightmap.h"
#include "pt_lmfilter.h"
#include "pt_adaptive_gather.h"
#include "pt_unwrap.h"
#include "pt_direct.h"
#include "pt_light_grid.h"
#include "bvh_refit.h"
#include "bvh_builder_gpu.h"

#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

extern thread_local std::string g_lastError;        // one for the whole library (pt_api_context.hip)

inline int fail(int code, const std::string& msg)
{
    g_lastError = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

// roctx ranges around every pass / scene upload (rocprofv3 --marker-trace shows them; the reference wraps its dispatch in
// _cmd.BeginSample / EndSample("Path Tracer"), PathTracer.cs:226,252)
struct RoctxRange {
    explicit RoctxRange(const char* name);
    ~RoctxRange();
};

// ---- owners: whatever a context or a group holds is released by its destructor; movable, not copyable ----
template <class T, hipError_t (*Destroy)(T)>
struct Owned {
    T h = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept { std::swap(h, o.h); return *this; }      // o's destructor releases what we held
    ~Owned() { if (h) Destroy(h); }
    operator T() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
// created on first use
inline int create(Stream& s) { if (!s.h) HIP_TRY(hipStreamCreateWithFlags(&s.h, hipStreamNonBlocking)); return PT_OK; }
inline int create(Event& e, unsigned flags = hipEventDisableTiming) { if (!e.h) HIP_TRY(hipEventCreateWithFlags(&e.h, flags)); return PT_OK; }
// The stream of state set `index` (PTContext::sets), created on first use (pt_api_context.hip).  The runtime multiplexes the
// streams of a process onto GPU_MAX_HW_QUEUES hardware queues, and streams that share one serialise.  Below a limit of 16 a set
// stream is made with hipExtStreamCreateWithCUMask and every CU enabled: a queue that carries a CU mask is never pooled, so each
// set has a hardware queue of its own at normal priority -- and, the call taking no flags, a stream that synchronises with the
// null stream.  With 16 or more, or where the runtime refuses, it is create().  *ownQueue: made here with a queue of its own.
int create_set_stream(uint32_t index, Stream& s, bool* ownQueue = nullptr);

// One device allocation (Pinned: one page-locked host allocation).
template <bool Pinned>
struct Buffer {
    void* ptr = nullptr;
    size_t bytes = 0;           // allocation capacity (a smaller request re-uses it)
    size_t used = 0;            // bytes of the last request
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : ptr(o.ptr), bytes(o.bytes), used(o.used) { o.ptr = nullptr; o.bytes = o.used = 0; }
    Buffer& operator=(Buffer&& o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); std::swap(used, o.used); return *this; }
    ~Buffer() { release(); }
    void release()
    {
        if (ptr) (void)(Pinned ? hipHostFree(ptr) : hipFree(ptr));
        ptr = nullptr;
        bytes = used = 0;
    }
    // Keeps an allocation that is large enough.  Otherwise frees it and allocates `need` bytes; work that may still use the old
    // memory must have finished by then: pass the stream it was enqueued on (drained here, only when there is something to free), or
    // say at the call which synchronisation covers it.
    int reserve(size_t need, hipStream_t drain = nullptr)
    {
        used = need;
        if (need <= bytes) return PT_OK;
        if (ptr && drain) HIP_TRY(hipStreamSynchronize(drain));
        release();
        HIP_TRY(Pinned ? hipHostMalloc(&ptr, need, hipHostMallocDefault) : hipMalloc(&ptr, need));
        bytes = used = need;
        return PT_OK;
    }
};
using DeviceBuffer = Buffer<false>;
using PinnedBuffer = Buffer<true>;

// N per-pixel device buffers that are resized together: afterwards all N hold w x h elements, or the set is empty (w = h = 0).
template <int N>
struct FrameSet {
    DeviceBuffer buf[N];
    uint32_t w = 0, h = 0;
    float4* f4(int k) const { return (float4*)buf[k].ptr; }
    void clear()
    {
        for (DeviceBuffer& b : buf) b.release();
        w = h = 0;
    }
    // elemBytes: bytes per pixel of each buffer; drain: as for Buffer::reserve
    int resize(uint32_t W, uint32_t H, std::initializer_list<size_t> elemBytes, hipStream_t drain)
    {
        if (w == W && h == H) return PT_OK;
        if (w && drain) HIP_TRY(hipStreamSynchronize(drain));
        clear();
        int k = 0;
        for (size_t e : elemBytes)
            if (int rc = buf[k++].reserve((size_t)W * H * e)) { clear(); return rc; }
        w = W; h = H;
        return PT_OK;
    }
};

// A small table the host rewrites per call and kernels read in stream order: a ring of pinned staging buffers and one device
// copy.  send() only waits for the upload made kRing sends ago to have left its staging buffer (an event recorded right behind
// that copy), never for kernels -- on a stream that sits behind the resolves of passes in flight a single buffer would make
// the host wait for the previous pass.
struct UploadTable {
    static constexpr int kRing = 4;
    DeviceBuffer dev;
    PinnedBuffer host[kRing];
    Event copied[kRing];
    bool recorded[kRing] = {};
    int next = 0;
    int send(const void* src, size_t bytes, hipStream_t stream)
    {
        const int k = next;
        next = (next + 1) % kRing;
        if (int rc = create(copied[k])) return rc;
        if (recorded[k]) HIP_TRY(hipEventSynchronize(copied[k]));
        if (int rc = host[k].reserve(bytes)) return rc;
        if (int rc = dev.reserve(bytes, stream)) return rc;         // growing: kernels that read the old copy ran on this stream
        memcpy(host[k].ptr, src, bytes);
        HIP_TRY(hipMemcpyAsync(dev.ptr, host[k].ptr, bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(copied[k], stream));
        recorded[k] = true;
        return PT_OK;
    }
};

struct EventPair { Event start, stop; uint32_t launches = 0; };

// what a host variant stages a caller's list and its results in on the device (host_round_trip), grown on demand; one per feature
struct HostStaging { DeviceBuffer in, out; };

struct PTContext {
    int device = 0;
    Stream stream;
    DeviceBuffer nodes, tris, attrs, materials, lights, lightConst, tex, tlas, tlasBfs, instances, instByLeaf, envTex, envCdf;
    DeviceBuffer batchScratch;                  // PTRenderPassBatchTo under the megakernel: the frame the odd passes of a batch write
    DeviceBuffer present;                       // PTPresentToHost staging frame
    DScene scene = {};
    bool hasScene = false;
    FrameSet<2> frames;
    int cur = 0;
    int rank = 0, world = 1;
    int statsLevel = 0;
    int schedule = -1;                          // -1 auto (default), 0 megakernel, 1 wavefront + refill trace, 2, 3: see PTSetSchedule
    DeviceBuffer dStats;                        // 16 counters, PTStats order, then the 4 of PTRepackStats
    bool profiling = false;
    std::vector<EventPair> pending;             // recorded, not yet read
    std::vector<EventPair> freeEvents;
    PTTimings timings = {};
    // wavefront schedules: PT_WF_SETS path-state sets, each with its own stream, so consecutive passes overlap
    struct WfSet {
        PTWfBuffers wf = {};
        DeviceBuffer arena;
        Stream stream;
        Event callEv, done;
        UploadTable blockTable;                 // PTRenderPassActive: the call's {block id, sample count} snapshot (pt_launch.h PTListMap)
    } sets[PT_WF_SETS];
    uint32_t nextSet = 0;
    uint32_t residentWaves = 0;                 // CUs x 4 SIMDs x 8 waves (device property, read once)
    uint32_t subFrames = 1;                     // launch chains a pass is cut into (PTSetSubFrames)
    uint32_t numSets = 0;                       // passes in flight = state sets in use (PTSetPassesInFlight); carved on first use
    bool ownQueues = false;                     // PTCreate got set 0's stream with a hardware queue of its own (create_set_stream): the default is every set
    uint32_t wfIterations = 0;                  // 0 = automatic
    // ray queries (PTTraceRays): grid caps per query kernel (read once), the CWBVH stack slab sized for the largest, host staging
    struct Query {
        uint32_t caps[PT_QUERY_KERNELS] = {};
        uint32_t directCaps[2] = {};            // pt_direct_light, pt_direct_light_tlas (Part 24): they share the slab
        uint32_t culledCaps[2] = {};            // pt_direct_light_grid, pt_direct_light_grid_tlas (Part 25), on first use: likewise
        uint32_t capMax = 0;
        DeviceBuffer slab;
        DeviceBuffer rays, hits, surface;       // PTTraceRaysHost staging, grown on demand
    } query;
    // guides (PTRenderGuides): allocated on first use, regrown on a size change
    struct Guide {
        uint32_t caps[2] = {};
        DeviceBuffer slab;
        FrameSet<2> frames;                     // albedo + coverage, normal + depth
    } guide;
    // denoising (PTDenoise): likewise
    struct Denoise {
        FrameSet<3> state;                      // filter state ping-pong (e.rgb, v) x 2, then the float2 depth gradient
        DeviceBuffer host;                      // PTDenoiseToHost staging frame
    } denoise;
    // moments across passes (PTAccumulateMoments / PTMeasureNoise / PTDenoiseMoments): likewise
    struct Moments {
        FrameSet<2> planes;                     // Srr Sgg Sbb Sll | Srg Srb Sgb 0
        uint32_t observations = 0;
        uint64_t samples = 0;
        // the frame last accumulated: one of the context's own frames (by index: they may be re-created) or a caller's pointer
        int lastOwn = -1;
        const void* lastPtr = nullptr;
        DeviceBuffer stats, blockSums, tiles;   // PTMeasureNoise: PT_NOISE_WORDS words, one float per 16x16 block each
    } moments;
    // adaptive sampling (include/ptmi_plugin.h Part 7): per-block sample counts and the active list, on the host; empty until PTAdaptiveBegin
    struct Adaptive {
        bool live = false;
        uint32_t w = 0, h = 0, blocksX = 0, blocksY = 0;
        uint32_t coverW = 0, coverH = 0;        // dispatch coverage of PTAdaptiveBegin's params (pt_make_tile_map)
        std::vector<uint32_t> samples;          // n_b, one per block of the frame
        bool allActive = true;                  // PTSetActiveBlocks(NULL, 0): every block (the state after PTAdaptiveBegin)
        std::vector<uint32_t> active;           // as given to PTSetActiveBlocks (ascending), when !allActive
        // moments per block (PTAccumulateMomentsActive); tracked only when PTAdaptiveBegin found moments that match
        bool moments = false;
        std::vector<uint32_t> obs;              // k_b
        std::vector<uint64_t> wsum;             // W_b
        // the adaptive call last enqueued: what PTAccumulateMomentsActive describes
        std::vector<uint2> lastTable;           // {block id, n_b at the start of the call}
        uint32_t lastM = 0;                     // samples the call added per block; 0 = none pending
        UploadTable momentsTable, invDof;       // on the context stream
    } adaptive;
    HostStaging radiance;                       // radiance queries (PTTraceRadianceHost)
    HostStaging gather;                         // irradiance gathers (PTGatherIrradianceHost)
    // SH light probes (PTProbeSH): the delta lights' rays, Li and any-hit records of a call, 64 bytes per (probe, light) pair,
    // written and read in stream order behind the context stream; PTProbeSHHost's staging
    struct Probe {
        DeviceBuffer deltaRays, deltaLi, deltaHits;
        HostStaging host;
    } probe;
    // probe volumes (PTProbeDepth): the rays and hit records of one chunk, 48 bytes per sample, used in stream order on the
    // context stream; PTProbeDepthHost's staging
    struct Volume {
        DeviceBuffer rays, hits;
        HostStaging host;
    } volume;
    // probe placement (PTProbePlace): the rays, hit and surface records of one chunk, 96 bytes per sample, used in stream order on
    // the context stream; PTProbePlaceHost's staging (its statistics come back through hostStats)
    struct Placement {
        DeviceBuffer rays, hits, surfaces;
        HostStaging host;
        DeviceBuffer hostStats;                 // regrows without a drain, as HostStaging does: every use of it ends in the synchronise
                                                // that closes the PTProbePlaceHost call that made it (host_round_trip)
    } placement;
    // reflection probes (PTReflectionCapture): the rays and the radiance of one slab of at most 2^22 slots, 48 bytes per slot, used
    // in stream order behind the context stream, kept across PTSetScene; PTReflectionCaptureHost's staging
    struct Reflection {
        DeviceBuffer rays, radiance;
        HostStaging host;
    } reflection;
    // shading from the bakes (PTShadeBakedFrame): the rays, hit and surface records of a frame, 96 bytes per pixel, used in stream
    // order on the context stream, kept across PTSetScene
    struct Shade {
        DeviceBuffer rays, hits, surfaces;
    } shade;
    // bound lightmaps (PTBindLightmaps): the table's device copy, rewritten in stream order on the context stream; count == 0:
    // nothing bound (PTSetScene unbinds: the spans name a scene)
    struct BoundLightmaps {
        UploadTable table;                      // PT_LIGHTMAP_MAX_BINDINGS records, whatever the count
        uint32_t count = 0;
        const PTLightmapBinding* device() const { return count ? (const PTLightmapBinding*)table.dev.ptr : nullptr; }
    } lightmaps;
    // lightmap charts (PTRasterizeChart / PTResolveLightmap): grown on demand, kept across PTSetScene
    struct Lightmap {
        DeviceBuffer owner;                     // 4 B per texel: the owner map
        DeviceBuffer blockBase;                 // 4 B per 256-texel block, then the 8-byte total
        DeviceBuffer prims;                     // 4 B per triangle twice: the record of every primitive, the list of large records
        DeviceBuffer image;                     // 16 B per texel: the resolve's second image
        PinnedBuffer count;                     // the total, read back
    } lightmap;
    // lightmap UVs (PTUnwrapCharts): kUnwrapBytesPerTriangle per triangle and the sort's temporary storage, grown on demand,
    // kept across PTSetScene
    struct Unwrap {
        DeviceBuffer work;
        PinnedBuffer small;                     // the counters and sweep flags, read back
    } unwrap;
    // the lightmap denoiser (PTDenoiseLightmap): 64 B per texel, grown on demand, kept across PTSetScene
    struct LightmapFilter {
        DeviceBuffer state[2];                  // 16 B per texel each: (e, v), the levels go from one to the other
        DeviceBuffer guideP, guideN;            // 16 B per texel each: (P, h2) and (N, flags)
    } lmfilter;
    // adaptive gathers (PTGatherIrradianceAdaptive and its steps): 56 B per entry and 16 B per 256 entries, grown on demand, kept
    // across PTSetScene
    struct AdaptiveGather {
        DeviceBuffer active[2];                 // 4 B per entry each: the active list of a round and of the next
        DeviceBuffer recv;                      // 32 B per entry: the active entries' receivers, compacted
        DeviceBuffer result;                    // 16 B per entry: what a round's gather wrote
        DeviceBuffer blockCounts;               // 16 B per 256-entry block, then the four 8-byte totals
        PinnedBuffer totals;                    // the totals, read back
        HostStaging host;                       // PTGatherIrradianceAdaptiveHost's staging
        DeviceBuffer hostCounts;                // ... and its counts: regrows without a drain, as HostStaging does
    } adaptiveGather;
    // scene updates (PTUpdateInstances / Lights / Materials): two generations of what an update rewrites, allocated on the first
    // update of each kind and discarded by PTSetScene.  cur = -1 while PTSetScene's own buffers are current.
    struct UpdGroup {
        DeviceBuffer gen[2];
        int cur = -1;
        Event freeEv[2];                                // recorded on the context stream when the generation stops being current
        bool freeRecorded[2] = {false, false};
        PinnedBuffer staging[2];                        // pinned host copies of the host variants' arrays
        Event stagedEv[2];
        bool stagedRecorded[2] = {false, false};
    };
    // geometry updates (PTUpdateGeometry): what the first one reads back and every later one reuses -- a refit never changes the
    // topology; a rebuild (PTRebuildGeometry) replaces the BLAS's plan with the new tree's
    struct GeomPlan {
        int32_t key[3] = {0, 0, 0};                     // bvhOffset, triOffset, triAttributeOffset
        uint32_t triCount = 0;
        uint32_t nodeCapacity = 0;                      // the BLAS's node span in PTSetScene's buffer
        DeviceBuffer order;                             // ptbvh::RefitPlan::order on the device
        std::vector<uint32_t> levelStart;
        // PTSetSkin: the BLAS's skin on the device, 40 bytes per vertex (+ 128 per triangle with rest attributes); jointCount == 0: none
        struct Skin {
            uint32_t jointCount = 0;
            DeviceBuffer rest, joints, weights, restAttrs;
        } skin;
        // PTSetMorph: the BLAS's morph on the device, its own rest pose and each stream in morph_rule.h's layout; targetCount == 0: none
        struct Morph {
            struct Stream {
                DeviceBuffer count, sliceBase, entries;
                PTMorphStream args() const { return {(const uint32_t*)count.ptr, (const uint32_t*)sliceBase.ptr, (const float4*)entries.ptr}; }
            };
            uint32_t targetCount = 0;
            DeviceBuffer rest, restAttrs;
            Stream position, normal, tangent;
        } morph;
    };
    struct Geometry {
        std::vector<PTFloat4> hostNodes;                // host copy of the node buffer (rows n1 and imask are what is read)
        std::vector<uint32_t> hostTriW;                 // the .w word of every triangle row (primIdx in every third)
        std::vector<int32_t> blasKeys;                  // HAS_TLAS: the three offsets of every instance (PTSetScene's records)
        std::vector<GeomPlan> plans;                    // one per BLAS updated so far
        DeviceBuffer nodeBox;                           // 24 B per node of the scene
        DeviceBuffer verts;                             // the host variant's vertices on the device, or the skin or morph kernel's
        DeviceBuffer buildWork;                         // the builder's work arrays, sized for the largest BLAS rebuilt so far
        DeviceBuffer qualityWork;                       // PTMeasureGeometry: results and per-workgroup partial sums
        UploadTable palette;                            // PTSkinGeometry: the host palette, on the update stream
        UploadTable morphWeights;                       // PTMorphGeometry: the host weights likewise
        DeviceBuffer skinWork;                          // the skinned vertices' box and its per-workgroup partials
        PinnedBuffer skinBounds;                        // ... read back (24 bytes)
    };
    struct Update {
        UpdGroup inst, lights, mats, geom, attrs;
        Geometry geometry;
        Stream stream;
        Event done;                                     // the last update's completion
        Event input;                                    // PTUpdateInstancesDevice: the context stream up to the call
        bool pending = false;                           // an update since PTSetScene: every pass waits for `done` first
        DeviceBuffer tlasWork;
        PTTlasWork tlasW = {};
        uint32_t instanceCount = 0, sceneLightCount = 0, origTlasNodes = 0;
        std::vector<uint32_t> validTextures;            // texture indices PTSetScene validated (sorted)
        std::vector<uint32_t> lightTypes;               // the current lights' types (PTSetScene, PTUpdateLights): Part 24 counts pairs on the host
        uint64_t lightGeneration = 0;                   // PTSetScene and PTUpdateLights each start one (Part 25: what a light grid was built for)
    } update;
    // the light grid of the culled direct-light calls (PTBuildLightGrid, Part 25): grown on demand, kept across PTSetScene, written
    // and read in stream order on the context stream; current only while generation == update.lightGeneration
    struct LightGrid {
        DeviceBuffer offsets, indices, rectBefore;      // light_grid_rule.h's storage
        DeviceBuffer blockCounts;                       // 4 B per block of 1024 cells, then the 4-byte total
        PinnedBuffer total;                             // the total, read back
        ptlgrid::Grid g = {};
        bool built = false;
        uint64_t generation = 0;
        uint32_t cells = 0, lightCount = 0, entries = 0;
        int64_t longest = -1;                           // PTLightGridInfo computes it on first use (-1: not yet)
    } lightGrid;
};

struct PTGroup {
    struct Dev {
        PTContext* ctx = nullptr;
        DeviceBuffer packed;            // on device i: its owned tiles, dense
        DeviceBuffer staged;            // on the root device: the same, after the peer copy (unused for the root: it unpacks `packed`)
        Event arrived;                  // recorded on ctx->stream after the peer copy
        Event unpacked;                 // recorded on the root's stream after the tiles were scattered into the assembled frame
        bool unpackedValid = false;
        float4* tiles() const { return (float4*)(staged.ptr ? staged.ptr : packed.ptr); }     // what the root unpacks
    };
    std::vector<Dev> dev;               // dev[0] is the root
    FrameSet<1> assembled;
};

// "Versioning" (include/ptmi_plugin.h): copy min(structSize, sizeof) bytes of the host's struct into a zeroed one of ours
template <class T>
int import_struct(const T* in, T& out, size_t minSize, const char* typeName, const char* nullMsg)
{
    if (!in) return fail(PT_ERR_INVALID_ARG, nullMsg);
    if (in->structSize < minSize || in->structSize > 4096u)
        return fail(PT_ERR_INVALID_ARG, std::string(typeName) + ".structSize is not set (must be sizeof(" + typeName + ") of the host's header)");
    memset(&out, 0, sizeof(out));
    memcpy(&out, in, in->structSize < sizeof(out) ? in->structSize : sizeof(out));
    out.structSize = (uint32_t)sizeof(out);
    return PT_OK;
}

inline int validate_params(const PTFrameParams& p)
{
    if (p.OutputWidth == 0 || p.OutputHeight == 0) return fail(PT_ERR_INVALID_ARG, "OutputWidth/OutputHeight == 0");
    if ((uint64_t)p.OutputWidth * p.OutputHeight > 0x7FFFFFFFull / 4) return fail(PT_ERR_INVALID_ARG, "frame too large");
    return PT_OK;
}

// what opens every entry point that takes frame parameters
inline int import_frame_params(const PTFrameParams* in, PTFrameParams& p)
{
    const int rc = import_struct(in, p, PT_FRAME_PARAMS_MIN_SIZE, "PTFrameParams", "params == NULL");
    return rc ? rc : validate_params(p);
}

// a device pointer the kernels read or write in units of `a` bytes; NULL counts as aligned (the NULL checks are the callers')
inline bool misaligned(const void* p, uintptr_t a = 16) { return ((uintptr_t)p & (a - 1u)) != 0u; }

// auto (-1): scenes whose whole BVH is a handful of nodes (Cornell box: 1 node) have no traversal to speak of; the
// wavefront's per-iteration path-state traffic then costs more than it buys (measured 8.7 vs 10.5 Grays/s)
inline int effective_schedule(const PTContext* c)
{
    if (c->schedule >= 0) return c->schedule;
    return (c->nodes.used <= 80u * 16u && !c->scene.hasTlas) ? 0 : 1;
}

// What the entry points that make `samples` samples per list entry check after the context (gathers, SH probes): params, the
// sample count, the bounce limit.  p1: params with one sample per slot
inline int import_sampled_params(const PTFrameParams* hostParams, uint32_t samples, const char* who, PTFrameParams& p1)
{
    if (!hostParams) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": params == NULL");
    if (int rc = import_frame_params(hostParams, p1)) return rc;
    p1.SamplesPerPass = 1;
    if (samples == 0u || samples > PT_GATHER_MAX_SAMPLES)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": samples = " + std::to_string(samples) + " (1 ... " + std::to_string(PT_GATHER_MAX_SAMPLES) + ")");
    if (p1.MaxRayBounces > 8191u) return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": MaxRayBounces > 8191 does not fit the packed path state");
    return PT_OK;
}

// a list call needs a scene and a schedule with launch sequences; noun: what the list holds ("ray", "receiver", "probe")
inline int check_list_schedule(const PTContext* c, const char* who, const char* noun)
{
    if (!c->hasScene) return fail(PT_ERR_NO_SCENE, "PTSetScene has not been called");
    const int schedule = effective_schedule(c);
    if (schedule < 1 || schedule > 3)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": schedule " + std::to_string(schedule) + " has no pass over a " + noun + " list (schedules 1, 2 and 3 do: PTSetSchedule)");
    return PT_OK;
}

// fn(first, n) for every launch of at most perLaunch (<= 2^32 - 1) entries that `count` entries are cut into, in order; stops at
// the first rc != PT_OK
template <class Fn>
int for_each_launch(uint64_t count, uint64_t perLaunch, Fn&& fn)
{
    for (uint64_t first = 0; first < count; first += perLaunch)
        if (int rc = fn(first, (uint32_t)(count - first < perLaunch ? count - first : perLaunch))) return rc;
    return PT_OK;
}

// A host variant's round trip: `count` entries of the caller's `in` to the device, body(dIn, dOut) -- the device variant's, which
// enqueues on the context stream or joins it --, `count` results back into `out`, synchronised.  count == 0: the body's checks only.
// The staging buffers regrow without a drain: every use of them ends in this call's final synchronise.
template <class In, class Out, class Body>
int host_round_trip(PTContext* c, HostStaging& s, const In* in, uint64_t count, Out* out, Body&& body)
{
    int rc;
    if (count) {
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = s.in.reserve(count * sizeof(In))) || (rc = s.out.reserve(count * sizeof(Out)))) return rc;
        HIP_TRY(hipMemcpyAsync(s.in.ptr, in, count * sizeof(In), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = body((const In*)s.in.ptr, (Out*)s.out.ptr)) || count == 0) return rc;
    HIP_TRY(hipMemcpyAsync(out, s.out.ptr, count * sizeof(Out), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

// the material slots that name a texture: baseColor, metallicRoughness, emission, occlusion (normal map is unused)
constexpr int kTextureSlots[4] = {22, 23, 25, 26};

// pt_api_denoise.hip: PTDenoise's body; variance != nullptr is PTDenoiseMoments (dSrc then is never NULL)
int denoise_frame(PTContext* c, const PTDenoiseParams* params, const void* dSrc, void* dDst, const PTDenoiseVariance* variance);
// pt_api_update.hip: the three steps of every update of a group (begin: the target generation, free to write on the update
// stream; stage: a host array through the target's pinned staging; end: the target becomes current)
int begin_update(PTContext* c, PTContext::UpdGroup& g, size_t genBytes, size_t stagingBytes, int& target);
int stage_host(PTContext* c, PTContext::UpdGroup& g, int target, const void* src, size_t bytes, void* dst);
int end_update(PTContext* c, PTContext::UpdGroup& g, int target);
// pt_api_geometry.hip: what the first geometry call of a scene reads back, once (synchronising), and the plan of the BLAS the three
// offsets name (made, and the BLAS walked, on its first use); triCount == 0: the BLAS's own count
int ensure_host_copy(PTContext* c);
int find_plan(PTContext* c, int32_t bvhOffset, int32_t triOffset, int32_t attrOffset, uint32_t triCount, PTContext::GeomPlan*& out);
// pt_api_gather.hip: PTGatherIrradiance's body, one launch sequence per chunk of floor(PT_RADIANCE_CHUNK / samples) whole entries
int gather_irradiance(PTContext* c, const PTFrameParams& p1, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                      PTIrradiance* dOut, const char* who);
// pt_api_radiance.hip: PTTraceRadiance's body, one launch sequence per chunk of PT_RADIANCE_CHUNK rays
int trace_radiance(PTContext* c, const PTFrameParams& p, const PTRadianceRay* dRays, uint64_t count, PTRadiance* dOut, const char* who);
// pt_api_shade.hip: what PTShadeBaked and PTShadeBakedFrame check of the struct before the context is used, and PTShadeBakedFrame's
// body -- the frame's rays, the closest-hit walk with surface records into the context's scratch, then shade(...) over them
int check_shade_inputs(const PTShadeInputs* in, const char* who);
// user: what the frame's entry point hands its own list call besides the inputs (Part 24: the direct parameters); may be null
using ShadeList = int (*)(PTContext* c, const PTShadeInputs& in, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count,
                          float4* dOut, const void* user);
int shade_frame(PTContext* c, const PTFrameParams* hostParams, const PTShadeInputs* inputs, float* dOut, PTRay* dOutRays, const char* who, ShadeList shade,
                const void* user = nullptr);
// pt_api_light_grid.hip: the context's grid for a culled call, or the refusal of an absent or stale one
int current_light_grid(PTContext* c, const char* who, PTLightGridDevice& out);
int query_prepare(PTContext* c);                                                // pt_api_query.hip: the grid caps and the stack slab of the query kernels, on first use
int set_scene(PTContext* c, const PTSceneDesc* hostScene, bool validate);      // pt_api_context.hip; PTGroupSetScene validates once
int drain_events(PTContext* c);                                                 // pt_api_context.hip
int ensure_frames(PTContext* c, uint32_t w, uint32_t h);                        // pt_api_render.hip
int import_batch(const PTFrameParams* hostParams, int count, PTFrameParams& first, PTBatch& batch);      // pt_api_render.hip
int take_event_pair(PTContext* c, EventPair& ep);                               // pt_api_render.hip: a start / stop pair for a profiled pass
int ensure_wavefront(PTContext* c, PTContext::WfSet& set, uint32_t numSlots, uint32_t maxIterations);      // pt_api_render.hip
// ---- enqueueing a wavefront launch sequence on the next state set (pt_api_render.hip): passes, adaptive passes, list calls ----
// the limits the packed state word sets on SamplesPerPass / MaxRayBounces; maxIterations: the iteration bound a state set is carved for
int wavefront_limits(const PTFrameParams& p, uint32_t& maxIterations);
PTContext::WfSet& next_wavefront_set(PTContext* c, uint32_t* index = nullptr);      // state sets take turns; index (may be null): which one
// The caller fills params, batch, the slot mapping, accumulated, output, orderAfter and zeroOutputFirst of L; scene, state set,
// counters, stream, schedule and iterations come from c and set.  On set.stream, in order: wait for a pending scene update, record
// profStart (null: none), the launch sequence, record profStop (null: none), record set.done.  launches += the sequence's kernel launches.
int enqueue_wavefront(PTContext* c, PTContext::WfSet& set, PTWfLaunch& L, hipEvent_t profStart, hipEvent_t profStop, uint32_t& launches);
// A list call (radiance queries, irradiance gathers, SH probes): one launch sequence per chunk of perChunk whole entries of a
// list of `count`, each entry slotsPerEntry slots (perChunk * slotsPerEntry <= PT_RADIANCE_CHUNK), under the ROCTX range
// rangeName.  Each sequence runs on the next state set and its stream, behind what the context stream holds at that moment; the
// context stream joins every set used, once, after the last chunk (pt_api_render.hip has the reasons).  The caller has checked
// the scene and the schedule (check_list_schedule); p is checked against wavefront_limits here, then count == 0 returns PT_OK.
// fill(first, n, L): the slot mapping and the output of chunk [first, first + n) into L, whose params are p already.
using ListChunkFill = void (*)(void* fill, uint64_t first, uint32_t n, PTWfLaunch& L);
int enqueue_list_chunks(PTContext* c, const PTFrameParams& p, uint64_t count, uint64_t perChunk, uint32_t slotsPerEntry, const char* rangeName,
                        ListChunkFill fill, void* fillArg);
template <class Fill>
int enqueue_list_chunks(PTContext* c, const PTFrameParams& p, uint64_t count, uint64_t perChunk, uint32_t slotsPerEntry, const char* rangeName, Fill&& fill)
{
    return enqueue_list_chunks(c, p, count, perChunk, slotsPerEntry, rangeName,
                               [](void* f, uint64_t first, uint32_t n, PTWfLaunch& L) { (*(std::remove_reference_t<Fill>*)f)(first, n, L); }, (void*)&fill);
}
// pt_api_adaptive.hip: the per-block 1 / ((k_b - 1) W_b) table on the device while adaptive state of the moments' size tracks
// moments, else NULL (rc != PT_OK on a failed upload); minObs / minSamples: the minimum over the blocks this context owns
// table == NULL: only the minima, nothing is uploaded
int adaptive_inv_dof(PTContext* c, const float** table, uint32_t* minObs, uint64_t* minSamples);
