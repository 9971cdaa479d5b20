// pt_api_context.hip — context, scene, statistics, timings and settings (include/ptmi_plugin.h Part 2).
// The pt_api_*.hip files replace what the reference does through Unity's ComputeShader API: buffer uploads
// (BVHScene.cs:640-667 ComputeBuffer.SetData), per-frame uniforms + DispatchCompute
// (PathTracer.cs:226-252) and the ping-pong frame bookkeeping (PathTracer.cs:246-247, 268-272).
// There is NO CPU fallback: without a HIP device PTCreate fails with PT_ERR_NO_DEVICE.
#include "pt_context.h"
#include "pt_env_cdf.h"

#include <dlfcn.h>

#include <cstdlib>
#include <algorithm>
#include <array>

thread_local std::string g_lastError;

namespace {

// Consecutive passes run on up to PT_WF_SETS streams so that one pass's launch tails are filled by its neighbours' kernels.
// The HIP runtime multiplexes the streams of one priority level onto GPU_MAX_HW_QUEUES hardware queues (default 4) and streams
// that share a queue serialise: more sets than queues is SLOWER than fewer sets.  The library never touches the
// host's environment; it reads the limit the runtime was started with.
uint32_t hw_queue_limit()
{
    const char* e = getenv("GPU_MAX_HW_QUEUES");
    const long q = e ? strtol(e, nullptr, 10) : 4;
    return q < 1 ? 1u : (q > 1024 ? 1024u : (uint32_t)q);
}

// A stream whose queue carries a CU mask -- here: every CU of the current device, no bit beyond them -- cannot be pooled by the
// runtime, so it always gets a hardware queue of its own, at normal priority, whatever GPU_MAX_HW_QUEUES says.  The call takes
// no flags: such a stream synchronises with the null stream.  false, with the error cleared and s.h null: no
// such stream to be had.
bool create_masked(Stream& s)
{
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        return false;
    }
    std::vector<uint32_t> mask(((uint32_t)cus + 31u) / 32u, 0xFFFFFFFFu);       // hipDeviceProp_t::multiProcessorCount bits
    if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
    if (hipExtStreamCreateWithCUMask(&s.h, (uint32_t)mask.size(), mask.data()) == hipSuccess) return true;
    (void)hipGetLastError();
    s.h = nullptr;
    return false;
}

// The default number of passes in flight follows the queues the set streams really have (profiles/normal_queues_ab.md).
// ownQueues: set 0's stream was made with a queue of its own (create_set_stream), and so is every other set's: all PT_WF_SETS.
// Otherwise every stream of the process shares the one normal pool, one queue of it the context stream's: >= 16 queues -> 12 sets,
// >= 8 -> 6, otherwise 3.  PTSetPassesInFlight overrides.
uint32_t default_passes_in_flight(bool ownQueues)
{
    const uint32_t q = hw_queue_limit();
    const uint32_t n = ownQueues || q >= 16u ? 12u : (q >= 8u ? 6u : 3u);
    return n < (uint32_t)PT_WF_SETS ? n : (uint32_t)PT_WF_SETS;
}

// Resolved lazily: a host on a runtime-only ROCm install without librocprofiler-sdk-roctx still loads the plugin, and the
// ranges are no-ops.
struct RoctxApi {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    RoctxApi()
    {
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_GLOBAL);
        if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_GLOBAL);
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
};
const RoctxApi& roctx_api() { static RoctxApi api; return api; }

int upload(PTContext* c, DeviceBuffer& b, const void* src, size_t bytes)
{
    int rc = b.reserve(bytes);          // set_scene has drained every stream of the context
    if (rc || bytes == 0) return rc;
    HIP_TRY(hipMemcpyAsync(b.ptr, src, bytes, hipMemcpyHostToDevice, c->stream));
    return PT_OK;
}

// Does material slot value f (>= 0; util/material.hlsl:8-82 reads the slots as float indices, < 0 = none) name a usable texture
// of textureData?  0 = yes, t is its index; otherwise why not: 1 = not a finite number, 2 = no descriptor, 3 = a descriptor
// {w, h, offset} that reaches outside textureData
int texture_slot(float f, const uint32_t* textureData, uint64_t textureDataUints, uint64_t& t)
{
    if (!(f >= 0.0f && f < 1.0e9f)) return 1;
    t = (uint64_t)f;
    if (4 * t + 3 >= textureDataUints) return 2;
    const uint32_t* d = textureData + 4 * t;
    if (d[0] == 0 || d[1] == 0 || (uint64_t)d[2] + (uint64_t)d[0] * d[1] > textureDataUints) return 3;
    return 0;
}

// One host pass over everything the kernels will index with scene data (D3D / WebGPU robust buffer access returns zeros for
// an out-of-range read; a HIP kernel faults the GPU): triangle -> material, material -> texture descriptor -> texels,
// CWBVH node -> child nodes / triangle rows, triangle row -> attribute record, TLAS node -> nodes / instances, instance ->
// BLAS offsets.  Costs a few milliseconds for a 250k-triangle scene, once per PTSetScene.
bool validate_scene(const PTSceneDesc& s, std::string& why)
{
    const uint64_t nodeCount = s.bvhNodesBytes / 80u, triRows = s.bvhTrisBytes / 16u, attrCount = s.triAttrsBytes / 128u;
    const bool textures = (s.features & PT_FEATURE_HAS_TEXTURES) != 0, tlasOn = (s.features & PT_FEATURE_HAS_TLAS) != 0;
    auto bad = [&](const std::string& m) { why = m; return false; };
    // materials -> textures
    const float* mats = (const float*)s.materials;
    for (uint32_t m = 0; m < s.materialCount; ++m) {
        for (int k : kTextureSlots) {
            const float f = mats[(size_t)m * 32 + k];
            if (!textures || f < 0.0f) continue;
            uint64_t t = 0;
            switch (texture_slot(f, s.textureData, s.textureDataUints, t)) {
            case 1: return bad("material " + std::to_string(m) + ": texture index is not a finite number");
            case 2: return bad("material " + std::to_string(m) + ": texture index " + std::to_string(t) + " has no descriptor");
            case 3: return bad("texture " + std::to_string(t) + ": descriptor {w, h, offset} reaches outside textureData");
            }
        }
    }
    // triangles -> materials
    const uint8_t* attrs = (const uint8_t*)s.triAttrs;
    if (!tlasOn)
        for (uint64_t i = 0; i < attrCount; ++i) {
            uint32_t mi;
            memcpy(&mi, attrs + i * 128 + 120, 4);
            if (mi >= s.materialCount) return bad("triangle " + std::to_string(i) + ": materialIndex " + std::to_string(mi) + " >= materialCount");
        }
    // CWBVH: children, triangle rows, primitive indices -- decoded EXACTLY as the kernels decode them (cwbvh_node_hitmask,
    // pt_device.h): a child is inner iff bits 3 and 4 of its meta byte are both set, whatever the upper bits say; a leaf's
    // triangle bits are (meta >> 5) & 7 shifted to bit (meta & 31).  Every BLAS is walked from its root with a visited map, so a
    // child pointer that points back (a cycle: traversal would never end) or sideways (two parents) is refused, and only what
    // a ray can reach has to be in range.  With HAS_TLAS the arrays hold several BLASes back to back; every distinct
    // (bvhOffset, triOffset, triAttributeOffset) triple is walked once.
    const uint8_t* nodes = (const uint8_t*)s.bvhNodes;
    const float* tris = (const float*)s.bvhTris;
    std::vector<uint8_t> seen(nodeCount, 0);
    auto walk_blas = [&](uint64_t nodeOff, uint64_t triOff, uint64_t attrOff, const std::string& who) -> bool {
        std::vector<uint32_t> todo(1, 0u);
        std::vector<uint64_t> touched;
        bool ok = true;
        while (ok && !todo.empty()) {
            const uint32_t rel = todo.back();
            todo.pop_back();
            const uint64_t n = nodeOff + rel;
            if (n >= nodeCount) { ok = bad(who + ": child index past the node array"); break; }
            if (seen[n]) { ok = bad(who + ": node " + std::to_string(n) + " is reachable twice (the node graph is not a tree)"); break; }
            seen[n] = 1;
            touched.push_back(n);
            const uint8_t* p = nodes + n * 80;
            uint32_t childBase, triBase;
            memcpy(&childBase, p + 16, 4);
            memcpy(&triBase, p + 20, 4);
            const uint8_t imask = p[15];
            uint32_t inner = 0;
            for (int k = 0; k < 8 && ok; ++k) {
                const uint32_t m = p[24 + k];
                if (m == 0) continue;
                if ((m & 0x18u) == 0x18u) {
                    // the kernel shifts (meta >> 5) & 7 to bit 24 + slot: anything but 1 sets the hit bit of ANOTHER slot
                    if ((m >> 5) != 1u) { ok = bad(who + ": node " + std::to_string(n) + " has an inner child whose meta byte is not (1 << 5) | (24 + slot)"); break; }
                    if ((uint64_t)childBase + inner >= 0xFFFFFFFFull) { ok = bad(who + ": child index overflow"); break; }
                    todo.push_back(childBase + inner);
                    inner++;
                    continue;
                }
                const uint32_t first = m & 31u, bits = (m >> 5) & 7u;
                if (bits == 0u) continue;
                const uint32_t top = first + (31u - (uint32_t)__builtin_clz(bits));        // highest triangle bit of the 24-bit triangle mask
                if (top >= 24u) { ok = bad(who + ": node " + std::to_string(n) + " has a leaf whose triangle bits leave the 24-bit mask"); break; }
                for (uint32_t q = first; q <= top; ++q) {
                    if (!((bits >> (q - first)) & 1u)) continue;
                    const uint64_t row = triOff + triBase + (uint64_t)q * 3u;
                    if (row + 2 >= triRows) { ok = bad(who + ": triangle rows past the triangle array"); break; }
                    uint32_t prim;
                    memcpy(&prim, tris + (row + 2) * 4 + 3, 4);
                    if (attrOff + prim >= attrCount) { ok = bad(who + ": primitive index " + std::to_string(prim) + " has no attribute record"); break; }
                }
            }
            if (ok && inner != (uint32_t)__builtin_popcount(imask)) ok = bad(who + ": node " + std::to_string(n) + ": imask does not match its inner children");
        }
        if (tlasOn) for (uint64_t n : touched) seen[n] = 0;          // BLASes may share nodes between instances, never within one
        return ok;
    };
    if (!tlasOn) {
        if (!walk_blas(0, 0, 0, "BVH")) return false;
    } else {
        if (s.tlasIndexOffset < 16u) return bad("tlasIndexOffset < 16: HAS_TLAS needs at least one TLAS node");
        const uint64_t tlasNodes = s.tlasIndexOffset / 16u, indices = s.tlasDataFloats - s.tlasIndexOffset;
        const uint32_t* T = (const uint32_t*)s.tlasData;
        // the 2-wide TLAS is walked from node 0 as the kernel walks it (tlas.hlsl:246-331): children in range, no node twice
        {
            std::vector<uint8_t> seenT(tlasNodes, 0);
            std::vector<uint32_t> todo(1, 0u);
            while (!todo.empty()) {
                const uint32_t n = todo.back();
                todo.pop_back();
                if (n >= tlasNodes) return bad("TLAS child index " + std::to_string(n) + " past the TLAS nodes");
                if (seenT[n]) return bad("TLAS node " + std::to_string(n) + " is reachable twice (the TLAS is not a tree)");
                seenT[n] = 1;
                const uint32_t left = T[(size_t)n * 16 + 3], right = T[(size_t)n * 16 + 7], count = T[(size_t)n * 16 + 11], first = T[(size_t)n * 16 + 15];
                if (count == 0) { todo.push_back(left); todo.push_back(right); }
                else if ((uint64_t)first + count > indices) return bad("TLAS node " + std::to_string(n) + ": instance range past the index list");
            }
        }
        for (uint64_t i = 0; i < indices; ++i)
            if (T[s.tlasIndexOffset + i] >= s.instanceCount) return bad("TLAS index " + std::to_string(i) + " >= instanceCount");
        const uint8_t* inst = (const uint8_t*)s.gpuInstances;
        std::vector<std::array<int32_t, 3>> walked;                  // distinct BLASes already validated
        for (uint32_t i = 0; i < s.instanceCount; ++i) {
            int32_t off[4];
            memcpy(off, inst + (size_t)i * 144 + 128, 16);
            if (off[0] < 0 || (uint64_t)off[0] >= nodeCount || off[1] < 0 || (uint64_t)off[1] > triRows || off[2] < 0 || (uint64_t)off[2] > attrCount ||
                off[3] < 0 || (uint32_t)off[3] >= s.materialCount)
                return bad("instance " + std::to_string(i) + ": bvhOffset / triOffset / triAttributeOffset / materialIndex out of range");
            const std::array<int32_t, 3> key = {off[0], off[1], off[2]};
            bool done = false;
            for (const auto& k : walked) if (k == key) { done = true; break; }
            if (done) continue;
            if (!walk_blas((uint64_t)off[0], (uint64_t)off[1], (uint64_t)off[2], "instance " + std::to_string(i))) return false;
            walked.push_back(key);
        }
    }
    return true;
}

// PTSetScene: drop the update generations (the scene's own buffers become current again)
void discard_updates(PTContext* c)
{
    PTContext::Update& u = c->update;
    if (u.stream) hipStreamSynchronize(u.stream);
    for (PTContext::UpdGroup* g : {&u.inst, &u.lights, &u.mats, &u.geom, &u.attrs}) *g = PTContext::UpdGroup();
    u.geometry = PTContext::Geometry();
    u.tlasWork.release();
    u.tlasW = {};
    u.pending = false;
}

} // namespace

RoctxRange::RoctxRange(const char* name) { if (roctx_api().push) roctx_api().push(name); }
RoctxRange::~RoctxRange() { if (roctx_api().pop) roctx_api().pop(); }

int create_set_stream(uint32_t index, Stream& s, bool* ownQueue)
{
    if (ownQueue) *ownQueue = false;
    if (s.h) return PT_OK;
    // A host that asked for 16 queues or more keeps what it had, call for call: the normal pool has a queue for every set
    // (profiles/own_queues_ab.md: that path reads less for even one more call in PTCreate).  Below that every set stream carries
    // the all-CU mask; at most PT_WF_SETS set streams exist per context, so at most that many queues outside the pool.  Where
    // the runtime refuses, the stream is an ordinary one of the normal pool.
    if (hw_queue_limit() < 16u && index < (uint32_t)PT_WF_SETS && create_masked(s)) {
        if (ownQueue) *ownQueue = true;
        return PT_OK;
    }
    return create(s);
}

int drain_events(PTContext* c)
{
    for (auto& ep : c->pending) {
        HIP_TRY(hipEventSynchronize(ep.stop));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ep.start, ep.stop));
        c->timings.passes++;
        c->timings.kernelMsTotal += ms;
        c->timings.kernelMsLast = ms;
        c->timings.kernelLaunches += ep.launches;
        c->freeEvents.push_back(std::move(ep));
    }
    c->pending.clear();
    return PT_OK;
}

int set_scene(PTContext* c, const PTSceneDesc* hostScene, bool validate)
{
    if (!c || !hostScene) return fail(PT_ERR_INVALID_ARG, "ctx/scene == NULL");
    PTSceneDesc sceneCopy;
    if (int rc = import_struct(hostScene, sceneCopy, PT_SCENE_DESC_MIN_SIZE, "PTSceneDesc", "ctx/scene == NULL")) return rc;
    const PTSceneDesc* s = &sceneCopy;
    RoctxRange range("PTSetScene (validate + upload)");
    const bool tlasOn = (s->features & PT_FEATURE_HAS_TLAS) != 0;
    if (tlasOn && (!s->tlasData || s->tlasDataFloats < 16 || !s->gpuInstances || s->instanceCount == 0 ||
                   s->tlasIndexOffset >= s->tlasDataFloats || s->tlasIndexOffset % 16 != 0))
        return fail(PT_ERR_INVALID_ARG, "HAS_TLAS needs tlasData (nodes + indices), tlasIndexOffset and gpuInstances");
    if (!s->bvhNodes || s->bvhNodesBytes < 80 || s->bvhNodesBytes % 80) return fail(PT_ERR_INVALID_ARG, "bvhNodes must be a non-empty multiple of 80 bytes");
    if ((uint64_t)s->bvhNodesBytes >= (1ull << 32)) return fail(PT_ERR_INVALID_ARG, "bvhNodes of 4 GiB and more are not supported (the kernels address nodes with 32-bit byte offsets)");
    if (!s->bvhTris || s->bvhTrisBytes % 48) return fail(PT_ERR_INVALID_ARG, "bvhTris must be a multiple of 48 bytes");
    if (!s->triAttrs || s->triAttrsBytes % 128) return fail(PT_ERR_INVALID_ARG, "triAttrs must be a multiple of 128 bytes");
    if (!s->materials || s->materialCount == 0) return fail(PT_ERR_INVALID_ARG, "materials missing");
    if ((s->features & PT_FEATURE_HAS_LIGHTS) && (!s->lights || s->lightCount == 0)) return fail(PT_ERR_INVALID_ARG, "HAS_LIGHTS without lights");
    if ((s->features & PT_FEATURE_HAS_TEXTURES) && (!s->textureData || s->textureDataUints == 0)) return fail(PT_ERR_INVALID_ARG, "HAS_TEXTURES without texture data");
    const bool envOn = (s->features & PT_FEATURE_HAS_ENVIRONMENT_TEXTURE) != 0;
    if (envOn && (!s->envTexture || s->envWidth == 0 || s->envHeight == 0 || (uint64_t)s->envWidth * s->envHeight > 0x7FFFFFFFull))
        return fail(PT_ERR_INVALID_ARG, "HAS_ENVIRONMENT_TEXTURE needs envTexture, envWidth, envHeight");
    if (validate) {
        std::string why;
        if (!validate_scene(*s, why)) return fail(PT_ERR_INVALID_ARG, "scene refused: " + why);
    }
    HIP_TRY(hipSetDevice(c->device));
    for (auto& set : c->sets) if (set.stream) HIP_TRY(hipStreamSynchronize(set.stream));   // no pass may still read the old scene
    HIP_TRY(hipStreamSynchronize(c->stream));
    discard_updates(c);
    c->lightmaps.count = 0;             // the bound lightmaps' spans named the old scene (Part 22)
    int rc;
    if ((rc = upload(c, c->nodes, s->bvhNodes, s->bvhNodesBytes))) return rc;
    if ((rc = upload(c, c->tris, s->bvhTris, s->bvhTrisBytes))) return rc;
    if ((rc = upload(c, c->attrs, s->triAttrs, s->triAttrsBytes))) return rc;
    if ((rc = upload(c, c->materials, s->materials, (size_t)s->materialCount * 128))) return rc;
    const bool lights = (s->features & PT_FEATURE_HAS_LIGHTS) != 0;
    const bool textures = (s->features & PT_FEATURE_HAS_TEXTURES) != 0;
    if (lights && (rc = upload(c, c->lights, s->lights, (size_t)s->lightCount * 64))) return rc;
    if (textures && (rc = upload(c, c->tex, s->textureData, (size_t)s->textureDataUints * 4))) return rc;
    if (tlasOn && (rc = upload(c, c->tlas, s->tlasData, (size_t)s->tlasDataFloats * 4))) return rc;
    if (tlasOn && (rc = upload(c, c->instances, s->gpuInstances, (size_t)s->instanceCount * 144))) return rc;
    std::vector<float> byLeaf, bfs;
    if (tlasOn) {
        // what entering an instance reads (util/tlas.hlsl:129-147: TLASData[TLASIndexOffset + k] -> GPUInstance) as ONE record per
        // index slot k, in the order the TLAS leaves list them: the kernels save a dependent fetch per instance entry
        const uint64_t indices = s->tlasDataFloats - s->tlasIndexOffset;
        const uint32_t* T = (const uint32_t*)s->tlasData;
        const float* inst = (const float*)s->gpuInstances;
        byLeaf.assign((size_t)indices * 24, 0.0f);
        for (uint64_t k = 0; k < indices; ++k) {
            const uint32_t idx = T[s->tlasIndexOffset + k];                 // validated above: < instanceCount
            memcpy(&byLeaf[k * 24], inst + (size_t)idx * 36 + 16, 20 * sizeof(float));      // worldToLocal + the offsets row
            memcpy(&byLeaf[k * 24 + 20], &idx, 4);
        }
        if ((rc = upload(c, c->instByLeaf, byLeaf.data(), byLeaf.size() * sizeof(float)))) return rc;
        // the nodes reachable from node 0, renumbered breadth-first: the top of the tree -- what nearly every ray visits -- becomes
        // the FIRST nodes of the array, which pt_wf_trace_refill_tlas copies into LDS.  Children indices are rewritten, every other
        // word (boxes, instance count, first index slot) is copied, so a walk visits the same nodes in the same order.
        const uint32_t tlasNodes = s->tlasIndexOffset / 16u;
        std::vector<uint32_t> order(1, 0u), renum(tlasNodes, 0xFFFFFFFFu);
        renum[0] = 0u;
        for (size_t i = 0; i < order.size(); ++i) {
            const uint32_t* n = T + (size_t)order[i] * 16;
            if (n[11] != 0u) continue;                                       // a leaf: instance count > 0
            for (uint32_t child : {n[3], n[7]})                              // < tlasNodes when the scene was validated; otherwise left alone
                if (child < tlasNodes && renum[child] == 0xFFFFFFFFu) { renum[child] = (uint32_t)order.size(); order.push_back(child); }
        }
        bfs.resize(order.size() * 16);
        for (size_t i = 0; i < order.size(); ++i) {
            uint32_t* d = (uint32_t*)&bfs[i * 16];
            memcpy(d, T + (size_t)order[i] * 16, 64);
            if (d[11] == 0u) { if (d[3] < tlasNodes) d[3] = renum[d[3]]; if (d[7] < tlasNodes) d[7] = renum[d[7]]; }
        }
        if ((rc = upload(c, c->tlasBfs, bfs.data(), bfs.size() * sizeof(float)))) return rc;
    }
    std::vector<float> cdf;
    float cdfSum = 0.0f;
    if (envOn) {
        // OnEnvTexReadback (PathTracer.cs:297-306): running fp32 sum of Color.grayscale = 0.299 r + 0.587 g + 0.114 b
        const size_t n = (size_t)s->envWidth * s->envHeight;
        cdf.resize(n);
        cdfSum = pt_env_build_cdf(s->envTexture, n, cdf.data());
        if ((rc = upload(c, c->envTex, s->envTexture, n * 16))) return rc;
        if ((rc = upload(c, c->envCdf, cdf.data(), n * 4))) return rc;
    }
    if (lights) {                                  // room for the per-light constants, filled below once the scene view is complete
        if ((rc = c->lightConst.reserve((size_t)s->lightCount * 64))) return rc;     // drained above, like upload()
    }
    HIP_TRY(hipStreamSynchronize(c->stream));      // inputs are borrowed for the duration of the call only
    c->scene.nodes = (const uint4*)c->nodes.ptr;
    c->scene.tris = (const float4*)c->tris.ptr;
    c->scene.attrs = (const float4*)c->attrs.ptr;
    c->scene.materials = (const float4*)c->materials.ptr;
    c->scene.lights = lights ? (const float4*)c->lights.ptr : nullptr;
    c->scene.tex = textures ? (const uint32_t*)c->tex.ptr : nullptr;
    c->scene.lightCount = lights ? (int32_t)s->lightCount : 0;
    c->scene.materialCount = s->materialCount;
    c->scene.hasLights = lights ? 1u : 0u;
    c->scene.hasTextures = textures ? 1u : 0u;
    c->scene.tlas = tlasOn ? (const float*)c->tlas.ptr : nullptr;
    c->scene.instances = tlasOn ? (const float4*)c->instances.ptr : nullptr;
    c->scene.instByLeaf = tlasOn ? (const float4*)c->instByLeaf.ptr : nullptr;
    c->scene.tlasBfs = tlasOn ? (const float*)c->tlasBfs.ptr : nullptr;
    c->scene.tlasNodeCount = tlasOn ? (uint32_t)(bfs.size() / 16) : 0u;
    c->scene.tlasIndexOffset = tlasOn ? s->tlasIndexOffset : 0u;
    c->scene.hasTlas = tlasOn ? 1u : 0u;
    c->scene.envTex = envOn ? (const float4*)c->envTex.ptr : nullptr;
    c->scene.envCdf = envOn ? (const float*)c->envCdf.ptr : nullptr;
    c->scene.envW = envOn ? (int32_t)s->envWidth : 0;
    c->scene.envH = envOn ? (int32_t)s->envHeight : 0;
    c->scene.envCdfSum = cdfSum;
    c->scene.hasEnvTex = envOn ? 1u : 0u;
    c->scene.lightConst = lights ? (const float4*)c->lightConst.ptr : nullptr;
    c->update.instanceCount = tlasOn ? s->instanceCount : 0u;
    c->update.sceneLightCount = lights ? s->lightCount : 0u;
    c->update.origTlasNodes = tlasOn ? s->tlasIndexOffset / 16u : 0u;
    ++c->update.lightGeneration;
    c->update.lightTypes.clear();
    for (uint32_t l = 0; lights && l < s->lightCount; ++l) c->update.lightTypes.push_back(((const PTLight*)s->lights)[l].type);
    std::vector<uint32_t>& valid = c->update.validTextures;
    valid.clear();
    if (textures) {                                // what PTUpdateMaterials may name: the textures this scene's materials named
        const float* mats = (const float*)s->materials;
        for (uint32_t m = 0; m < s->materialCount; ++m)
            for (int k : kTextureSlots) {
                uint64_t t = 0;
                if (texture_slot(mats[(size_t)m * 32 + k], s->textureData, s->textureDataUints, t) == 0) valid.push_back((uint32_t)t);
            }
        std::sort(valid.begin(), valid.end());
        valid.erase(std::unique(valid.begin(), valid.end()), valid.end());
    }
    if (lights) {
        HIP_TRY(pt_launch_derive_lights(c->scene, (float4*)c->lightConst.ptr, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->hasScene = true;
    return PT_OK;
}

extern "C" {

PT_API int PTCreate(int deviceIndex, PTContext** outCtx)
{
    if (!outCtx) return fail(PT_ERR_INVALID_ARG, "outCtx == NULL");
    *outCtx = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(PT_ERR_NO_DEVICE, std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                                          "); this library has no CPU fallback");
    if (deviceIndex < 0 || deviceIndex >= count) return fail(PT_ERR_INVALID_ARG, "deviceIndex out of range");
    HIP_TRY(hipSetDevice(deviceIndex));
    PTContext* c = new PTContext();
    c->device = deviceIndex;
    hipError_t se = hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking);
    if (se != hipSuccess) { delete c; return fail(PT_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(se)); }
    // Where the sets are to have queues of their own, set 0's stream is made here: whether it really has one decides the default
    // number of passes in flight.  Otherwise (16 queues or more) not one call differs from what it was.
    if (hw_queue_limit() < 16u) {
        if (int rc = create_set_stream(0u, c->sets[0].stream, &c->ownQueues)) { delete c; return rc; }
    }
    c->numSets = default_passes_in_flight(c->ownQueues);
    se = hipMalloc(&c->dStats.ptr, (16 + 4) * sizeof(unsigned long long));       // PTStats, PTRepackStats
    if (se != hipSuccess) { delete c; return fail(PT_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(se)); }
    hipMemsetAsync(c->dStats.ptr, 0, (16 + 4) * sizeof(unsigned long long), c->stream);
    *outCtx = c;
    return PT_OK;
}

PT_API int PTDestroy(PTContext* c)
{
    if (!c) return PT_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->update.stream) hipStreamSynchronize(c->update.stream);
    for (auto& set : c->sets) if (set.stream) hipStreamSynchronize(set.stream);
    delete c;
    return PT_OK;
}

PT_API int PTSetScene(PTContext* c, const PTSceneDesc* hostScene) { return set_scene(c, hostScene, true); }

PT_API int PTSetTileOwnership(PTContext* c, int rank, int worldSize)
{
    if (!c || worldSize < 1 || rank < 0 || rank >= worldSize) return fail(PT_ERR_INVALID_ARG, "bad rank/worldSize");
    c->rank = rank;
    c->world = worldSize;
    return PT_OK;
}

PT_API int PTSynchronize(PTContext* c)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

PT_API void* PTGetStream(PTContext* c) { return c ? (void*)c->stream : nullptr; }

PT_API int PTSetStatsLevel(PTContext* c, int level)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    c->statsLevel = level > 0 ? 1 : 0;
    return PT_OK;
}

PT_API int PTGetStats(PTContext* c, PTStats* out)
{
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "ctx/out == NULL");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long h[16];
    HIP_TRY(hipMemcpyAsync(h, c->dStats.ptr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    static_assert(sizeof(PTStats) == 16 * 8, "PTStats is 16 counters");
    memcpy(out, h, sizeof(PTStats));
    return PT_OK;
}

// the four counters the repack's decide kernel adds to on the device (pt_wavefront.hip), read on demand
PT_API int PTGetRepackStats(PTContext* c, PTRepackStats* out)
{
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "ctx/out == NULL");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long h[4];
    HIP_TRY(hipMemcpyAsync(h, (unsigned long long*)c->dStats.ptr + 16, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    static_assert(sizeof(PTRepackStats) == 4 * 8, "PTRepackStats is 4 counters");
    memcpy(out, h, sizeof(PTRepackStats));
    return PT_OK;
}

PT_API int PTResetStats(PTContext* c)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->dStats.ptr, 0, 16 * sizeof(unsigned long long), c->stream));
    return PT_OK;
}

PT_API int PTSetProfiling(PTContext* c, int enabled)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    c->profiling = enabled != 0;
    return PT_OK;
}

PT_API int PTGetTimings(PTContext* c, PTTimings* out)
{
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "ctx/out == NULL");
    HIP_TRY(hipSetDevice(c->device));
    int rc = drain_events(c);
    if (rc) return rc;
    *out = c->timings;
    return PT_OK;
}

PT_API int PTResetTimings(PTContext* c)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    int rc = drain_events(c);
    if (rc) return rc;
    c->timings = PTTimings{};
    return PT_OK;
}

PT_API int PTGetSchedule(PTContext* c)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    return effective_schedule(c);
}

PT_API int PTSetSchedule(PTContext* c, int schedule)
{
    if (!c) return fail(PT_ERR_INVALID_ARG, "ctx == NULL");
    if (schedule < -1 || schedule > 4)
        return fail(PT_ERR_UNSUPPORTED, "unknown schedule (0 = megakernel, 1 = wavefront + refill trace, 2 = wavefront, one ray per lane, 3 = wavefront + persistent dynamic-chunk trace, 4 = fused persistent wavefront)");
    c->schedule = schedule;
    return PT_OK;
}

PT_API int PTSetPassesInFlight(PTContext* c, int passes)
{
    if (!c || passes < 0 || passes > PT_WF_SETS) return fail(PT_ERR_INVALID_ARG, "ctx == NULL or passes outside 0.." + std::to_string(PT_WF_SETS));
    HIP_TRY(hipSetDevice(c->device));
    for (auto& set : c->sets) if (set.stream) HIP_TRY(hipStreamSynchronize(set.stream));
    c->numSets = passes == 0 ? default_passes_in_flight(c->ownQueues) : (uint32_t)passes;
    c->nextSet = 0u;
    // sets that are no longer used give their memory back
    for (uint32_t k = c->numSets; k < (uint32_t)PT_WF_SETS; ++k) {
        c->sets[k].arena.release();
        c->sets[k].wf = PTWfBuffers{};
    }
    return PT_OK;
}

PT_API int PTSetSubFrames(PTContext* c, int subFrames)
{
    if (!c || subFrames < 1 || subFrames > PT_WF_SETS) return fail(PT_ERR_INVALID_ARG, "ctx == NULL or subFrames outside 1.." + std::to_string(PT_WF_SETS));
    c->subFrames = (uint32_t)subFrames;
    return PT_OK;
}

PT_API int PTGetPassesInFlight(PTContext* c) { return c ? (int)c->numSets : fail(PT_ERR_INVALID_ARG, "ctx == NULL"); }

PT_API int PTSetWavefrontIterations(PTContext* c, int iterations)
{
    if (!c || iterations < 0) return fail(PT_ERR_INVALID_ARG, "ctx == NULL or iterations < 0");
    c->wfIterations = (uint32_t)iterations;
    return PT_OK;
}

PT_API const char* PTGetLastError(void) { return g_lastError.c_str(); }
PT_API int PTGetVersion(void) { return (0 << 16) | 2; }

} // extern "C"
