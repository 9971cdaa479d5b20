/*
 * ptmi_plugin.h — C-ABI of libunity-webgpu-pathtracer-plugin.so, the MI355X drop-in.
 *
 * Part 1 re-exports, symbol for symbol, the native plugin the Unity C# host binds with
 *   [DllImport("unity-webgpu-pathtracer-plugin")]  (Assets/Scripts/util/TinyBVH.cs:15-50)
 * and that the reference builds from Assets/Plugins/Web/plugin.cpp (Plugin/CMakeLists.txt:7-11).
 *
 * Part 2 adds the render entry points.  The reference has no render FFI: it renders
 * through Unity's ComputeShader API (Assets/Scripts/PathTracer.cs:226-252).  The PT*
 * functions below take exactly what those calls bind: the buffers of
 * BVHScene.PrepareShader (Assets/Scripts/util/BVHScene.cs:140-167) and the uniforms of
 * PathTracer.OnRenderImage (PathTracer.cs:230-249), and replace DispatchCompute (:251).
 *
 * Conventions: cdecl, blittable arguments only (pointers, ints, floats, POD structs);
 * inputs are borrowed for the duration of the call; outputs returned by Get*Data are
 * owned by the library until the matching Destroy*.  Functions that returned C++ `bool`
 * in the reference return a full-width int 0/1 here (ABI-compatible with both the 1-byte
 * and the 4-byte marshalling of C# `bool`).  Nothing in this library ever calls exit():
 * degenerate input yields a negative handle / error code and PTGetLastError() text.
 * Like the reference (unsynchronised globals, plugin.cpp:5-6) the handle tables are
 * single-threaded by contract.
 */
#ifndef PTMI_PLUGIN_H
#define PTMI_PLUGIN_H

#include <stdint.h>
#include "ptmi_layouts.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define PT_API __declspec(dllexport)
#else
#define PT_API __attribute__((visibility("default")))
#endif

/* ------------------------------------------------------------------------------------
 * Part 1 — acceleration-structure exports (replaces Assets/Plugins/Web/plugin.h:14-29)
 * ------------------------------------------------------------------------------------ */

/* plugin.cpp:35-40.  Synchronous CWBVH build over 3*triangleCount 16-byte vertices
 * (w ignored).  Returns the handle (first free slot), or -1 on triangleCount <= 0 / NULL. */
PT_API int   BuildBVH(const PTFloat4* vertices, int triangleCount);
/* plugin.cpp:42-52.  Out-of-range or already-destroyed handle is a no-op. */
PT_API void  DestroyBVH(int index);
/* plugin.cpp:54-58 */
PT_API int   IsBVHReady(int index);
/* plugin.cpp:23-33.  Opaque object pointer (never dereferenced by the C# host). */
PT_API void* GetBVHPtr(int index);
PT_API void* GetBVH(int index);
/* plugin.cpp:60-64.  BYTES of CWBVH node data (nodes * 80); 0 for an invalid handle. */
PT_API int   GetCWBVHNodesSize(int index);
/* plugin.cpp:66-70.  BYTES of CWBVH triangle data (triangles * 48). */
PT_API int   GetCWBVHTrisSize(int index);
/* plugin.cpp:72-86.  Borrowed pointers, valid until DestroyBVH(index). */
PT_API int   GetCWBVHData(int index, PTFloat4** bvhNodes, PTFloat4** bvhTris);

/* No reference counterpart: the same CWBVH format built ON the MI355X -- LBVH (63-bit Morton keys, radix
 * sort, Karras radix tree), greedy surface-area collapse to 8-wide, CWBVH encode, all in HIP kernels.  The tree differs from
 * BuildBVH's binned-SAH tree (so the bytes differ), every ray finds the same closest hit.  The handle lives in BuildBVH's
 * table: GetCWBVHNodesSize / GetCWBVHTrisSize / GetCWBVHData / IsBVHReady / DestroyBVH apply.  Returns -1 on degenerate input
 * or when deviceIndex is not a HIP device (PTGetBVHBuildError() has the text); there is no CPU fallback behind this entry.
 * A vertex that is not finite is refused too ("vertex i is not finite", as PTRefitBVH says it): the host looks at the array
 * before the upload, outside the interval PTGetBVHBuildMs reports. */
PT_API int   PTBuildBVHDevice(int deviceIndex, const PTFloat4* vertices, int triangleCount);
PT_API const char* PTGetBVHBuildError(void);
/* Build time of a handle in milliseconds: host wall time of BuildBVH, device time (kernels only) of PTBuildBVHDevice. */
PT_API double PTGetBVHBuildMs(int index);

/* Refit (Part 9 has the rule): the handle of BuildBVH / PTBuildBVHDevice keeps its topology and takes the boxes and triangle
 * records of `vertices` (3 * triangleCount, the primitive order it was built from); GetCWBVHData then returns the refitted
 * arrays.  Host only, no GPU.  Returns 1, or 0 with PTGetBVHBuildError() set for a bad handle, a count mismatch or a
 * non-finite vertex.  PTRefitBVHArrays does the same in place on arrays the host copied out of a handle (nodeBytes = nodes *
 * 80, triBytes = triangleCount * 48); arrays that are no CWBVH of triangleCount triangles are refused, never followed. */
PT_API int   PTRefitBVH(int index, const PTFloat4* vertices, int triangleCount);
PT_API int   PTRefitBVHArrays(PTFloat4* bvhNodes, uint64_t nodeBytes, PTFloat4* bvhTris, uint64_t triBytes, const PTFloat4* vertices, int triangleCount);

/* plugin.cpp:111-118.  2-wide SAH BVH over the instances' world AABBs, Aila-Laine layout. */
PT_API int   BuildTLAS(const PTBlasInstance* instances, int instanceCount);
PT_API void  DestroyTLAS(int index);                                     /* plugin.cpp:120-130 */
PT_API int   IsTLASReady(int index);                                     /* plugin.cpp:132-136 */
PT_API int   GetTLASNodesSize(int index);                                /* plugin.cpp:138-142, bytes = nodes*64 */
PT_API int   GetTLASData(int index, PTFloat4** tlasNodes, uint32_t** tlasIndices); /* plugin.cpp:144-158 */

/* ------------------------------------------------------------------------------------
 * Part 2 — render entry points (replace the ComputeShader dispatch of PathTracer.cs:226-252)
 * ------------------------------------------------------------------------------------ */

typedef struct PTContext PTContext;   /* opaque; one per GPU (one process per GPU) */

/* Feature bits = the reference's shader keywords (PathTracer.compute:6-9). */
#define PT_FEATURE_HAS_LIGHTS    0x1u   /* HAS_LIGHTS   (PathTracer.cs:372,469) */
#define PT_FEATURE_HAS_TEXTURES  0x2u   /* HAS_TEXTURES (PathTracer.cs:185)     */
#define PT_FEATURE_HAS_TLAS      0x4u   /* HAS_TLAS     (BVHScene.cs:145-149): two-level traversal, util/tlas.hlsl       */
#define PT_FEATURE_HAS_ENVIRONMENT_TEXTURE 0x8u   /* HAS_ENVIRONMENT_TEXTURE (PathTracer.cs:119-143): util/sky.hlsl:7-88 */

/* Versioning of the two input structs: the FIRST member of PTSceneDesc and PTFrameParams is structSize = sizeof(the struct
 * the host was compiled against).  New members are only ever appended; the library reads min(structSize, its own sizeof)
 * bytes and treats the rest as zero, and rejects a structSize smaller than the first published layout (PT_ERR_INVALID_ARG:
 * almost always a host that forgot to set it).  So a host built against an older header keeps working unchanged. */

/* The buffers BVHScene.PrepareShader binds (BVHScene.cs:151-166) + Lights (PathTracer.cs:471).
 * All pointers are HOST pointers; PTSetScene copies them into HBM and VALIDATES every index the kernels will follow
 * (material indices, texture descriptors, CWBVH child / triangle ranges, primitive indices, TLAS nodes and instance offsets):
 * a scene that would make a kernel read out of bounds is refused with PT_ERR_INVALID_ARG instead of faulting the GPU. */
typedef struct PTSceneDesc {
    uint32_t        structSize;      uint32_t _pad3;             /* = sizeof(PTSceneDesc) of the host's header */
    const void*     bvhNodes;        uint64_t bvhNodesBytes;     /* PTCwbvhNode[]          "BVHNodes"; below 4 GiB (53 M nodes): the kernels address nodes with 32-bit byte offsets */
    const void*     bvhTris;         uint64_t bvhTrisBytes;      /* PTCwbvhTri[]           "BVHTris"  */
    const void*     triAttrs;        uint64_t triAttrsBytes;     /* PTTriangleAttributes[] "TriangleAttributesBuffer" */
    const void*     materials;       uint32_t materialCount;  uint32_t _pad0;  /* PTMaterialData[] "Materials" */
    const void*     lights;          uint32_t lightCount;     uint32_t _pad1;  /* PTLight[] "Lights" + LightCount */
    const uint32_t* textureData;     uint64_t textureDataUints;  /* "TextureData": K x {w,h,offset,0} then texels */
    uint32_t        features;        uint32_t _pad2;             /* PT_FEATURE_* */
    /* HAS_TLAS only (BVHScene.cs:155-160, 700-758).  bvhNodes / bvhTris / triAttrs then hold the per-mesh BLASes back to back
     * and each PTGpuInstance carries its offsets into them. */
    const float*    tlasData;        uint64_t tlasDataFloats;    /* "TLASData": PTTlasNode[] (16 floats each) then the instance indices */
    uint32_t        tlasIndexOffset; uint32_t instanceCount;     /* "TLASIndexOffset" (in floats); number of PTGpuInstance           */
    const void*     gpuInstances;                                /* PTGpuInstance[]        "BLASInstances"                            */
    /* HAS_ENVIRONMENT_TEXTURE only: the RGBAFloat copy of PathTracer.environmentTexture (PathTracer.cs:125-137), envWidth x
     * envHeight float4, in the order of the readback array `data[i]` the reference builds its CDF from (PathTracer.cs:297-306).
     * PTSetScene builds "EnvironmentCDF" / EnvironmentCdfSum from it exactly as OnEnvTexReadback does (sequential fp32 sum of
     * Color.grayscale).  SampleLevel(uv) is restated as bilinear with clamp addressing; memory row r is the texel row at
     * v = 1 - (r + 0.5) / envHeight, which makes SampleEnvMap's `uv.y = 1 - uv.y` (sky.hlsl:71) address the row whose CDF entry
     * it picked.  (Sampler state and row order belong to Unity's platform layer: parity unpinned there, see DESIGN.md.) */
    const float*    envTexture;      uint32_t envWidth;  uint32_t envHeight;
} PTSceneDesc;
#define PT_SCENE_DESC_MIN_SIZE  ((uint32_t)(uintptr_t)&((PTSceneDesc*)0)->envTexture)      /* layout before the environment texture */

/* The uniform block PathTracer.OnRenderImage sets every frame (PathTracer.cs:230-249;
 * declarations util/globals.hlsl:7-17, util/camera.hlsl:7-10, PathTracer.compute:40-41).
 * Matrices are 16 floats in Unity Matrix4x4 memory order: element (row r, col c) at [c*4+r],
 * applied to column vectors (mul(M, v)). */
typedef struct PTFrameParams {
    uint32_t structSize;              /* = sizeof(PTFrameParams) of the host's header (see "Versioning" above) */
    uint32_t _pad0;
    float    CamInvProj[16];          /* _camera.projectionMatrix.inverse  (PathTracer.cs:230) */
    float    CamToWorld[16];          /* _camera.cameraToWorldMatrix       (PathTracer.cs:231) */
    uint32_t RngSeedRoot;             /* fresh random value per frame      (PathTracer.cs:233) */
    uint32_t MaxRayBounces;           /* host passes max(.,1)              (PathTracer.cs:234) */
    int32_t  SamplesPerPass;          /* host passes max(1,.)              (PathTracer.cs:235) */
    uint32_t OutputWidth;
    uint32_t OutputHeight;
    uint32_t CurrentSample;           /* samples already accumulated       (PathTracer.cs:238) */
    int32_t  EnvironmentMode;         /* 0 environment colour, 1 basic sky (PathTracer.cs:239) */
    float    EnvironmentIntensity;
    float    EnvironmentColor[4];
    float    EnvironmentMapRotation;  /* only read by HAS_ENVIRONMENT_TEXTURE (PathTracer.cs:243)  */
    float    FocalLength;
    float    Aperture;
    int32_t  UseFireflyFilter;
    float    MaxFireflyLuminance;
    int32_t  UseRussianRoulette;
    /* DispatchCompute(kernel, dispatchX, dispatchY, 1) group counts of 8x8 threads
     * (PathTracer.cs:203-208,251).  0,0 = cover every pixel (ceil).  The C# host uses integer
     * division there, so for sizes that are not multiples of 8 it leaves edge pixels untouched;
     * pass its values to reproduce that exactly. */
    uint32_t DispatchGroupsX;
    uint32_t DispatchGroupsY;
} PTFrameParams;
#define PT_FRAME_PARAMS_MIN_SIZE ((uint32_t)(uintptr_t)&((PTFrameParams*)0)->DispatchGroupsX) /* DispatchGroups default to 0, 0 */

/* Work counters, accumulated over passes since the last PTResetStats.  One "ray" is one
 * call of RayIntersectBvh (util/bvh.hlsl:126): SURVEY.md §8(d). */
typedef struct PTStats {
    uint64_t paths;                /* samples started (pixels * SamplesPerPass)            */
    uint64_t closestHitRays;       /* RayIntersect calls      (util/bvh.hlsl:217)          */
    uint64_t shadowRays;           /* ShadowRayIntersect calls (util/bvh.hlsl:228)         */
    uint64_t nodeVisits;           /* CWBVH nodes fetched + tested (80 B each)             */
    uint64_t triTests;             /* IntersectTriangle calls (48 B each)                  */
    uint64_t attrFetches;          /* TriangleAttributes fetched (128 B each)              */
    uint64_t materialFetches;      /* MaterialData fetched (128 B each)                    */
    uint64_t lightFetches;         /* Light records read (64 B each)                       */
    uint64_t texelFetches;         /* texels read (4 B each)                               */
    uint64_t texDescriptorFetches; /* texture descriptors read (16 B each)                 */
    uint64_t pixelsWritten;        /* Output texels written (16 B each)                    */
    uint64_t pixelsRead;           /* AccumulatedOutput texels read (16 B each)            */
    uint64_t maxStackDepth;        /* deepest traversal stack seen (reference limit is 32) */
    uint64_t stackOverflows;       /* walks that dropped a stack entry (Part 3: the overflow rule) */
    uint64_t tlasNodeVisits;       /* HAS_TLAS: TLAS nodes read (64 B each)                */
    uint64_t instanceVisits;       /* HAS_TLAS: BLAS instances entered (144 B each)        */
} PTStats;

/* Device-side timing of the render kernels, measured with HIP events recorded on the
 * context's own stream around each launch (enabled by PTSetProfiling). */
typedef struct PTTimings {
    uint64_t passes;               /* passes timed since the last reset          */
    double   kernelMsTotal;        /* sum of event-to-event kernel time, ms      */
    double   kernelMsLast;         /* the most recent pass                        */
    uint64_t kernelLaunches;       /* device kernels launched in those passes     */
} PTTimings;

/* Error codes (negative int returns). */
#define PT_OK                 0
#define PT_ERR_INVALID_ARG   -1
#define PT_ERR_NO_DEVICE     -2   /* HIP runtime / MI355X not available: the product path never falls back to a CPU */
#define PT_ERR_HIP           -3
#define PT_ERR_NO_SCENE      -4
#define PT_ERR_UNSUPPORTED   -5

/* Create a render context on HIP device `deviceIndex`.  Fails with PT_ERR_NO_DEVICE when
 * there is no GPU: there is no CPU fallback. */
PT_API int PTCreate(int deviceIndex, PTContext** outCtx);
PT_API int PTDestroy(PTContext* ctx);

/* Copy the scene buffers into HBM (replaces ComputeBuffer.SetData, BVHScene.cs:640-667). */
PT_API int PTSetScene(PTContext* ctx, const PTSceneDesc* scene);

/* Screen-tile sharding for one-process-per-GPU rendering (no reference counterpart;
 * SURVEY.md §8e).  The frame is cut into 16x16-pixel blocks; block (bx,by) belongs to rank
 * (bx + by) % worldSize.  A context renders only its own blocks and writes exact zeros
 * (rgba = 0) elsewhere, so that a sum over ranks reproduces the single-GPU frame bit for bit.
 * rank 0 / worldSize 1 (the default) owns everything. */
PT_API int PTSetTileOwnership(PTContext* ctx, int rank, int worldSize);

/* Frame assembly for tile sharding: a rank's OWNED tiles packed densely (16 bytes per owned pixel, in the order the kernels
 * enumerate pixels) instead of a whole zero-padded frame -- 1/worldSize of the bytes of a sum-reduce.  One process per GPU:
 * pack on every rank, gather the packed buffers on the root (RCCL gather: bench.py), unpack each rank's buffer there.
 * PTGetOwnedTileSlots: float4 slots of the packed buffer for THIS context's ownership and these params (includes padding of
 * partially covered blocks; differs by at most one block row between ranks -- size a gather by the maximum).
 * All buffers are DEVICE pointers on the context's device; the calls are ordered on the context's stream. */
PT_API int PTGetOwnedTileSlots(PTContext* ctx, const PTFrameParams* params, uint64_t* outFloat4Slots);
PT_API int PTPackOwnedTiles(PTContext* ctx, const PTFrameParams* params, const void* dFrame, void* dPacked);
/* Scatters the packed tiles of rank `rank` of `worldSize` into dFrame (any context may unpack any rank's buffer). */
PT_API int PTUnpackTiles(PTContext* ctx, const PTFrameParams* params, int rank, int worldSize, const void* dPacked, void* dFrame);

/* One process, N devices (a C or C# host without an MPI-style launcher): a group owns one context per device, replicates the
 * scene, gives context i the tiles of rank i of N, and assembles every pass on the first device: each device packs its tiles,
 * hipMemcpyPeerAsync moves them over xGMI, the root unpacks.  The per-device passes are enqueued from one host thread per
 * device.  Progressive accumulation works as on one GPU: every device keeps the history of its own tiles
 * (PTGroupFlipFrames / PTGroupResetFrames mirror PTFlipFrames / PTResetFrames on all of them).  The same device may be
 * listed more than once (rehearsal on a one-GPU box).  Frames are bit-identical to the single-GPU frame. */
typedef struct PTGroup PTGroup;
PT_API int PTCreateMulti(const int* deviceIndices, int deviceCount, PTGroup** outGroup);
PT_API int PTGroupDestroy(PTGroup* group);
PT_API int PTGroupSize(PTGroup* group);
PT_API PTContext* PTGroupGetContext(PTGroup* group, int index);      /* for PTSetSchedule / PTSetStatsLevel / ... per device */
PT_API int PTGroupSetScene(PTGroup* group, const PTSceneDesc* scene);
PT_API int PTGroupRenderPass(PTGroup* group, const PTFrameParams* params);
PT_API int PTGroupRenderPassBatch(PTGroup* group, const PTFrameParams* params, int count);   /* `count` passes per device as one launch sequence (PTRenderPassBatch), one assembly */
PT_API int PTGroupFlipFrames(PTGroup* group);
PT_API int PTGroupResetFrames(PTGroup* group);
PT_API int PTGroupSynchronize(PTGroup* group);
PT_API int PTGroupReadback(PTGroup* group, float* dstRGBA, uint64_t dstFloats);   /* the assembled frame of the last pass */
PT_API void* PTGroupGetAssembledFrame(PTGroup* group);                            /* its device pointer (first device)    */
PT_API int PTGroupGetStats(PTGroup* group, PTStats* out);                         /* summed over devices (max for maxStackDepth) */
PT_API int PTGroupResetStats(PTGroup* group);

/* One progressive pass = one DispatchCompute of the PathTracer kernel (PathTracer.cs:251),
 * using the context's internal ping-pong frames exactly as PathTracer.cs:246-247,268-272:
 * Output = frame[cur], AccumulatedOutput = frame[1-cur]; the caller advances CurrentSample
 * and calls PTFlipFrames()/PTResetFrames() as the C# host flips _currentRT / calls Reset(). */
PT_API int PTRenderPass(PTContext* ctx, const PTFrameParams* params);
PT_API int PTFlipFrames(PTContext* ctx);       /* _currentRT = 1 - _currentRT  (PathTracer.cs:271-272) */
PT_API int PTResetFrames(PTContext* ctx);      /* Reset(): _currentRT = 0      (PathTracer.cs:318-322) */

/* Same pass, but into caller-owned DEVICE buffers (float4 per pixel, row-major):
 * dOutput is written, dAccumulated (may be NULL when CurrentSample == 0) is read. */
PT_API int PTRenderPassTo(PTContext* ctx, const PTFrameParams* params, void* dOutput, const void* dAccumulated);

/* `count` consecutive progressive passes (1..8) enqueued as ONE launch sequence: params[j] are the uniforms of pass j and may
 * differ in RngSeedRoot and CurrentSample only.  The result in dOutput is bit-identical to calling PTRenderPassTo `count` times
 * with the caller ping-ponging two frames (pass j reads what pass j-1 wrote; pass 0 reads dAccumulated when its CurrentSample > 0):
 * the paths of different passes are independent and the running mean of PathTracer.compute:89-98 is applied pass by pass in the
 * resolve kernel -- only the intermediate frames are never stored.  For offline / converging renders (the reference keeps
 * dispatching passes until _maxSamples, PathTracer.cs:194-272) and for tile-sharded rendering, where one rank's share of one
 * pass is too small a launch to fill an MI355X: eight passes of a 1/8 share are one whole frame's worth of paths.  PTStats counts
 * pixelsWritten / pixelsRead as the `count` separate passes would. */
PT_API int PTRenderPassBatchTo(PTContext* ctx, const PTFrameParams* params, int count, void* dOutput, const void* dAccumulated);
/* The same over the context's internal frame pair: Output = the current frame, AccumulatedOutput = the other one, as PTRenderPass;
 * the caller advances _currentSample by count x SamplesPerPass and flips ONCE (the intermediate frames do not exist). */
PT_API int PTRenderPassBatch(PTContext* ctx, const PTFrameParams* params, int count);

/* Block until every pass launched so far has finished. */
PT_API int PTSynchronize(PTContext* ctx);
/* Copy the current Output frame (frame[cur]) to host memory: width*height float4. */
PT_API int PTReadback(PTContext* ctx, float* dstRGBA, uint64_t dstFloats);
/* Device pointer of internal frame `which` (0/1) or of the current Output frame (-1). */
PT_API void* PTGetFramePointer(PTContext* ctx, int which);
/* The presentation blit (Assets/Resources/Presentation.shader:36-73 with util/tonemap.hlsl), i.e. the uniforms
 * PathTracer.cs:255-264 sets on _presentationMaterial.  Mode = TonemapMode (PathTracer.cs:8-14). */
typedef struct PTPresentParams {
    uint32_t OutputWidth, OutputHeight;
    int32_t  Mode;            /* 0 none, 1 ACES, 2 Filmic, 3 Reinhard, 4 Lottes */
    int32_t  sRGB;            /* LinearToSrgb after the operator */
    float    Exposure, Brightness, Contrast, Saturation, Vignette;
} PTPresentParams;
/* dst = present(src): both DEVICE pointers to OutputWidth*OutputHeight float4; src == NULL reads the context's current
 * Output frame.  Ordered on the context stream after every pass launched so far (cmd.Blit after DispatchCompute). */
PT_API int PTPresent(PTContext* ctx, const PTPresentParams* params, const void* dSrc, void* dDst);
/* Presents the context's current Output frame into host memory (width*height float4). */
PT_API int PTPresentToHost(PTContext* ctx, const PTPresentParams* params, float* dstRGBA, uint64_t dstFloats);
/* ---- scene ingestion: the two compute shaders that turn Unity meshes / textures into the path
 * tracer's buffers, run on the MI355X.  Inputs and outputs are HOST memory; the work is staged through HBM. ---- */

/* One Dispatch of Assets/Resources/MeshProcessing.compute as BVHScene.ProcessMeshes sets it up (BVHScene.cs:489-553). */
#define PT_MESH_HAS_32_BIT_INDICES 0x1u   /* mesh.indexFormat == UInt32 (only read when indexBuffer != NULL) */
#define PT_MESH_HAS_NORMALS        0x2u
#define PT_MESH_HAS_TANGENTS       0x4u
#define PT_MESH_HAS_UVS            0x8u
typedef struct PTMeshDesc {
    const void* vertexBuffer;  uint64_t vertexBufferBytes;   /* mesh.GetVertexBuffer(0): interleaved, fp32 attributes      */
    const void* indexBuffer;   uint64_t indexBufferBytes;    /* mesh.GetIndexBuffer(); NULL = HAS_INDEX_BUFFER off          */
    uint32_t VertexStride, PositionOffset, NormalOffset, TangentOffset, UVOffset;   /* bytes (Utilities.FindVertexAttribute) */
    uint32_t MaterialIndex;
    uint32_t TriangleCount, OutputTriangleStart;
    float    LocalToWorld[16], WorldToLocal[16];              /* Unity Matrix4x4 memory order, as in PTFrameParams          */
    uint32_t flags;            uint32_t _pad;                 /* PT_MESH_HAS_*                                                */
} PTMeshDesc;
/* ProcessMeshes + the readback (BVHScene.cs:429-560): runs the kernel once per mesh and returns
 * VertexPositionBuffer (3 float4 per triangle, w = 0: BuildBVH's input) and TriangleAttributesBuffer (PTTriangleAttributes
 * per triangle).  totalTriangles = the size of both outputs; every mesh writes [OutputTriangleStart, +TriangleCount). */
PT_API int PTProcessMeshes(PTContext* ctx, const PTMeshDesc* meshes, uint32_t meshCount, uint32_t totalTriangles,
                           float* outVertexPositions, void* outTriangleAttributes);

/* The texture loop of BVHScene.UpdateMaterialData (BVHScene.cs:386-417) over Assets/Resources/CopyTextureData.compute:
 * every texture (RGBA fp32 texels, row y = Texture.Load(int3(x, y, 0))) becomes a {w, h, offset, 0} descriptor and w*h RGBA8
 * words.  outTextureData must hold 4*count + sum(w*h) uints. */
typedef struct PTTextureDesc {
    const float* texels;  uint32_t width, height;  int32_t hasAlpha;  uint32_t _pad;
} PTTextureDesc;
PT_API int PTCopyTextureData(PTContext* ctx, const PTTextureDesc* textures, uint32_t count, uint32_t* outTextureData, uint64_t outUints);

/* The hipStream_t (as void*) all passes of this context are launched on. */
PT_API void* PTGetStream(PTContext* ctx);

/* Counters: level 0 = rays/paths only (always on, free), 1 = full PTStats (slower kernel variant). */
PT_API int PTSetStatsLevel(PTContext* ctx, int level);
PT_API int PTGetStats(PTContext* ctx, PTStats* out);
PT_API int PTResetStats(PTContext* ctx);
/* The mid-pass slot repack of the default schedule: passes over the context's own blocks, on frames large enough
 * for it, move the state of their live paths to the front of the state set a few times per pass, so that the shading waves stay
 * full.  Frames and PTStats do not depend on it.  Counted on the device since the context was created (PTResetStats leaves
 * them), read with the same ordering as PTGetStats. */
typedef struct PTRepackStats {
    uint64_t sequences;            /* launch sequences that had at least one repack candidate          */
    uint64_t candidates;           /* candidates: points of a sequence where the live slots are counted */
    uint64_t repacks;              /* candidates at which the state was moved                           */
    uint64_t slotsMoved;           /* live slots moved, summed over the repacks                         */
} PTRepackStats;
PT_API int PTGetRepackStats(PTContext* ctx, PTRepackStats* out);
/* The rule of a repack on the host (csrc/repack_rule.h), no GPU involved: flags = numSlots 32-bit state words (a slot is live
 * unless (word & 3) == 2; numSlots a multiple of 256), capacity = slots the temporary region holds, fill = fillNum / fillDen.
 * outPlan[3] = {1 if the set is repacked else 0, live slots L, extent E}; outDest (may be NULL): the slot every live slot moves
 * to (0xFFFFFFFF for a finished one).  Returns 1, or 0 for a NULL array, a numSlots that is no multiple of 256 or fillDen == 0. */
PT_API int PTRepackPlanHost(const uint32_t* flags, uint32_t numSlots, uint32_t capacity, uint32_t fillNum, uint32_t fillDen,
                            uint32_t* outPlan, uint32_t* outDest);

PT_API int PTSetProfiling(PTContext* ctx, int enabled);
PT_API int PTGetTimings(PTContext* ctx, PTTimings* out);
PT_API int PTResetTimings(PTContext* ctx);

/* Select the kernel schedule.  All schedules produce bit-identical frames and counters:
 *  -1  auto (default): 1, except for scenes whose BVH has <= 16 nodes (no traversal to speak of), which use 0
 *   0  megakernel: one lane per pixel, one launch per pass
 *   1  wavefront: slot-indexed path state, refill trace kernel + shade kernel, host-sync-free, passes overlap
 *   2  wavefront with the plain one-ray-per-lane trace kernel
 *   3  wavefront with the persistent dynamic-chunk trace kernel
 *   4  fused persistent wavefront: ONE launch per pass; a persistent wave owns 128 path contexts, alternates between tracing
 *      their rays and shading them, and hands a context whose pixel has finished the next pixel of the frame.  One path-state
 *      set of ~0.5 M contexts instead of one slot per pixel and pass in flight; the fastest schedule when passes are NOT
 *      pipelined (a host that presents every pass).  HAS_TLAS scenes run schedule 1's kernels. */
PT_API int PTSetSchedule(PTContext* ctx, int schedule);
/* The schedule (0..4) the next pass will run with the current scene: resolves -1 (auto).  Negative = error code. */
PT_API int PTGetSchedule(PTContext* ctx);
/* Wavefront schedules: number of trace+shade iterations launched per pass before the cleanup kernel finishes whatever is
 * still alive.  0 (default) = SamplesPerPass * (MaxRayBounces + 2) + 4.  Any value gives the same frame; it only moves
 * work between the wavefront kernels and the cleanup kernel (tuning / test knob). */
PT_API int PTSetWavefrontIterations(PTContext* ctx, int iterations);

/* Wavefront schedules: how many consecutive passes may be in flight at once, each on its own path-state set and HIP stream
 * (the pixel write of a pass is decoupled from its path loop, so pass k+1 traces while pass k drains; only the resolves are
 * ordered).  1 = passes run back to back (what a host that reads every frame back gets anyway).  0 (default) = sized to the
 * hardware queues the set streams get (streams that share a hardware queue serialise).  The HIP runtime pools the streams of a
 * process on GPU_MAX_HW_QUEUES queues (4 when unset); with a limit below 16 the set streams are created with a CU mask that
 * enables every CU (hipExtStreamCreateWithCUMask), which the runtime never pools, so every set has a queue of its own whatever
 * the host exported: 12.  Such a stream synchronises with the null stream.  With 16 or more, or where the
 * runtime refuses such a stream, the sets share the process's one pool: GPU_MAX_HW_QUEUES >= 16 -> 12, >= 8 -> 6, otherwise 3.
 * The library never changes the environment itself.  A number above what has its own queue is legal, and slower, not wrong.  Each set costs
 * ~290 B per owned pixel and is allocated on the first pass that can use it; lowering the number frees the sets no longer
 * used.  Same frame for every value. */
PT_API int PTSetPassesInFlight(PTContext* ctx, int passes);
PT_API int PTGetPassesInFlight(PTContext* ctx);
/* Wavefront schedules: cut every pass into `subFrames` (1 .. passes in flight) interleaved subsets of the context's 16x16 pixel
 * blocks, each rendered by its own launch sequence on its own state set and stream into the same output frame.  For a host that
 * consumes every frame before it asks for the next (the reference presents every pass, PathTracer.cs:251-272) this gives ONE
 * pass the overlap that otherwise only several passes in flight have.  Same frame for every value; 1 (default) = off. */
PT_API int PTSetSubFrames(PTContext* ctx, int subFrames);

/* =====================================================================================================================
 * Part 3: ray queries.  What does a ray hit in the scene of a context (PTSetScene)?  Picking, autofocus, line of sight,
 * visibility baking -- on the GPU, against the scene already resident there, with the render's own traversal code.
 *
 * Semantics (the shader's rules, util/bvh.hlsl and util/tlas.hlsl, not new ones):
 *  - Flat scene: hits are accepted for 1e-4 < t < tmax (util/bvh.hlsl:47).  The direction is NOT normalised: t is the ray
 *    parameter (origin + t * direction).  PT_QUERY_CLOSEST returns, bit for bit, the record of the render's closest-hit walk
 *    started at distance tmax (and of the CPU oracle's oracle_trace_uv).
 *  - The overflow rule of the traversal stacks, for the render and for every query alike.  Both stacks -- the CWBVH stack of a
 *    flat scene or of one instance, and the TLAS stack -- hold 32 entries.  A push at index >= 32 stores nothing but still
 *    advances the stack pointer.  A pop from an index >= 32 yields nothing and the walk pops again.  The walk ends when the
 *    pointer reaches 0 without having yielded an entry.  A ray whose TLAS walk dropped at least one entry adds 1 to
 *    PTStats.stackOverflows, once per ray, in addition to the 1 that each of its CWBVH walks (one per instance entered) adds
 *    when it dropped an entry.  What hung on a dropped entry is not visited: such a ray may miss geometry that it crosses.
 *    (The reference shader writes past a local array there, so there is no behaviour of its own to keep.)
 *  - HAS_TLAS scene (util/tlas.hlsl): the direction is normalised for the TLAS walk, triangles accept LOCAL parameters
 *    t > 0 (not 1e-4), and a closest hit's t is the WORLD-space distance length(position - origin); later instances compare
 *    their local parameters against it (the reference's quirk).  For a parametric t, pass unit directions.  An any-hit
 *    record's t is the parameter in the local space of the instance that was hit.
 *  - A ray whose tmax is NaN or <= 0 is a miss by definition: its record is {tmax, 0, 0, 0xFFFFFFFF}, written without a
 *    walk.  A ray with a NaN in its origin or direction misses (no walk either, as in the render).
 *  - A miss is {tmax, 0, 0, 0xFFFFFFFF}.  PT_QUERY_ANY_HIT (occlusion) stops at the first accepted triangle and reports that
 *    triangle's t, u, v, prim: prim != 0xFFFFFFFF <=> something lies between the near limit and tmax.
 *  - PT_QUERY_SURFACE (with closest hits only) also writes a PTRaySurface where a hit was found (elsewhere the array is
 *    left untouched): the shader's hit-attribute fetch (util/bvh.hlsl:201-212, util/tlas.hlsl:208-229).
 *  - Results go to hits[i] for rays[i]; rays are not reordered.
 * With PTSetStatsLevel(ctx, 1) a query adds to PTStats: closestHitRays or shadowRays (every ray of the batch), nodeVisits,
 * triTests, attrFetches, maxStackDepth, stackOverflows, tlasNodeVisits, instanceVisits -- the render's definitions.  At level
 * 0 a query counts nothing.
 * Errors: PT_ERR_INVALID_ARG for a NULL context or required pointer, an unknown flag bit, SURFACE together with ANY_HIT, and
 * (PTTraceRaysHost) a nonzero `reserved` word; PT_ERR_NO_SCENE before PTSetScene.  count == 0 returns PT_OK and launches
 * nothing.  There is no CPU fallback.
 * ===================================================================================================================== */
typedef struct PTRay {            /* 32 bytes: the layout of the oracle's n x 8 float rays */
    float    origin[3];
    float    direction[3];        /* need not be unit length */
    float    tmax;                /* hits are accepted for t < tmax; PT_FAR_PLANE = "unbounded" */
    uint32_t reserved;            /* must be 0 (PTTraceRaysHost checks it; the device path ignores it) */
} PTRay;

typedef struct PTRayHit {         /* 16 bytes */
    float    t;                   /* hit distance; tmax on a miss */
    float    u, v;                /* barycentrics; 0, 0 on a miss */
    uint32_t prim;                /* the TriangleAttributes index of the hit; 0xFFFFFFFF on a miss */
} PTRayHit;

typedef struct PTRaySurface {     /* 48 bytes, written only where a closest hit was found */
    float    position[3]; float    t;
    float    normal[3];   int32_t  materialIndex;  /* interpolated shading normal (unit length), not face-forwarded */
    float    uv[2];       uint32_t instance;       /* HAS_TLAS: the instance that owns the hit; else 0xFFFFFFFF */
                          uint32_t prim;
} PTRaySurface;

#ifdef __cplusplus
static_assert(sizeof(PTRay) == 32, "PTRay is 32 bytes");
static_assert(sizeof(PTRayHit) == 16, "PTRayHit is 16 bytes");
static_assert(sizeof(PTRaySurface) == 48, "PTRaySurface is 48 bytes");
#else
_Static_assert(sizeof(PTRay) == 32, "PTRay is 32 bytes");
_Static_assert(sizeof(PTRayHit) == 16, "PTRayHit is 16 bytes");
_Static_assert(sizeof(PTRaySurface) == 48, "PTRaySurface is 48 bytes");
#endif

#define PT_QUERY_CLOSEST  0u
#define PT_QUERY_ANY_HIT  1u      /* occlusion: stop at the first accepted triangle */
#define PT_QUERY_SURFACE  2u      /* with CLOSEST only: also fill PTRaySurface */

/* Device pointers, stream-ordered on the context's stream (PTGetStream); returns before the rays are traced.
 * Any count: batches of more than 2^28 rays are split into several launches. */
PT_API int PTTraceRays(PTContext* ctx, const PTRay* dRays, uint64_t count, uint32_t flags,
                       PTRayHit* dHits, PTRaySurface* dSurface /* NULL unless PT_QUERY_SURFACE */);
/* Host arrays (a C# host via [DllImport]): staged through device buffers the context keeps and grows; synchronous. */
PT_API int PTTraceRaysHost(PTContext* ctx, const PTRay* rays, uint64_t count, uint32_t flags,
                           PTRayHit* hits, PTRaySurface* surface);

/* =====================================================================================================================
 * Part 4: guide buffers and denoising.  First-hit guides (albedo, normal, depth) rendered on the GPU with the render's own
 * traversal, and an edge-avoiding a-trous filter (SVGF's spatial half) that runs between the Output frame and PTPresent.
 *
 * Guides (PTRenderGuides), for every pixel (x, y) of params' OutputWidth x OutputHeight, with S samples and n = sqrt(S):
 *  - Sample (i, j), taken in the order j = 0..n-1, i = 0..n-1 (i fastest), is the pinhole ray through
 *    (x + (i + 0.5) / n, y + (j + 0.5) / n): generate_camera_ray's arithmetic on CamInvProj / CamToWorld with the jitter
 *    removed (every offset is exact in float32; for S = 1 it is the ray through the pixel centre).  Aperture, FocalLength,
 *    the seeds and DispatchGroups are ignored: no thin lens.  Each sample is a closest-hit walk with tmax = PT_FAR_PLANE,
 *    the same as PTTraceRays(PT_QUERY_CLOSEST | PT_QUERY_SURFACE).  Flat and HAS_TLAS scenes.
 *  - Albedo guide: rgb = the material's base colour after texturing (GetBaseColorOpacity, as the render's material fetch
 *    computes it), summed in float32 in sample order starting from 0, a missing sample contributing (1, 1, 1), then divided
 *    by S.  w = (hitting samples) / S: the coverage mask, 0 = background.
 *  - Normal + depth guide: xyz = the interpolated shading normal of the hitting samples (PTRaySurface.normal): with one
 *    hitting sample that normal as it is, with more their float32 sum in sample order normalised with the device's
 *    normalize3 (0 if the sum vanishes); 0 where nothing hit.  w = the mean hit distance over the hitting samples (their
 *    sum in sample order divided by their count), 0 where nothing hit.
 *  - The guides ignore opacity and alpha cutouts and do not see the visible analytic lights.
 *  - Guides count nothing in PTStats and are not part of PTGetTimings.
 *
 * Filter (PTDenoise): DESIGN.md 5.9 gives the exact formula.  Pixels with coverage 0 pass through bit for bit and are never
 * taps; iterations == 0 returns the input's bits; out.a is always the input's alpha.
 *
 * Memory: guide and filter buffers belong to the context, are allocated on first use, regrown when the size changes and
 * freed by PTDestroy.  A context that never calls these functions allocates nothing for them.
 * Errors: PT_ERR_INVALID_ARG for a NULL context or required pointer, samplesPerPixel not 1, 4 or 16, iterations outside
 * 0..8, a sigma that is NaN or <= 0, an unknown flag bit, a structSize below sizeof(PTDenoiseParams) of this header, and
 * PTDenoise without guides or with guides of another size than the frame; PT_ERR_NO_SCENE for PTRenderGuides before
 * PTSetScene.  There is no CPU fallback.
 * ===================================================================================================================== */
#define PT_DENOISE_DEMODULATE_ALBEDO 0x1u   /* filter colour / max(albedo, 1e-3), multiply back afterwards */

typedef struct PTDenoiseParams {  /* 24 bytes; versioned like PTFrameParams: min(structSize, sizeof) read, rest zero */
    uint32_t structSize;          /* = sizeof(PTDenoiseParams) of the host's header */
    int32_t  iterations;          /* a-trous levels 0..8 (steps 1, 2, 4, ...); suggested 5 */
    float    sigmaLuminance;      /* suggested 4 */
    float    sigmaNormal;         /* exponent of the normal weight; suggested 128 */
    float    sigmaDepth;          /* suggested 1 */
    uint32_t flags;               /* PT_DENOISE_DEMODULATE_ALBEDO; suggested on */
} PTDenoiseParams;

#ifdef __cplusplus
static_assert(sizeof(PTDenoiseParams) == 24, "PTDenoiseParams is 24 bytes");
#else
_Static_assert(sizeof(PTDenoiseParams) == 24, "PTDenoiseParams is 24 bytes");
#endif

/* First-hit guides for the camera of `params` (its size, CamInvProj, CamToWorld); samplesPerPixel is 1, 4 or 16.
 * Stream-ordered on the context's stream; returns before the guides are written. */
PT_API int PTRenderGuides(PTContext* ctx, const PTFrameParams* params, int samplesPerPixel);
/* dDst = denoise(dSrc), both DEVICE pointers to guide-size float4 frames; dSrc == NULL reads the current Output frame (which
 * must then have the guides' size) and is never written unless it is dDst; dSrc == dDst is allowed.  Stream-ordered after
 * every pass launched so far, the same as PTPresent. */
PT_API int PTDenoise(PTContext* ctx, const PTDenoiseParams* params, const void* dSrc, void* dDst);
/* Denoises the current Output frame into host memory (width*height float4); synchronous. */
PT_API int PTDenoiseToHost(PTContext* ctx, const PTDenoiseParams* params, float* dstRGBA, uint64_t dstFloats);
/* Device pointer of guide `which`: 0 albedo + coverage, 1 normal + depth (width*height float4 each); NULL before the first
 * PTRenderGuides or for another `which`.  A host may write its own guides there before PTDenoise. */
PT_API void* PTGetGuidePointer(PTContext* ctx, int which);

/* =====================================================================================================================
 * Part 5: scene updates.  Move instances, lights and materials of the scene PTSetScene uploaded, without setting it again
 * (the reference's BVHScene.UpdateTLAS, PathTracer.UpdateLights / UpdateMaterialData).
 *
 * Instances: `count` PTBlasInstance records (the 192-byte input of BuildTLAS); count must equal the scene's instanceCount.
 * localToWorld, worldToLocal, aabbMin and aabbMax are read; blasIndex is ignored as in BuildTLAS; the BLAS offsets and
 * materialIndex stay as PTSetScene set them.  The TLAS is rebuilt on the GPU, byte-identical to BuildTLAS of the same
 * records (PTReadTLAS returns it), and the frames, ray queries and guides equal those of a fresh PTSetScene.  The host
 * variant refuses non-finite AABBs and matrices; the device variant does not look at the data: such input gives an
 * unspecified tree that is still memory-safe.
 * Lights: 1..lightCount (of PTSetScene) PTLight records, 64 bytes; the scene must have HAS_LIGHTS.
 * Materials: materialCount PTMaterialData records, 128 bytes; a texture slot is negative (none) or names a texture that
 * PTSetScene validated.
 * Ordering: passes, queries and guides enqueued before an update see the old scene, everything enqueued after sees the new
 * one.  Updates never block the host for the GPU; the host variants copy the caller's array before they return (they may
 * wait for their own staging buffer).  PTUpdateInstancesDevice reads dInstances in the context stream's order.
 * The library does not reset accumulation: call PTResetFrames / start again at CurrentSample = 0.
 * Memory: allocated on the first update of each kind (two generations of what changes); PTSetScene discards the update
 * state and PTDestroy frees it.
 * Errors: PT_ERR_INVALID_ARG for a NULL context or array, a count mismatch, a refused record; PT_ERR_NO_SCENE before
 * PTSetScene; PT_ERR_UNSUPPORTED for instance updates without HAS_TLAS and light updates without HAS_LIGHTS.
 * ===================================================================================================================== */
PT_API int PTUpdateInstances(PTContext* ctx, const PTBlasInstance* instances, uint32_t count);          /* host array, copied before return */
PT_API int PTUpdateInstancesDevice(PTContext* ctx, const PTBlasInstance* dInstances, uint32_t count);   /* device array, read in stream order */
PT_API int PTUpdateLights(PTContext* ctx, const void* lights, uint32_t count);                          /* PTLight records, 64 B */
PT_API int PTUpdateMaterials(PTContext* ctx, const void* materials, uint32_t count);                    /* PTMaterialData records, 128 B */
/* The current TLAS in BuildTLAS's layout: *outNodeCount nodes (64 bytes each) into dstNodes and instanceCount indices into
 * dstIndices.  Synchronising.  Before any instance update it returns what PTSetScene was given. */
PT_API int PTReadTLAS(PTContext* ctx, void* dstNodes, uint64_t dstNodeBytes, uint32_t* dstIndices, uint64_t dstIndexCount,
                      uint32_t* outNodeCount);

/* =====================================================================================================================
 * Part 6: per-pixel variance across passes.  How far is the running mean from converged?  The accumulation already carries
 * the answer: after a pass Output and AccumulatedOutput are the running mean after and before m new samples, and by Welford's
 * update identity their difference is the term that advances the per-pixel sum of squared deviations.  No render kernel is
 * touched; the view is static; the only history is the running mean the reference itself keeps.
 *
 * Moments (PTAccumulateMoments[To]): one call records ONE observation -- the `count` passes (1..8) that PTRenderPass[To] or
 * PTRenderPassBatch[To] just enqueued with these params (a batch is one observation: its intermediate frames do not exist).
 * n = params[0].CurrentSample, m = count * max(1, SamplesPerPass).
 *  - n == 0: both planes are written with zeros, Acc is not read; observations = 1, samples = m.
 *  - n > 0: n must equal the stored sample count and the size the stored size.  Per pixel, in float32, every operation one
 *    IEEE operation in this order (no contraction):
 *        f  = (float)((double)n * (double)(n + m) / (double)m)                     (host)
 *        d  = Out.rgb - Acc.rgb;  dl = 0.2126f*d.r + 0.7152f*d.g + 0.0722f*d.b
 *        plane0 += ((d.r*d.r)*f, (d.g*d.g)*f, (d.b*d.b)*f, (dl*dl)*f)               Srr Sgg Sbb Sll
 *        plane1 += ((d.r*d.g)*f, (d.r*d.b)*f, (d.g*d.b)*f, 0)                       Srg Srb Sgb
 *    then observations += 1, samples = n + m, and Out becomes "the frame last accumulated".
 *  With k observations of W samples in all, S / ((k - 1) * W) estimates the variance of the running mean (invDof below).
 *  Ordering: enqueued on the context stream -- after the resolve of the passes it describes, before the resolve of any later
 *  pass (which overwrites Acc's buffer); the trace chains of passes in flight do not wait for it.  Call it after the pass and
 *  before PTFlipFrames.
 *
 * Noise (PTMeasureNoise; needs observations k >= 2), per pixel of the blocks this context owns (PTSetTileOwnership), float32:
 *        invDof = (float)(1.0 / ((double)(k - 1) * (double)W))                     (host)
 *        l   = 0.2126f*r + 0.7152f*g + 0.0722f*b                                    of dFrame.rgb
 *        eps = sqrtf(Sll * invDof) / (l + relFloor)          relative standard error of the mean; NaN or negative -> +inf
 *        bin = clamp((int)(bits(eps) >> 20) - ((127 - 24) << 3), 0, 255)            eighth-octave bins from 2^-24 to 2^8
 *  pixels = pixels counted, pixelsBelow = those with eps <= threshold, maxError / meanError = maximum / mean of eps,
 *  percentileError = the upper edge of the first bin at which the cumulative count reaches ceil(percentile * pixels)
 *  (+inf for bin 255; 0 when pixels == 0).  The tile map holds the mean eps of every 16x16 block, 0 for blocks of other
 *  ranks; a multi-rank host adds the integer fields of its ranks.  Two calls on the same data return the same bytes (integer
 *  atomics and ordered sums only).
 *
 * Denoising led by that variance (PTDenoiseMoments): PTDenoise with one change -- the prepass's v at a covered pixel is the
 * variance of the mean of the filter luminance instead of the 3x3 spatial variance:
 *        not demodulated:  v = Sll * invDof
 *        demodulated:      q_c = w_c / max(albedo_c, 1e-3), w = (0.2126, 0.7152, 0.0722),
 *                          v = max(0, (q_r^2 Srr + q_g^2 Sgg + q_b^2 Sbb + 2 (q_r q_g Srg + q_r q_b Srb + q_g q_b Sgb)) * invDof)
 *  so a converged frame is left alone.  Needs guides of the moments' size and observations >= 2.
 *
 * Memory: allocated on first use, regrown on a size change, freed by PTDestroy; a context that never calls these functions
 * allocates nothing for them.
 * Errors: PT_ERR_INVALID_ARG for a NULL context or required pointer, count outside 1..8, n != the stored sample count or
 * another size (the message names both numbers), relFloor or threshold not > 0, percentile outside (0, 1], fewer than 2
 * observations, a short structSize.  There is no CPU fallback.
 * ===================================================================================================================== */
typedef struct PTNoiseParams {    /* 16 bytes */
    uint32_t structSize;          /* = sizeof(PTNoiseParams) of the host's header */
    float    relFloor;            /* added to the luminance in the denominator; suggested 0.01 */
    float    threshold;           /* pixelsBelow counts eps <= threshold; suggested 0.02 */
    float    percentile;          /* in (0, 1]; suggested 0.95 */
} PTNoiseParams;

typedef struct PTNoiseStats {     /* 1072 bytes */
    uint32_t structSize;          /* in: sizeof(PTNoiseStats) of the host's header */
    uint32_t observations;
    uint64_t samples;
    uint64_t pixels;
    uint64_t pixelsBelow;
    float    meanError, maxError, percentileError;
    uint32_t _pad;
    uint32_t histogram[256];
} PTNoiseStats;

#ifdef __cplusplus
static_assert(sizeof(PTNoiseParams) == 16, "PTNoiseParams is 16 bytes");
static_assert(sizeof(PTNoiseStats) == 1072, "PTNoiseStats is 1072 bytes");
#else
_Static_assert(sizeof(PTNoiseParams) == 16, "PTNoiseParams is 16 bytes");
_Static_assert(sizeof(PTNoiseStats) == 1072, "PTNoiseStats is 1072 bytes");
#endif

/* Out = frame[cur], Acc = frame[1 - cur] of the context's own frames: call after the pass, before PTFlipFrames. */
PT_API int PTAccumulateMoments(PTContext* ctx, const PTFrameParams* params, int count);
/* The same over caller-owned DEVICE frames (dAccumulated may be NULL when CurrentSample == 0). */
PT_API int PTAccumulateMomentsTo(PTContext* ctx, const PTFrameParams* params, int count, const void* dOutput, const void* dAccumulated);
/* Any of the four outputs may be NULL.  Before the first accumulation everything is 0. */
PT_API int PTGetMomentsInfo(PTContext* ctx, uint32_t* observations, uint64_t* samples, uint32_t* width, uint32_t* height);
/* Device pointer of plane 0 (Srr Sgg Sbb Sll) or 1 (Srg Srb Sgb 0): width*height float4 each; NULL before first use. */
PT_API void* PTGetMomentsPointer(PTContext* ctx, int which);
/* dFrame: DEVICE pointer to the frame whose luminance is the denominator; NULL = the frame last accumulated.  Synchronous. */
PT_API int PTMeasureNoise(PTContext* ctx, const PTNoiseParams* params, const void* dFrame, PTNoiseStats* out);
/* ceil(W/16) * ceil(H/16) floats, row-major: the mean eps of each 16x16 block after PTMeasureNoise; NULL before. */
PT_API void* PTGetNoiseTilePointer(PTContext* ctx);
/* PTDenoise with the moments' variance; dSrc == NULL reads the frame last accumulated. */
PT_API int PTDenoiseMoments(PTContext* ctx, const PTDenoiseParams* params, const void* dSrc, void* dDst);
/* Denoises the frame last accumulated into host memory (width*height float4); synchronous. */
PT_API int PTDenoiseMomentsToHost(PTContext* ctx, const PTDenoiseParams* params, float* dstRGBA, uint64_t dstFloats);

/* =====================================================================================================================
 * Part 7: adaptive sampling.  Passes over the ACTIVE 16x16 blocks of the frame only, every block with its own sample count.
 * The stop criterion of Part 6 is global: the host pays for every pixel until the worst ones are good enough.  Here the
 * blocks that still are noisy (the tile map of PTMeasureNoise) -- or any explicit list: a region of interest -- are
 * rendered on, the rest of the frame moves on unchanged.
 *
 * A block is a 16x16 tile of the frame; its id is by * ceil(W/16) + bx, the indexing of the noise tile map.  The adaptive
 * state holds one sample count n_b per block, on the host side of the context (allocated by PTAdaptiveBegin, dropped by
 * PTAdaptiveEnd and PTDestroy; a context that never calls this part allocates nothing).
 *
 * The contract (bit-exact): PTRenderPassActive[To] renders `count` passes (1..8) of spp = max(1, SamplesPerPass) samples
 * over the active blocks.  For an active block b and pass j, cs = n_b + j * spp, and every pixel of b is computed exactly as
 * PTRenderPassTo computes it with CurrentSample = cs and RngSeedRoot = params[j].RngSeedRoot (the seed of a pixel is
 * pixelIndex * (cs + 1) + seedRoot; the running mean (color + acc * cs) / (cs + spp), or color / spp when cs == 0), the
 * passes applied in order, the intermediate frames never stored.  params[j].CurrentSample is not read.  Afterwards
 * n_b += count * spp.  Every pixel that is not in an active block, not in a block this context owns (PTSetTileOwnership) or
 * outside the dispatch coverage gets Output = Accumulated, bit for bit -- so ping-pong and PTFlipFrames work as before.
 *  (a) every block active and all n_b equal: the frame of PTRenderPassBatch on the same params, bit for bit;
 *  (b) in general: a per-block composite of the frames PTRenderPassTo gives for each distinct cs.
 * Ordering and PTStats as for PTRenderPassBatchTo (one launch sequence on the next state set; passes in flight overlap):
 * paths = active covered pixels x spp x count; the copy of the inactive pixels is not counted.  Sub-frames are not applied.
 * An empty list enqueues only the copy.  dOutput == dAccumulated is refused; dAccumulated may be NULL only when every block is
 * active and every n_b is 0.  Schedules 1, 2 and 3 (flat and HAS_TLAS); schedules 0 and 4 return PT_ERR_UNSUPPORTED.
 *
 * Moments: when PTAdaptiveBegin finds moments (Part 6) of the frame's size with samples == currentSample, every block
 * starts with the global (k, W) and PTAccumulateMomentsActive[To] records ONE observation of the adaptive call just
 * enqueued: the update of PTAccumulateMoments over that call's blocks, with f_b = (float)((double)n_b * (double)(n_b + m)
 * / (double)m) per block (n_b before the call, m = count * spp), then k_b += 1, W_b += m.  An inactive pixel has
 * Out - Acc == 0, so skipping it is exact.  While such state is live PTMeasureNoise, PTDenoiseMoments and
 * PTDenoiseMomentsToHost use invDof_b = (float)(1.0 / ((double)(k_b - 1) * (double)W_b)) per block, PTNoiseStats.observations
 * / samples (and PTGetMomentsInfo) report the minimum over the blocks this context owns, and PTAccumulateMoments (the global
 * one) is refused.  Without moments at PTAdaptiveBegin the render calls work and the moments calls fail.
 *
 * Errors: PT_ERR_INVALID_ARG, with the offending numbers in PTGetLastError, for a call without PTAdaptiveBegin, params of
 * another frame size, ids not strictly ascending or out of range, count outside 1..8, n_b + m past 2^32,
 * PTAccumulateMoments while adaptive state is live, a short structSize.  Invalid input is refused before any launch.
 * ===================================================================================================================== */
typedef struct PTAdaptiveSelect {   /* 20 bytes */
    uint32_t structSize;            /* = sizeof(PTAdaptiveSelect) of the host's header */
    float    threshold;             /* a block is selected when its tile mean eps > threshold ... */
    uint32_t maxSamples;            /* ... and n_b + addSamples <= maxSamples */
    uint32_t addSamples;            /* what the next adaptive call will add per block (count * spp) */
    uint32_t dilate;                /* 0 or 1: also the up to eight neighbours of a selected block that meet the sample limit */
} PTAdaptiveSelect;

#ifdef __cplusplus
static_assert(sizeof(PTAdaptiveSelect) == 20, "PTAdaptiveSelect is 20 bytes");
#else
_Static_assert(sizeof(PTAdaptiveSelect) == 20, "PTAdaptiveSelect is 20 bytes");
#endif

/* Every block of the OutputWidth x OutputHeight frame of `params` holds currentSample samples; every block active. */
PT_API int PTAdaptiveBegin(PTContext* ctx, const PTFrameParams* params, uint32_t currentSample);
PT_API int PTAdaptiveEnd(PTContext* ctx);
/* Strictly ascending block ids; NULL with count 0 = every block (a non-NULL pointer with count 0 = none).  Blocks of other
 * ranks and blocks without a covered pixel are dropped silently; *kept (may be NULL) = how many remain. */
PT_API int PTSetActiveBlocks(PTContext* ctx, const uint32_t* blocks, uint32_t count, uint32_t* kept);
/* Selects on the host from the tile map of the last PTMeasureNoise (read back: synchronous) and the sample counts. */
PT_API int PTSelectActiveBlocks(PTContext* ctx, const PTAdaptiveSelect* select, uint32_t* kept);
/* The blocks the next adaptive call renders, ascending; dst may be NULL to ask for *count only. */
PT_API int PTGetActiveBlocks(PTContext* ctx, uint32_t* dst, uint32_t capacity, uint32_t* count);
/* n_b of every block of the frame, row-major: ceil(W/16) * ceil(H/16) values. */
PT_API int PTGetBlockSamples(PTContext* ctx, uint32_t* dst, uint64_t capacity);
/* params: an array of `count` PTFrameParams as for PTRenderPassBatchTo (may differ in RngSeedRoot only; CurrentSample ignored). */
PT_API int PTRenderPassActive(PTContext* ctx, const PTFrameParams* params, int count);
PT_API int PTRenderPassActiveTo(PTContext* ctx, const PTFrameParams* params, int count, void* dOutput, const void* dAccumulated);
/* One observation for the blocks of the adaptive call just enqueued (same params[0] and count); before PTFlipFrames. */
PT_API int PTAccumulateMomentsActive(PTContext* ctx, const PTFrameParams* params, int count);
PT_API int PTAccumulateMomentsActiveTo(PTContext* ctx, const PTFrameParams* params, int count, const void* dOutput, const void* dAccumulated);

/* =====================================================================================================================
 * Part 8: radiance queries.  How much light arrives along a ray?  Part 3 says what a ray hits; radiance so far exists only for
 * the pixels of one camera (PTRenderPass*).  Here the host hands the path tracer a LIST of rays -- light and reflection
 * probes, lightmap texels with host-made gather directions, sensor simulation, scattered pixels, ray batches across many
 * cameras -- and gets the path-traced radiance of each, computed by the render's own code.  The reference has nothing like
 * it: an addition beside its ABI, like Parts 3 to 7.
 *
 * The contract of PTTraceRadiance (bit-exact):
 *  - Entry i runs n = max(SamplesPerPass, 1) samples.  Sample 0 starts in the state the render's path_init leaves --
 *    sample index 0, colour 0, no pending NEE -- with RNG state rays[i].rng and the entry's origin and direction as the
 *    first ray; the direction is used as given, never re-normalised.  Every later sample restarts from the SAME ray with the
 *    RNG continuing where the previous sample left it (what the render does at the end of a sample, with the camera drawing
 *    nothing).  Everything from there on is the render's code in the render's order: the path step, the firefly filter,
 *    Russian roulette and MaxRayBounces of `params`, the environment mode, lights, textures, HAS_TLAS.
 *  - out[i].rgb = colour / (float)n, the expression of the render's pixel write for CurrentSample == 0 (one fp32 division
 *    per channel); out[i].rng = the RNG state after the last draw.  Feeding it back as rays[i].rng continues the chain:
 *    one call with n samples equals n calls with one sample each, their colours summed in order and divided by (float)n.
 *  - Results are in the caller's order; nothing past `count` is written.
 *  - Not read from PTFrameParams: CamInvProj, CamToWorld, OutputWidth, OutputHeight, CurrentSample, RngSeedRoot, Aperture,
 *    FocalLength, DispatchGroupsX / Y.  The struct is still validated as for a pass (structSize, a non-empty frame size).
 *  - A NaN in an origin or direction behaves as in the render: no walk, the sky.  A direction that is not of unit length is
 *    the caller's error: some finite or NaN colour, never an out-of-bounds access.
 *  - Stream-ordered on the context's stream, like PTTraceRays: the call returns before anything is traced, dRays is read
 *    after everything enqueued on that stream so far, and must stay valid until the call has run (samples after the first
 *    re-read it).  dRays and dOut are 16-byte aligned.  Calls take the context's state sets round-robin exactly as passes do
 *    (PTSetPassesInFlight); each call's output is its own (no ordering between resolves).
 *  - A list of more than 2^21 entries is cut into chunks of 2^21, each a launch sequence on the next state set: a state set
 *    never grows beyond what a 1080p frame needs, and the chunks of one call overlap like passes in flight.  Two calls do not
 *    overlap (the second one's rays are ordered after the first one's results): one long list beats many short ones.
 *  - PTStats (at the level set): paths = count x n; every ray, node, triangle, fetch and TLAS counter by the render's
 *    definitions; pixelsWritten and pixelsRead do not move.  With profiling on, every chunk is one entry of PTGetTimings.
 *  - Schedules 1, 2 and 3, flat and HAS_TLAS scenes; schedules 0 and 4 return PT_ERR_UNSUPPORTED (PTSetSchedule; note that
 *    the automatic schedule of a scene with a handful of BVH nodes is 0).  PT_ERR_UNSUPPORTED also for SamplesPerPass > 4095
 *    or MaxRayBounces > 8191.  count == 0 returns PT_OK and launches nothing.  PT_ERR_INVALID_ARG for a NULL context or
 *    pointer, a misaligned pointer and (PTTraceRadianceHost) a nonzero `reserved` word; PT_ERR_NO_SCENE before PTSetScene.
 *    There is no CPU fallback.
 *
 * The contract of PTCameraRays: for pixel index k = py * OutputWidth + px the entry is what the render's path_init makes of
 * that pixel: the RNG is seeded with k * (CurrentSample + 1) + RngSeedRoot, the camera ray is generated (two draws; four with
 * Aperture > 0 and FocalLength > 0), and the entry holds that ray's origin and direction and the RNG state AFTER the draws.
 * dPixelIndices == NULL: entry i is pixel i, and count > OutputWidth * OutputHeight is PT_ERR_INVALID_ARG.  In a device list
 * an index >= OutputWidth * OutputHeight yields an entry with a NaN direction and rng = 0 (never an out-of-range read).
 * Stream-ordered on the context's stream; needs no scene.
 *
 * Together: PTCameraRays followed by PTTraceRadiance with SamplesPerPass = 1 gives, bit for bit, the rgb PTRenderPassTo
 * writes for those pixels with SamplesPerPass = 1 and CurrentSample = 0.
 * ===================================================================================================================== */
typedef struct PTRadianceRay {    /* 32 bytes */
    float    origin[3];
    float    direction[3];        /* unit length; used as given, never re-normalised */
    uint32_t rng;                 /* RNG state the path starts with */
    uint32_t reserved;            /* must be 0 (PTTraceRadianceHost checks it; the device path ignores it) */
} PTRadianceRay;

typedef struct PTRadiance {       /* 16 bytes */
    float    rgb[3];              /* mean over the samples: sum / (float)n */
    uint32_t rng;                 /* RNG state after the last sample */
} PTRadiance;

#ifdef __cplusplus
static_assert(sizeof(PTRadianceRay) == 32, "PTRadianceRay is 32 bytes");
static_assert(sizeof(PTRadiance) == 16, "PTRadiance is 16 bytes");
#else
_Static_assert(sizeof(PTRadianceRay) == 32, "PTRadianceRay is 32 bytes");
_Static_assert(sizeof(PTRadiance) == 16, "PTRadiance is 16 bytes");
#endif

/* Device pointers, stream-ordered on the context's stream; dPixelIndices == NULL = every pixel in index order. */
PT_API int PTCameraRays(PTContext* ctx, const PTFrameParams* params, const uint32_t* dPixelIndices, uint64_t count, PTRadianceRay* dRays);
PT_API int PTTraceRadiance(PTContext* ctx, const PTFrameParams* params, const PTRadianceRay* dRays, uint64_t count, PTRadiance* dOut);
/* Host arrays: staged through device buffers the context keeps and grows; synchronous. */
PT_API int PTTraceRadianceHost(PTContext* ctx, const PTFrameParams* params, const PTRadianceRay* rays, uint64_t count, PTRadiance* out);

/* =====================================================================================================================
 * Part 9: geometry updates.  New vertex positions for one BLAS of the scene PTSetScene uploaded (skinning, cloth, a morph),
 * without rebuilding or setting the scene again: the CWBVH is REFITTED on the GPU.
 *
 * The rule.  A refit keeps the topology: row n1 of every node (childBaseIndex, triBaseIndex, meta[8]), imask, the order of
 * the triangle records and their primIdx, all counts.  It rewrites every triangle record (e2 = v[3p+2] - v[3p], e1 = v[3p+1] -
 * v[3p], v0 = v[3p] for p = primIdx; the bytes BuildBVH writes) and every node's lo, exponents and 48 quantised bytes.  A leaf
 * slot's box is the box of the original vertices of its popcount(meta >> 5) records from record (meta & 31) of triBaseIndex; an
 * inner slot's box is the refitted box of that child; a node's box is the fold over its occupied slots in ascending order,
 * all with compare-and-select (b < acc ? b : acc).  The encode is PTBuildBVHDevice's: per axis the smallest e in -120 ... 126
 * with 255 * 2^e >= extent, q_lo = clamp(floor((c.mn - lo) / 2^e)), q_hi = clamp(ceil((c.mx - lo) / 2^e)) into 0 ... 255, empty
 * slots 0.  Every step is exact or correctly rounded: PTReadGeometry after an update equals PTRefitBVH of the same tree and
 * vertices byte for byte, and frames, queries and guides equal those of a fresh PTSetScene of the refitted arrays.  The tree's
 * quality is the caller's to watch: a refit of a strongly deformed mesh traverses more nodes than a rebuild;
 * Part 10 measures it (PTMeasureGeometry) and rebuilds in place (PTRebuildGeometry).
 *
 * The BLAS is named by the three offsets of its PTGpuInstance records: bvhOffset (nodes), triOffset (float4s),
 * triAttributeOffset (triangles); 0, 0, 0 for a scene without HAS_TLAS.  vertices: 3 * triangleCount PTFloat4 in the BLAS's
 * primitive order (BuildBVH's input order), w ignored.  attrs: NULL keeps the attribute records, otherwise triangleCount
 * records replace the BLAS's (new normals and tangents).  The host variant copies both arrays before it returns and refuses
 * non-finite vertices and, without HAS_TLAS, a materialIndex >= materialCount.  The device variant reads them in the context
 * stream's order and does not look at the vertices: non-finite ones give an unspecified tree that is still memory-safe, since
 * no index is rewritten; a device record whose materialIndex is out of range keeps the index it had.
 * HAS_TLAS: the library does not touch the TLAS.  The world bounds of the instances of a deformed BLAS are the caller's to
 * resend through PTUpdateInstances -- the caller has the vertices.
 * The first update of a scene reads the node and triangle buffers back once (synchronising) and the first update of a BLAS
 * walks it as PTSetScene's validation does; PTSetScene itself does nothing for this part.
 * Ordering, accumulation, memory and lifetime are Part 5's: work enqueued before the call sees the old geometry, work enqueued
 * after it the new; two generations of nodes + triangles (and of the attributes, once they are given), allocated on the first
 * update, the current one copied into the other by every update; PTSetScene discards the state, PTDestroy frees it.
 * Instances may share a BLAS only whole (the same three offsets): a BLAS whose root or first record lies inside another one's
 * is refused; BLASes that overlap in any other way are the caller's to avoid -- a refit of one changes the other.
 * Errors: PT_ERR_NO_SCENE before PTSetScene; PT_ERR_INVALID_ARG for a NULL context or array, offsets that name no BLAS, a
 * triangleCount that is not the BLAS's, a refused array.
 * PTReadGeometry: the current node, triangle and (dstAttrs != NULL) attribute buffers of the whole scene, in PTSetScene's
 * layout and sizes.  Synchronising.  Before any geometry update it returns what PTSetScene was given.
 * ===================================================================================================================== */
PT_API int PTUpdateGeometry(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* vertices,
                            int triangleCount, const PTTriangleAttributes* attrsOrNull);                  /* host arrays, copied before return */
PT_API int PTUpdateGeometryDevice(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* dVertices,
                                  int triangleCount, const PTTriangleAttributes* dAttrsOrNull);           /* device arrays, read in stream order */
PT_API int PTReadGeometry(PTContext* ctx, void* dstNodes, uint64_t nodeBytes, void* dstTris, uint64_t triBytes, void* dstAttrs, uint64_t attrBytes);

/* =====================================================================================================================
 * Part 10: geometry rebuilds and tree quality.  Part 9 keeps the topology; a pose that has drifted far from the one the tree was
 * built for is traversed through ever looser boxes.  PTRebuildGeometry builds a NEW tree for the BLAS, in
 * place, on the GPU: PTBuildBVHDevice's builder runs on the update stream, from vertices on the device, straight into the
 * generation that is not current -- no node or triangle read-back, no PTSetScene.  PTMeasureGeometry tells the host when.
 *
 * Rebuild.  The arguments, ordering, generations, carry-over, attribute handling, the TLAS rule (the instances' world bounds are
 * the caller's to resend), lifetime and errors are Part 9's: accumulation is not reset, PTSetScene discards everything,
 * PTDestroy frees it.  The result is the tree of PTBuildBVHDevice's rule for these vertices, built at bvhOffset / triOffset of the
 * target generation after the carry-over copy (node and row indices inside a BLAS are relative to its offsets).  All
 * 3 * triangleCount triangle rows are rewritten; primIdx stays the caller's primitive order, so the attribute records still
 * match.  Node numbering within the tree is the builder's (atomic allocation, level by level) and may differ from call to call.
 * Node capacity.  The new tree's node count K generally differs from the old one's.  A BLAS's capacity is its node span in the
 * scene PTSetScene was given: from bvhOffset to the next larger distinct bvhOffset among the instances, or to the end of the
 * node buffer (a scene without HAS_TLAS: the whole buffer).  PTSetScene's validation only follows what a ray can reach, so a
 * host that plans to rebuild pads the span with unreferenced (zero) nodes.  K <= capacity: the K nodes are written and nodes
 * K ... capacity - 1 of the span are zero-filled.  K > capacity: PT_ERR_INVALID_ARG, the message names K and the capacity;
 * nothing is ever written outside the span, no buffer grows, no offset moves.
 * Non-finite vertices are refused by both variants with PT_ERR_INVALID_ARG ("vertex ... is not finite"): the host variant looks
 * on the host, the device variant on the device (a flag the builder's bounds kernel writes, read before anything else of the
 * build is launched) -- one NaN centroid would poison every Morton key.
 * A refused call (bad arguments, over capacity, a non-finite vertex, an out-of-range materialIndex in a host array, a HIP error)
 * leaves the scene exactly as it was: PTReadGeometry returns the same bytes, frames are the same, later calls work.
 * Host traffic: one 4-byte counter per tree level and the flags are read back, never nodes or triangle rows.  The call
 * therefore SYNCHRONISES WITH THE UPDATE STREAM (not with the passes in flight on the other streams).  The builder's work
 * arrays and the sort's temporary storage live in the context, sized for the largest BLAS rebuilt so far: no allocation per
 * call after the first.  After a rebuild PTUpdateGeometry refits the new tree and PTMeasureGeometry measures it.
 *
 * Quality.  nodeCount and levels are those of the nodes reachable from the root.  sahCost = 1 + the sum over every occupied
 * slot of every reachable node of halfArea(slot) / rootHalfArea * (1 for an inner slot, popcount(meta >> 5) for a leaf slot),
 * halfArea = ex*ey + ey*ez + ez*ex of the slot's decoded extent (q_hi - q_lo) * 2^e; rootHalfArea is that of the fold of the
 * root's occupied slots' decoded boxes lo + q * 2^e; all in float64; rootHalfArea == 0 (a degenerate tree) gives sahCost = 0.  It
 * is the expected number of node visits plus triangle tests of a random ray that hits the root box.
 * PTMeasureGeometry measures the BLAS's current tree on the device (after the updates enqueued so far), synchronises and reads
 * back one small record.  Before any update of the BLAS it walks it as the first update would; the BLAS's triangle count is
 * then taken from its row span (triOffset to the next larger distinct triOffset among the instances, or the end of the rows).
 * PTMeasureBVHArrays is the host twin (no GPU) on arrays as GetCWBVHData / PTReadGeometry return them (root = node 0): it
 * refuses (0, PTGetBVHBuildError has the reason) anything that is not a CWBVH of triangleCount triangles; nodeCapacity there is
 * nodeBytes / 80, so zero nodes appended to the array change nothing else.  Returns 1 on success.
 * ===================================================================================================================== */
typedef struct PTGeometryQuality {
    uint32_t structSize;          /* sizeof(PTGeometryQuality) of the caller's header; members are only appended */
    uint32_t nodeCapacity;        /* nodes of the BLAS's span */
    uint32_t nodeCount;           /* nodes reachable from the root */
    uint32_t triangleCount;
    uint32_t levels;
    uint32_t reserved;
    double   rootHalfArea;
    double   sahCost;
} PTGeometryQuality;

#ifdef __cplusplus
static_assert(sizeof(PTGeometryQuality) == 40, "PTGeometryQuality is 40 bytes");
#else
_Static_assert(sizeof(PTGeometryQuality) == 40, "PTGeometryQuality is 40 bytes");
#endif

PT_API int PTRebuildGeometry(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* vertices,
                             int triangleCount, const PTTriangleAttributes* attrsOrNull);                 /* host arrays, copied before return */
PT_API int PTRebuildGeometryDevice(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const PTFloat4* dVertices,
                                   int triangleCount, const PTTriangleAttributes* dAttrsOrNull);          /* device arrays, read in stream order */
PT_API int PTMeasureGeometry(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, PTGeometryQuality* out);
PT_API int PTMeasureBVHArrays(const PTFloat4* bvhNodes, uint64_t nodeBytes, const PTFloat4* bvhTris, uint64_t triBytes, int triangleCount,
                              PTGeometryQuality* out);                                                    /* host twin, no GPU */

/* =====================================================================================================================
 * Part 11: skinned geometry.  Parts 9 and 10 take a deforming mesh once its new vertices exist; this part makes them, on the
 * GPU, from what a skinned character changes per frame: a joint palette (48 bytes per joint).  PTSetSkin uploads the rest pose,
 * the joint indices and the weights of one BLAS once; PTSkinGeometry then takes a palette, skins the vertices into a buffer the
 * context owns and runs exactly the refit (Part 9) or rebuild (Part 10) the ...Device variants run on them.  No vertex is
 * uploaded per frame and none is read back: the one number the host then lacks, the mesh's local box, is returned.
 *
 * The rule (skin_rule.h; bit-defined under DESIGN.md 3: one IEEE binary32 operation per operator, left to right, no
 * contraction).  The palette is jointCount x 12 floats: the three rows of the 3x4 matrix M[j] that takes rest space to the BLAS's
 * local space (joint world x inverse bind).  For a vertex with joints j0 ... j3 and weights w0 ... w3, each of the 12 elements of
 * its blend matrix is  B = ((w0*M[j0] + w1*M[j1]) + w2*M[j2]) + w3*M[j3]  -- all four terms always, a zero weight is not
 * skipped, the weights are used as given (not renormalised).  Position, per row r:  ((B[r][0]*x + B[r][1]*y) + B[r][2]*z) +
 * B[r][3]; the output w is 0.  Normals and tangents, per corner:  v' = B3 * v (the rows without the translation), then
 * v' * (1 / sqrt(dot(v', v')));  if dot is 0 or not finite the REST vector is kept.  B3 itself transforms the normals: the rule
 * assumes joints without non-uniform scale (a sheared normal would need the inverse transpose).  The pads, uv0, uv1, uv2 and
 * materialIndex of a record are copied from restAttrs.  Bounds: compare-and-select min and max over the 3 * T positions.
 *
 * PTSetSkin.  The BLAS is named and checked as in Part 9 (the three offsets, triangleCount).  restVertices: 3 * T PTFloat4 in the
 * BLAS's primitive order (PTUpdateGeometry's input layout, w ignored); joints: 3 * T x 4 uint16; weights: 3 * T x 4 float;
 * restAttrs: T records, or NULL (the attribute records then are never touched).  Checked once, on the host: 1 <= jointCount <=
 * PT_SKIN_MAX_JOINTS, every joint index < jointCount, weights and rest vertices finite, and without HAS_TLAS every
 * materialIndex < materialCount -- the kernels then index the palette and the materials with nothing else.  The arrays are
 * copied before the call returns and stay on the device: 40 bytes per vertex, plus 128 bytes per triangle with restAttrs.  A
 * second call for the same BLAS replaces its skin, a NULL desc removes it (both wait for the update stream); PTSetScene
 * discards every skin, PTDestroy frees them.
 *
 * PTSkinGeometry (palette in host memory, copied before return; non-finite matrices are refused) and PTSkinGeometryDevice
 * (palette in device memory, 16-byte aligned, read in the context stream's order; not inspected: non-finite matrices give an
 * unspecified but memory-safe tree on a refit, and the builder's finiteness flag refuses them on a rebuild).  flags: 0 = refit,
 * PT_SKIN_REBUILD = Part 10's rebuild with its capacity rule and refusals.  On the update stream, in this order: the palette
 * upload, the skin kernel, the attribute records straight into the target attribute generation (a skin with restAttrs), then
 * the refit or the rebuild.  Generations, carry-over, ordering against passes in flight, "accumulation is not reset" and "a
 * refused call leaves the scene as it was" are Part 9's and Part 10's.  outBounds (may be NULL): min.xyz then max.xyz of the
 * skinned vertices, a 24-byte read-back -- the call then synchronises with the update stream only (as a rebuild always does);
 * with NULL a refit does not synchronise.  On a HAS_TLAS scene these are the local bounds whose transformed corners the caller
 * sends through PTUpdateInstances.
 * Errors: PT_ERR_NO_SCENE before PTSetScene; PT_ERR_INVALID_ARG for a NULL context or array, a BLAS without a skin, a jointCount
 * that is not the skin's, a refused array.
 *
 * PTSkinVerticesHost is the host twin (no GPU): the same rule on the host, byte for byte.  outAttrs needs desc->restAttrs;
 * outAttrs and outBounds may be NULL.  It makes PTSetSkin's checks (no material count) and refuses non-finite matrices; returns
 * 1, or 0 with PTGetBVHBuildError() set.
 * ===================================================================================================================== */
#define PT_SKIN_MAX_JOINTS 1024u
#define PT_SKIN_REBUILD    0x1u

typedef struct PTSkinDesc {
    uint32_t        structSize;   /* sizeof(PTSkinDesc) of the caller's header; members are only appended */
    uint32_t        jointCount;   /* 1 ... PT_SKIN_MAX_JOINTS */
    const PTFloat4* restVertices; /* 3 * triangleCount */
    const uint16_t* joints;       /* 3 * triangleCount x 4 */
    const float*    weights;      /* 3 * triangleCount x 4 */
    const PTTriangleAttributes* restAttrs;   /* triangleCount, or NULL */
} PTSkinDesc;

#ifdef __cplusplus
static_assert(sizeof(PTSkinDesc) == 40, "PTSkinDesc is 40 bytes");
#else
_Static_assert(sizeof(PTSkinDesc) == 40, "PTSkinDesc is 40 bytes");
#endif

PT_API int PTSetSkin(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, int triangleCount, const PTSkinDesc* descOrNull);
PT_API int PTSkinGeometry(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const float* jointMatrices,
                          uint32_t jointCount, uint32_t flags, float* outBounds);                         /* host palette, copied before return */
PT_API int PTSkinGeometryDevice(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const float* dJointMatrices,
                                uint32_t jointCount, uint32_t flags, float* outBounds);                   /* device palette, read in stream order */
PT_API int PTSkinVerticesHost(const PTSkinDesc* desc, int triangleCount, const float* jointMatrices, PTFloat4* outVertices,
                              PTTriangleAttributes* outAttrsOrNull, float* outBoundsOrNull);               /* host twin, no GPU */

/* =====================================================================================================================
 * Part 12: morph targets.  A glTF character deforms in two steps: morph targets first, then the skin.  Part 11 is the second
 * step; this part adds the first and runs both in one kernel.  PTSetMorph uploads the sparse targets of one BLAS once;
 * PTMorphGeometry then takes one float per target (and optionally Part 11's joint palette), makes the vertices on the GPU and
 * runs the refit (Part 9) or rebuild (Part 10) on them, exactly as PTSkinGeometry does.
 *
 * The data.  A morph has targetCount targets and up to three streams: position deltas (required, may be empty), normal deltas
 * and tangent deltas (each optional: offsets and entries both NULL).  A stream is CSR over the BLAS's 3 * T corners, in
 * PTUpdateGeometry's input order: offsets[3T + 1] (offsets[0] == 0, non-decreasing), then entries {dx, dy, dz, target}; the
 * entries of one corner are in strictly ascending target order.  ONLY LISTED ENTRIES ARE APPLIED: a dense glTF target is the
 * case where every corner lists every target; a listed zero delta is still multiplied and added; an unlisted delta does not
 * exist (it is not a zero: -0, NaN and infinite-weight cases differ).
 *
 * The rule (morph_rule.h; bit-defined under DESIGN.md 3: one IEEE binary32 operation per operator, left to right, no
 * contraction).  Position: acc = rest.xyz; for each entry of the corner in order, per component, acc = acc + w[target] * d (one
 * product, one sum).  Without a palette the result is acc, output w = 0; with a palette it is Part 11's  B * (acc, 1)  with B the
 * blend matrix of the BLAS's skin (its joints and weights; the skin's own rest pose is not used).  Normals and tangents, per
 * corner, from the rest record's row: m = rest.xyz folded with the corner's entries of that stream in the same way.  Without a
 * palette a corner with no entry in the stream is copied bit for bit; otherwise d = (m.x*m.x + m.y*m.y) + m.z*m.z, and the result
 * is m * (1 / sqrt(d)), or the REST vector if d is 0 or not finite.  With a palette every corner is  B3 * m  normalised as in Part
 * 11, and a dot that is 0 or not finite keeps the REST vector (not m).  A tangent's w, the pads, uv0 .. uv2 and materialIndex are
 * the rest record's.  Bounds: compare-and-select min and max over the 3 * T output positions.
 *
 * PTSetMorph.  The BLAS is named and checked as in Part 9.  Checked once, on the host: 1 <= targetCount <=
 * PT_MORPH_MAX_TARGETS; for every stream offsets[0] == 0, offsets non-decreasing, every target < targetCount, targets strictly
 * ascending within a corner, deltas finite; rest vertices finite; without HAS_TLAS every materialIndex < materialCount; a normal
 * or tangent stream needs restAttrs -- the kernels then index the weights with a stored target and nothing else.  The arrays
 * are copied before the call returns and stay on the device, each stream as sliced ELL (slices of 64 corners, each padded to
 * its longest corner; padding is stored, never applied): 16 bytes per vertex for the morph's OWN rest pose (kept even when the
 * BLAS also has a skin: with both, the rest positions are on the device twice), 16 bytes per stored entry, 4 bytes per corner
 * and per slice and stream, plus 128 bytes per triangle with restAttrs.  A second call replaces the morph, a NULL desc
 * removes it (both wait for the update stream); PTSetScene discards every morph, PTDestroy frees them.
 *
 * PTMorphGeometry (weights and palette in host memory, copied before return; non-finite weights or matrices are refused before
 * anything is enqueued) and PTMorphGeometryDevice (both in device memory, 16-byte aligned, read in the context stream's order,
 * not inspected).  targetCount must be the morph's.  jointMatrices may be NULL: a plain morph, also on a skinned BLAS; a
 * palette needs a skin on the BLAS with that jointCount.  flags: 0 = refit, PT_SKIN_REBUILD = Part 10's rebuild.  outBounds,
 * ordering, generations, carry-over, "accumulation is not reset" and "a refused call leaves the scene as it was" are Part 11's.
 * Errors: PT_ERR_NO_SCENE before PTSetScene; PT_ERR_INVALID_ARG for a NULL context or weights, a BLAS without a morph, a
 * targetCount that is not the morph's, a palette without a skin, a jointCount that is not the skin's, a refused array.
 *
 * PTMorphVerticesHost is the host twin (no GPU): the same rule, byte for byte.  skin (with jointMatrices) supplies joints and
 * weights only; jointMatrices == NULL is a plain morph, jointMatrices without skin is refused.  outAttrs needs desc->restAttrs.
 * Returns 1, or 0 with PTGetBVHBuildError() set.  PTMorphLayoutHost is the host's conversion of one CSR stream into the device
 * layout, for tests: outCount[cornerCount], outSliceBase[ceil(cornerCount / 64) + 1], outEntries[the returned count]; slot s of
 * corner c is outEntries[outSliceBase[c / 64] + 64 * s + c % 64] and is the corner's s-th entry if s < outCount[c], else padding
 * (all zero).  With all three NULL it only returns the stored entry count; UINT64_MAX: that count does not fit 32 bits.
 * ===================================================================================================================== */
#define PT_MORPH_MAX_TARGETS 1024u

typedef struct PTMorphEntry { float dx, dy, dz; uint32_t target; } PTMorphEntry;

typedef struct PTMorphDesc {
    uint32_t        structSize;   /* sizeof(PTMorphDesc) of the caller's header; members are only appended */
    uint32_t        targetCount;  /* 1 ... PT_MORPH_MAX_TARGETS */
    const PTFloat4* restVertices; /* 3 * triangleCount, the morph's own rest pose */
    const PTTriangleAttributes* restAttrs;   /* triangleCount, or NULL; required by a normal or tangent stream */
    const uint32_t*     positionOffsets;     /* 3 * triangleCount + 1 */
    const PTMorphEntry* positionEntries;     /* may be NULL if positionOffsets[3 * triangleCount] == 0 */
    const uint32_t*     normalOffsets;       /* both NULL: no stream */
    const PTMorphEntry* normalEntries;
    const uint32_t*     tangentOffsets;
    const PTMorphEntry* tangentEntries;
} PTMorphDesc;

#ifdef __cplusplus
static_assert(sizeof(PTMorphEntry) == 16, "PTMorphEntry is 16 bytes");
static_assert(sizeof(PTMorphDesc) == 72, "PTMorphDesc is 72 bytes");
#else
_Static_assert(sizeof(PTMorphEntry) == 16, "PTMorphEntry is 16 bytes");
_Static_assert(sizeof(PTMorphDesc) == 72, "PTMorphDesc is 72 bytes");
#endif

PT_API int PTSetMorph(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, int triangleCount, const PTMorphDesc* descOrNull);
PT_API int PTMorphGeometry(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const float* weights, uint32_t targetCount,
                           const float* jointMatricesOrNull, uint32_t jointCount, uint32_t flags, float* outBounds);      /* host arrays, copied before return */
PT_API int PTMorphGeometryDevice(PTContext* ctx, int32_t bvhOffset, int32_t triOffset, int32_t triAttributeOffset, const float* dWeights, uint32_t targetCount,
                                 const float* dJointMatricesOrNull, uint32_t jointCount, uint32_t flags, float* outBounds); /* device arrays, read in stream order */
PT_API int PTMorphVerticesHost(const PTMorphDesc* desc, const PTSkinDesc* skinOrNull, int triangleCount, const float* weights, const float* jointMatricesOrNull,
                               PTFloat4* outVertices, PTTriangleAttributes* outAttrsOrNull, float* outBoundsOrNull);      /* host twin, no GPU */
PT_API uint64_t PTMorphLayoutHost(const uint32_t* offsets, const PTMorphEntry* entries, uint32_t cornerCount, uint32_t* outCount, uint32_t* outSliceBase,
                                  PTMorphEntry* outEntries);                                                               /* the device layout of one stream, for tests */

/* =====================================================================================================================
 * Part 13: irradiance gathers.  How much light arrives AT a surface point?  Part 8 answers it along one ray; a lightmap texel
 * or a light probe wants the irradiance E at a receiver: a position and a normal.  The host hands over a list of receivers and
 * a sample range, the path tracer builds every gather direction itself, lights the receiver directly (NEE at the receiver:
 * point and spot lights included) and runs the samples of an entry in parallel.  An addition beside the reference's ABI,
 * detected by symbol; PTGetVersion is unchanged.
 *
 * The rule (bit-exact).  A receiver is a white Lambertian point with normal N; irradiance is PI times the radiance it sends out.
 *  - Seeding.  Sample j (0 <= j < samples) of entry i is independent of the entry's other samples: its RNG starts at
 *    s = seed_i; pt_rng_next(&s); s += firstSample + j  (uint32 arithmetic) and depends on nothing else, so the samples
 *    [a, a + n) of one call are the samples of any split of that range into calls.
 *  - The receiver step runs in the order of the render's material branch (path_shade_hit) with the same code for everything
 *    but the BSDF.  No alpha draw and no roulette at the receiver.  hit.position = P, hit.normal = hit.ffnormal = N (as
 *    given, never re-normalised).  The NEE origin is P + N * PT_EPSILON.  Environment NEE and light NEE take the render's
 *    draws, light pick and EvalLight arithmetic; the BSDF is Lambert, f = pdf = max(dot(N, L), 0) / PT_PI; the validity codes
 *    stay (a traced ray that adds nothing when pdf <= 0).  Then two draws r1, r2:
 *    L = onb_to_world(make_onb(N), cosine_sample_hemisphere(r1, r2)), pdf = L_local.z / PT_PI.  With pdf > 0 the path goes
 *    on with direction L, origin P + L * PT_EPSILON, throughput (1, 1, 1) exactly (the Lambert term over the pdf, never
 *    divided out), scatterPdf = pdf, maxRoughness = 1 and depth 1; else the sample ends.  Either way the receiver's NEE is
 *    pending with throughput 1 and the radiance so far is 0.
 *  - The rest of the path is the render's own: firefly filter, Russian roulette, environment, lights, textures and HAS_TLAS of
 *    `params`; MaxRayBounces counts the receiver as the first bounce.  SamplesPerPass is not read.  A sample's value is
 *    e_j = c_j * PT_PI per channel (one fp32 multiply), c_j being the sample's radiance after the fold (the firefly filter
 *    acts on c_j).
 *  - out[i].rgb = (e_0 + e_1 + ...) / (float)samples, summed in ascending j; out[i].m2 = the sum of luminance3(e_j)^2 in the
 *    same order (the sample variance of the luminance is (m2 - samples * lum(rgb)^2) / (samples - 1)).  Nothing past `count`
 *    is written.
 *  - PTGatherRays writes, for slot i * samples + j, the ray {origin, direction} and the RNG state the receiver step leaves:
 *    what PTTraceRadiance continues from.  A sample that ended at the receiver gets a NaN direction.  It needs a scene (the
 *    NEE draws depend on the lights and the environment) and counts nothing in PTStats.
 *  - Stream-ordered on the context's stream like Part 8; dRecv, dOut and dRays are 16-byte aligned.  Slot i * samples + j
 *    carries sample j of entry i; a launch sequence holds floor(2^21 / samples) whole entries, longer lists are cut into
 *    such chunks, each on the next state set, joined after the last one.
 *  - PTStats: paths = count x samples; rays and fetches by the render's definitions (the receiver's shadow rays and light
 *    fetch included); pixelsWritten and pixelsRead do not move.  With profiling on, every chunk is one entry of PTGetTimings.
 *  - Schedules 1, 2 and 3; schedules 0 and 4 return PT_ERR_UNSUPPORTED, as do samples == 0, samples > 65536 and
 *    MaxRayBounces > 8191.  PT_ERR_INVALID_ARG for a NULL or misaligned pointer and (PTGatherIrradianceHost) a nonzero
 *    `reserved`; PT_ERR_NO_SCENE before PTSetScene.  count == 0 returns PT_OK and launches nothing.  No CPU fallback.
 * ===================================================================================================================== */
#define PT_GATHER_MAX_SAMPLES 65536u

typedef struct PTReceiver {       /* 32 bytes: two 16-byte loads */
    float    position[3];
    uint32_t seed;
    float    normal[3];           /* unit normal, used as given */
    uint32_t reserved;            /* must be 0 (PTGatherIrradianceHost checks it; the device path ignores it) */
} PTReceiver;

typedef struct PTIrradiance {     /* 16 bytes */
    float    rgb[3];              /* irradiance E: mean over the samples */
    float    m2;                  /* sum over the samples of luminance(e_j)^2 */
} PTIrradiance;

#ifdef __cplusplus
static_assert(sizeof(PTReceiver) == 32, "PTReceiver is 32 bytes");
static_assert(sizeof(PTIrradiance) == 16, "PTIrradiance is 16 bytes");
#else
_Static_assert(sizeof(PTReceiver) == 32, "PTReceiver is 32 bytes");
_Static_assert(sizeof(PTIrradiance) == 16, "PTIrradiance is 16 bytes");
#endif

/* Device pointers, stream-ordered on the context's stream. */
PT_API int PTGatherIrradiance(PTContext* ctx, const PTFrameParams* params, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                              PTIrradiance* dOut);
/* Host arrays: staged through device buffers the context keeps and grows; synchronous. */
PT_API int PTGatherIrradianceHost(PTContext* ctx, const PTFrameParams* params, const PTReceiver* recv, uint64_t count, uint32_t firstSample, uint32_t samples,
                                  PTIrradiance* out);
/* dRays: count * samples entries, entry-major. */
PT_API int PTGatherRays(PTContext* ctx, const PTFrameParams* params, const PTReceiver* dRecv, uint64_t count, uint32_t firstSample, uint32_t samples,
                        PTRadianceRay* dRays);

/* =====================================================================================================================
 * Part 14: lightmap charts.  Part 13 answers "what is the irradiance at these receivers"; this part makes the receivers of a
 * lightmap from a mesh and an atlas size, on the GPU, and turns the gathered list back into an image: PTRasterizeChart
 * rasterises the UV chart of one BLAS of the CURRENT scene into a compacted device list of PTReceiver entries, one per covered
 * texel; PTGatherIrradiance gathers; PTResolveLightmap scatters the PTIrradiance list into an RGBA image and dilates the chart
 * borders.  No vertex, receiver or texel crosses the bus.  An addition beside the reference's ABI, detected by symbol;
 * PTGetVersion is unchanged.
 *
 * The rasterisation rule (chart_rule.h; coverage is decided in integers, so any evaluation order gives the same bytes).
 *  - Inputs.  The BLAS is named as in Parts 9 to 12 (bvhOffset, triOffset, triAttributeOffset, triangleCount).  instance: -1 for
 *    the identity transform, else the index of a PTGpuInstance record as it currently stands on the device, whose three offsets
 *    must be the ones given: its localToWorld places the receivers, its worldToLocal turns the normals.  width, height: 1 ...
 *    8192.  Lightmap UVs: 6 floats per triangle (u0 v0 u1 v1 u2 v2), indexed by primIdx (the BLAS's primitive order), or NULL:
 *    uv0, uv1, uv2 of the BLAS's current PTTriangleAttributes.  Geometry is the CURRENT generation of the triangle records (v0,
 *    e1, e2, primIdx) and attribute records: a chart made after a refit, rebuild, skin or morph sees the deformed mesh.
 *  - Snap.  Corner k of primitive p: X_k = (int64)rintf(u_k * (float)(width * 256)), Y_k = (int64)rintf(v_k * (float)(height *
 *    256)): one fp32 multiply, round half even, 8 sub-texel bits.  A triangle with a non-finite UV or any |X|, |Y| > 2^23 is not
 *    in the chart (this is how a caller excludes triangles).  No wrap, no repeat.
 *  - Edge functions, int64, exact: E(a, b; s) = (b.X - a.X) * (s.Y - a.Y) - (b.Y - a.Y) * (s.X - a.X); A = E(p0, p1; p2).  A
 *    triangle with A == 0 is skipped, and so is one whose fp32 cross(e1, e2) (cross3's expression) has a squared length (dot3's)
 *    that is 0 or not finite.  A negative A flips the sign of all three edge values: mirrored charts rasterise.
 *  - Coverage.  Texel (x, y), 0 <= x < width, 0 <= y < height, is sampled at s = (256 x + 128, 256 y + 128) and covered by p
 *    when E(p1, p2; s), E(p2, p0; s) and E(p0, p1; s), so signed, are all >= 0 (edges are inclusive).  Its owner is the covering
 *    primitive with the lowest primIdx: shared edges are watertight, overlaps deterministic.
 *  - Barycentrics.  b1 = (float)((double)E(p2, p0; s) / (double)A) (corner 1, the role of a hit's u), b2 = (float)((double)
 *    E(p0, p1; s) / (double)A) (corner 2, a hit's v); the conversions are exact, the fp64 divide and the narrowing correctly
 *    rounded.  Corner 0 gets 1.0f - b1 - b2.
 *  - Receiver.  Local position per component (v0 + e1 * b1) + e2 * b2 from the triangle record, so the receiver lies on the
 *    triangle the intersector sees; world position per row r  ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r]  with m =
 *    localToWorld (instance -1: the local position).  Normal: n = (n0 * (1.0f - b1 - b2) + n1 * b1) + n2 * b2 per component, then
 *    n * (1 / sqrt((n.x*n.x + n.y*n.y) + n.z*n.z)); with an instance then t[r] = ((n.x * w[4r] + n.y * w[4r + 1]) + n.z *
 *    w[4r + 2]) + 0.0f * w[4r + 3] with w = worldToLocal, normalised the same way (the render's HAS_TLAS hit).  If any component
 *    of the result is not finite, cross(e1, e2) takes n's place through the same steps.  seed = seedBase + texelIndex in uint32
 *    arithmetic, texelIndex = y * width + x; reserved = 0.  Every fp32 operator is one binary32 operation, left to right.
 *  - Output.  The covered texels in ascending texelIndex: texels[i] and recv[i].  A texel's receiver depends on its own index,
 *    its owner and the inputs only.
 *
 * PTRasterizeChart.  Device arrays (dTexels 4-byte, dRecv and dUvs 16-byte aligned), on the context's stream and ordered like
 * PTGatherRays; every scene update joins that stream.  *count receives the number of covered texels: an 8-byte read-back, so
 * THE CALL SYNCHRONISES WITH THE CONTEXT STREAM.  dTexels == NULL and dRecv == NULL: only the count.  count > capacity:
 * PT_ERR_INVALID_ARG with *count set and nothing written.  The compaction runs on the device (owner map, per-block counts, a
 * scan, emit).  The first call on a scene reads the node and triangle buffers back once and the first call on a BLAS walks it,
 * as Part 9's first update does.  Memory, in the context, grown on demand, kept across PTSetScene, freed by PTDestroy: 4 bytes
 * per texel (the owner map), 4 per 256 texels, 8 per triangle; PTResolveLightmap with dilate > 0: 16 bytes per texel.
 * Errors: PT_ERR_NO_SCENE before PTSetScene; PT_ERR_INVALID_ARG for a NULL context, desc or count, a misaligned pointer, only one
 * of dTexels and dRecv, offsets that name no BLAS, a triangleCount that is not the BLAS's, an instance out of range or of
 * another BLAS, a size outside 1 ... 8192, a nonzero reserved field.
 *
 * PTResolveLightmap.  image: width * height RGBA float32, 16-byte aligned.  Every texel is cleared to 0, then image[texels[i]] =
 * (irr[i].rgb, 1.0f).  Texel indices must be unique (with duplicates one of them is written); an index >= width * height is
 * skipped (the host twin refuses it).  Then `dilate` passes, 0 ... 16; pass p reads the image of pass p - 1: a texel with w != 0
 * is copied; a texel with w == 0 looks at its 8 neighbours inside the image in the order (dy, dx) = (-1,-1), (-1,0), (-1,1),
 * (0,-1), (0,1), (1,-1), (1,0), (1,1); with n > 0 of them at w != 0 it becomes (((0 + rgb_a) + rgb_b) + ...) / (float)n over
 * those, in that order, with w = 0.5f, else it stays 0.  The result ends in the caller's image; the second image is the
 * context's.  Stream-ordered on the context's stream, not synchronising, needs no scene.
 *
 * The host twins (no context, no GPU; they return 1, or 0 with PTGetBVHBuildError() set).  PTRasterizeChartHost: tris = the BLAS's
 * 3 * triangleCount rows and attrs = its triangleCount records as PTReadGeometry returns them (from triOffset, from
 * triAttributeOffset); the desc's offsets and instance are not read; localToWorld and worldToLocal: 16 floats each in the
 * record's memory order, or both NULL.  count > capacity returns 0 with *count set.  PTResolveLightmapHost: the same image.
 * ===================================================================================================================== */
#define PT_CHART_MAX_SIZE   8192u
#define PT_CHART_MAX_DILATE 16u

typedef struct PTChartDesc {
    uint32_t structSize;          /* sizeof(PTChartDesc) of the caller's header; members are only appended */
    int32_t  bvhOffset, triOffset, triAttributeOffset;
    int32_t  triangleCount;
    int32_t  instance;            /* -1: identity */
    uint32_t width, height;       /* 1 ... PT_CHART_MAX_SIZE */
    uint32_t seedBase;
    uint32_t reserved[3];         /* must be 0 */
} PTChartDesc;

#ifdef __cplusplus
static_assert(sizeof(PTChartDesc) == 48, "PTChartDesc is 48 bytes");
#else
_Static_assert(sizeof(PTChartDesc) == 48, "PTChartDesc is 48 bytes");
#endif

/* Device arrays, on the context's stream; synchronises (the count). */
PT_API int PTRasterizeChart(PTContext* ctx, const PTChartDesc* desc, const float* dUvsOrNull, uint32_t* dTexels, PTReceiver* dRecv, uint64_t capacity,
                            uint64_t* count);
PT_API int PTRasterizeChartHost(const PTChartDesc* desc, const PTFloat4* tris, const PTTriangleAttributes* attrs, const float* uvsOrNull,
                                const float* localToWorldOrNull, const float* worldToLocalOrNull, uint32_t* texels, PTReceiver* recv, uint64_t capacity,
                                uint64_t* count);                                                          /* host twin, no GPU */
/* Device arrays, stream-ordered on the context's stream. */
PT_API int PTResolveLightmap(PTContext* ctx, const uint32_t* dTexels, const PTIrradiance* dIrr, uint64_t count, uint32_t width, uint32_t height,
                             uint32_t dilate, void* dImage);
PT_API int PTResolveLightmapHost(const uint32_t* texels, const PTIrradiance* irr, uint64_t count, uint32_t width, uint32_t height, uint32_t dilate,
                                 void* image);                                                             /* host twin, no GPU */

/* =====================================================================================================================
 * Part 15: SH light probes.  Parts 13 and 14 bake the static surfaces; what lights an object that MOVES through the baked
 * scene is a probe: a point without a normal that keeps the light arriving from every direction as nine spherical-harmonic
 * coefficients per channel (bands 0 to 2), from which the irradiance for any normal is nine multiply-adds.  The host hands over
 * positions and a sample range; directions, paths, projection and the direct light of point and spot lights are made on the
 * GPU.  An addition beside the reference's ABI, detected by symbol; PTGetVersion is unchanged.
 *
 * The rule (bit-exact; sh_rule.h is its one definition: the kernels, the host twins and tests/probe_ref.py evaluate it).
 *  - Seeding.  Part 13's, word for word: sample j (0 <= j < samples) of probe i starts at s = seed_i; pt_rng_next(&s);
 *    s += firstSample + j  (uint32 arithmetic).  Samples are independent of each other: the samples [a, a + n) of one call are
 *    the samples of any split of that range into calls.
 *  - Direction.  Two draws r1, r2 (pt_random_float): z = 1.0f - 2.0f * r1; rho = sqrt(max(1.0f - z * z, 0.0f));
 *    phi = PT_TWO_PI * r2; w = (rho * pt_cos(phi), rho * pt_sin(phi), z).  Uniform on the sphere, pdf 1 / (4 PI); one fp32
 *    operation per operator, pt_sin / pt_cos of ptmi_math.h, no renormalisation.
 *  - Path.  PTTraceRadiance's: the sample is the path whose first ray is {origin P, direction w} with the RNG state after the
 *    two draws -- the state Part 8 starts an entry with: depth 0, nothing pending --, and everything after that is the
 *    render's code under `params` (bounces, roulette, firefly filter, environment, lights, textures, HAS_TLAS).  SamplesPerPass
 *    is not read.  The sample's value L_j is the path's colour after the fold, so rectangle lights and the sky are seen as a
 *    camera ray sees them.
 *  - Basis.  Real SH with x, y, z the components of w, in this order and as these expression trees:
 *      Y0 = 0.28209479f               Y1 = 0.48860251f * y           Y2 = 0.48860251f * z
 *      Y3 = 0.48860251f * x           Y4 = 1.09254843f * (x * y)     Y5 = 1.09254843f * (y * z)
 *      Y6 = 0.31539157f * (3.0f * (z * z) - 1.0f)                    Y7 = 1.09254843f * (x * z)
 *      Y8 = 0.54627422f * (x * x - y * y)
 *  - Projection.  Lane l of 64 owns the samples j = l, l + 64, ... in ascending j.  Its 28 partial sums start at +0.0f:
 *    acc[k][c] = acc[k][c] + L_j[c] * Y_k(w_j)  (a multiply, then an add; no fma) and m2 = m2 + lum * lum with
 *    lum = (L.r * 0.299f + L.g * 0.587f) + L.b * 0.114f.  The 64 partials v[0..63] of each sum are folded by the fixed tree:
 *    for h = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l + h] for every l < h.  sh[k][c] = (v[0] * 12.566371f) / (float)samples;
 *    m2 is v[0], unscaled.
 *  - Delta lights (flag PT_PROBE_DELTA_LIGHTS).  No path can hit a point or a spot light, so they are added after the scaling,
 *    for every light of the scene in ascending index that is a point or a spot light: lsDirection, lsDistance and
 *    Li = emission * falloff exactly as the render's light NEE makes them (SampleOneLight and EvalLight) with scatterPos = P;
 *    one any-hit ray {P, lsDirection, tmax = PT_FAR_PLANE} by Part 3's rules (the render's shadow ray, which has no far end: a
 *    light that geometry encloses lights no probe, as it lights no pixel and no receiver).  A pair whose light is of another
 *    type, or whose Li is zero in every channel, has tmax = 0 -- Part 3's miss without a walk -- and is skipped.  A visible pair
 *    adds sh[k][c] = sh[k][c] + Li[c] * Y_k(lsDirection); an occluded or skipped pair adds nothing, so the bits stay.
 *    (Cosine-convolved, the term is Li * max(dot(N, L), 0): what Part 13's receiver gets from the same light.)
 *  - Evaluation.  E(N)[c] = the sum over k = 0 ... 8, ascending, from +0.0f, of (A_k * sh[k][c]) * Y_k(N) with
 *    A = 3.14159265f (k = 0), 2.09439510f (k = 1, 2, 3), 0.78539816f (k = 4 ... 8).  PTProbeIrradiance: out[q] = {E(normal_q) of
 *    probe probe_q, m2 = 0}; a probe index >= probeCount yields zeros and reads nothing.
 *  - PTProbeRays writes, for slot i * samples + j, the PTRadianceRay {P, w, the RNG state after the two draws, 0}: what
 *    PTTraceRadiance continues from.  It needs no scene and counts nothing.
 *  - Nothing past `count` is written.  Stream-ordered on the context's stream like Part 13; every device pointer is 16-byte
 *    aligned.  Slot i * samples + j carries sample j of probe i; a launch sequence holds floor(2^21 / samples) whole probes,
 *    longer lists are cut into such chunks on successive state sets, joined after the last one.  The delta rays of the whole
 *    call run first, on the context's stream, in scratch the context keeps and grows (64 bytes per probe and light).
 *  - PTStats: paths = count x samples with or without the flag; rays and fetches by the render's definitions; pixelsWritten and
 *    pixelsRead do not move.  With the flag and PTSetStatsLevel(ctx, 1), shadowRays also grows by count x lightCount (Part 3
 *    counts every ray of a batch).  With profiling on, every chunk is one entry of PTGetTimings.
 *  - Schedules 1, 2 and 3; schedules 0 and 4 return PT_ERR_UNSUPPORTED, as do samples == 0, samples > 65536 and
 *    MaxRayBounces > 8191.  PT_ERR_INVALID_ARG for a NULL or misaligned pointer and an unknown flag bit; PT_ERR_NO_SCENE
 *    before PTSetScene (PTProbeSH, PTProbeSHHost).  count == 0 returns PT_OK and launches nothing.  No CPU fallback.
 *  - The host twins take no context and no GPU; they return 1, or 0 with PTGetBVHBuildError() set.  PTProbeDirectionsHost
 *    writes PTProbeRays' entries.  PTProbeProjectHost: directions and colours are count x samples x 3 floats, entry-major;
 *    out[i] is the projection above (no delta term: that needs a scene).  PTProbeIrradianceHost is PTProbeIrradiance.
 * ===================================================================================================================== */
#define PT_PROBE_DELTA_LIGHTS 1u  /* add the direct light of point and spot lights */

typedef struct PTProbe {          /* 16 bytes: one 16-byte load */
    float    position[3];
    uint32_t seed;
} PTProbe;

typedef struct PTProbeCoeffs {    /* 112 bytes: seven 16-byte stores; what PTProbeSH writes (C has one name space for both) */
    float    sh[9][3];            /* coefficient k, channel c */
    float    m2;                  /* sum over the samples of luminance(L_j)^2 */
} PTProbeCoeffs;

typedef struct PTProbeQuery {     /* 16 bytes */
    float    normal[3];           /* unit normal, used as given */
    uint32_t probe;               /* index into the PTProbeCoeffs array */
} PTProbeQuery;

#ifdef __cplusplus
static_assert(sizeof(PTProbe) == 16, "PTProbe is 16 bytes");
static_assert(sizeof(PTProbeCoeffs) == 112, "PTProbeCoeffs is 112 bytes");
static_assert(sizeof(PTProbeQuery) == 16, "PTProbeQuery is 16 bytes");
#else
_Static_assert(sizeof(PTProbe) == 16, "PTProbe is 16 bytes");
_Static_assert(sizeof(PTProbeCoeffs) == 112, "PTProbeCoeffs is 112 bytes");
_Static_assert(sizeof(PTProbeQuery) == 16, "PTProbeQuery is 16 bytes");
#endif

/* Device pointers, stream-ordered on the context's stream. */
PT_API int PTProbeSH(PTContext* ctx, const PTFrameParams* params, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples,
                     uint32_t flags, PTProbeCoeffs* dOut);
/* Host arrays: staged through device buffers the context keeps and grows; synchronous. */
PT_API int PTProbeSHHost(PTContext* ctx, const PTFrameParams* params, const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples,
                         uint32_t flags, PTProbeCoeffs* out);
/* dRays: count * samples entries, entry-major. */
PT_API int PTProbeRays(PTContext* ctx, const PTFrameParams* params, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples,
                       PTRadianceRay* dRays);
/* dSH: probeCount entries; dQueries, dOut: count entries. */
PT_API int PTProbeIrradiance(PTContext* ctx, const PTProbeCoeffs* dSH, uint64_t probeCount, const PTProbeQuery* dQueries, uint64_t count, PTIrradiance* dOut);
/* host twins, no GPU */
PT_API int PTProbeDirectionsHost(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, PTRadianceRay* rays);
PT_API int PTProbeProjectHost(const float* directions, const float* colours, uint64_t count, uint32_t samples, PTProbeCoeffs* out);
PT_API int PTProbeIrradianceHost(const PTProbeCoeffs* sh, uint64_t probeCount, const PTProbeQuery* queries, uint64_t count, PTIrradiance* out);

/* =====================================================================================================================
 * Part 16: probe volumes.  Part 15 evaluates one probe the caller names.  A point BETWEEN the probes of a regular grid is lit
 * by the eight probes around it, and a blend that does not know where the walls are leaks light through them: the probe in the
 * lit room brightens the dark room next door.  So every probe also keeps a small octahedral map of the distances it sees, and
 * the lookup weighs each corner by trilinear position, by the side of the surface it is on (wrap shading) and by a Chebyshev
 * bound on its visibility.  The host hands over positions and normals -- Part 13's receivers, so the lists of
 * PTRasterizeChart go in unchanged -- and gets irradiance back.  An addition detected by symbol; PTGetVersion is unchanged.
 *
 * The rule (bit-exact; volume_rule.h is its one definition: the kernels, the host twins and tests/volume_ref.py evaluate it;
 * every fp32 operator below is one IEEE binary32 operation in the order written, no fma).
 *  - Depth record.  PTProbeDepthMap holds an 8 x 8 octahedral map, texel l = v * 8 + u: moments[l][0] is the weighted mean
 *    distance, moments[l][1] the weighted mean squared distance.
 *  - Texel direction d_l.  a = ((float)u + 0.5f) * 0.25f - 1.0f, b likewise from v (never 0).  z = (1.0f - |a|) - |b|.
 *    If z < 0: x = (1.0f - |b|) * sgn(a), y = (1.0f - |a|) * sgn(b); otherwise x = a, y = b.
 *    len = sqrt((x * x + y * y) + z * z); d_l = (x / len, y / len, z / len).
 *  - Samples.  Sample j of probe i has Part 15's seeding and direction w_j, word for word.  Its ray is the PTRay
 *    {P, w_j, tmax = maxDistance, 0}, traced as a closest-hit query by Part 3's rules; dist_j is the returned t, which is
 *    maxDistance on a miss: a far or absent surface reads maxDistance.
 *  - Accumulation.  Every texel sums over ALL samples in ascending j from +0.0f (no fold: one texel's sums are sequential):
 *    c = max((d.x * w.x + d.y * w.y) + d.z * w.z, 0.0f); c2 = c * c; c4 = c2 * c2; c8 = c4 * c4; c16 = c8 * c8;
 *    wt = c16 * c16  (cos^32);  sw = sw + wt;  s1 = s1 + wt * dist;  s2 = s2 + wt * (dist * dist).
 *    If sw > 0: mean = s1 / sw, mean2 = s2 / sw.  If sw == 0, no sample reached the texel and it counts as open:
 *    mean = maxDistance, mean2 = maxDistance * maxDistance.
 *  - Grid.  The probe at integer (ix, iy, iz) has index (iz * ny + iy) * nx + ix and position
 *    Q[a] = origin[a] + (float)i_a * spacing[a].
 *  - Lookup of the query {position P, normal N} (the seed is ignored):
 *    1. Pb[a] = P[a] + N[a] * normalBias.
 *    2. Per axis: g = (P[a] - origin[a]) / spacing[a]; g = g > 0.0f ? g : 0.0f (a NaN lands on 0);
 *       g = min(g, (float)(counts[a] - 1)).  With counts[a] > 1: i0 = min((uint32_t)g, counts[a] - 2), f = g - (float)i0;
 *       otherwise i0 = 0, f = 0.0f.
 *    3. Corners o = 0 ... 7 ascending; bit a of o selects the upper probe on axis a: i_a = min(i0 + bit, counts[a] - 1),
 *       t_a = bit ? f : 1.0f - f, tri = (t_x * t_y) * t_z.  A corner with tri == 0.0f is skipped and reads nothing.
 *    4. w = 1.0f.  v = Q - Pb, r = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z).  Only if r > 0:
 *       dir = v / r.
 *       PT_GRID_WRAP: t = (((dir.x * N.x + dir.y * N.y) + dir.z * N.z) + 1.0f) * 0.5f; w = w * (t * t + 0.2f).
 *       PT_GRID_VISIBILITY: e = -dir (from the probe to the point), s = (|e.x| + |e.y|) + |e.z|, a = e.x / s, b = e.y / s;
 *       if e.z < 0: a' = (1.0f - |b|) * sgn(a), b' = (1.0f - |a|) * sgn(b), with sgn(0) = +1.
 *       u = min((uint32_t)((a * 0.5f + 0.5f) * 8.0f), 7), v likewise from b (a NaN lands on 0); nearest texel, no filter.
 *       With that texel's mean and mean2, if r > mean: var = |mean2 - mean * mean|, dl = r - mean,
 *       ch = var / (var + dl * dl), w = w * ((ch * ch) * ch).
 *       Then, flags or not: if w < 0.2f, w = w * ((w * w) * 25.0f) (the crush); w = w * tri.
 *    5. E_o = Part 15's E(N) of the corner's coefficients; acc[c] = acc[c] + w * E_o[c]; sumW = sumW + w.
 *    6. out.rgb[c] = sumW > 0 ? acc[c] / sumW : 0; out.m2 = sumW, the support the point had (1 up to rounding with both
 *       flags off).
 *  - PTProbeDepth: stream-ordered on the context's stream.  The rays and hit records live in scratch the context keeps, 48
 *    bytes per sample, sized for one chunk of floor(2^21 / samples) whole probes; chunks run one after another on that
 *    stream.  PTStats moves as a PTTraceRays call of the same rays moves it.  PTProbeGridIrradiance needs no scene.
 *  - Nothing past `count` is written.  Every device pointer is 16-byte aligned.  dDepth may be NULL only without
 *    PT_GRID_VISIBILITY.
 *  - PT_ERR_INVALID_ARG for a NULL or misaligned pointer, an unknown flag bit, a nonzero `reserved`, a count of 0 or above
 *    1024 on an axis, an origin that is not finite, a spacing that is not finite and positive, a normalBias that is not
 *    finite and non-negative, a maxDistance that is not finite, not positive or not below PT_FAR_PLANE.  PT_ERR_UNSUPPORTED
 *    for samples == 0 and samples > 65536.  PT_ERR_NO_SCENE for PTProbeDepth before PTSetScene.  count == 0 returns PT_OK
 *    and launches nothing.  Arguments are checked before the context is used.  No CPU fallback.
 *  - The host twins take no context and no GPU; they return 1, or 0 with PTGetBVHBuildError() set.
 *    PTProbeDepthProjectHost takes the count x samples distances as an array, entry-major, and makes the directions itself.
 *    PTProbeGridIrradianceHost is PTProbeGridIrradiance.
 * ===================================================================================================================== */
#define PT_GRID_WRAP        1u    /* weigh a corner by the side of the surface it is on */
#define PT_GRID_VISIBILITY  2u    /* weigh a corner by the Chebyshev bound of its depth record */

typedef struct PTProbeDepthMap {     /* 512 bytes: one 8-byte store per lane of a wave */
    float    moments[64][2];      /* texel l = v * 8 + u: mean distance, mean squared distance */
} PTProbeDepthMap;

typedef struct PTProbeGrid {      /* 48 bytes; a host struct, passed by pointer */
    float    origin[3];           /* the position of probe (0, 0, 0) */
    uint32_t flags;               /* PT_GRID_... */
    float    spacing[3];          /* finite, > 0 */
    float    normalBias;          /* finite, >= 0 */
    uint32_t counts[3];           /* 1 ... 1024 probes per axis, x fastest */
    uint32_t reserved;            /* must be 0 */
} PTProbeGrid;

#ifdef __cplusplus
static_assert(sizeof(PTProbeDepthMap) == 512, "PTProbeDepthMap is 512 bytes");
static_assert(sizeof(PTProbeGrid) == 48, "PTProbeGrid is 48 bytes");
#else
_Static_assert(sizeof(PTProbeDepthMap) == 512, "PTProbeDepthMap is 512 bytes");
_Static_assert(sizeof(PTProbeGrid) == 48, "PTProbeGrid is 48 bytes");
#endif

/* Device pointers, stream-ordered on the context's stream. */
PT_API int PTProbeDepth(PTContext* ctx, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples, float maxDistance,
                        PTProbeDepthMap* dOut);
/* Host arrays: staged through device buffers the context keeps and grows; synchronous. */
PT_API int PTProbeDepthHost(PTContext* ctx, const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, float maxDistance,
                            PTProbeDepthMap* out);
/* dSH, dDepth: one entry per probe of the grid; dQueries, dOut: count entries. */
PT_API int PTProbeGridIrradiance(PTContext* ctx, const PTProbeGrid* grid, const PTProbeCoeffs* dSH, const PTProbeDepthMap* dDepth,
                                 const PTReceiver* dQueries, uint64_t count, PTIrradiance* dOut);
/* host twins, no GPU */
PT_API int PTProbeDepthProjectHost(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const float* distances,
                                   float maxDistance, PTProbeDepthMap* out);
PT_API int PTProbeGridIrradianceHost(const PTProbeGrid* grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth, const PTReceiver* queries,
                                     uint64_t count, PTIrradiance* out);

/* =====================================================================================================================
 * Part 17: the lightmap denoiser.  "The bake is the gather" (DESIGN.md 5.19), so a cheaper bake is one that needs fewer samples
 * per texel.  PTDenoiseLightmap filters a gathered list in texel space between PTGatherIrradiance and PTResolveLightmap: list
 * in, list out.  Part 4's filter cannot do it: its guides are a camera's, and it knows nothing of charts -- two texels that
 * touch in an atlas may lie in different rooms or on either side of a fold, and an image filter bleeds light across such a
 * seam.  Here every texel has an exact world position and normal (its PTReceiver) and a variance (PTIrradiance.m2), and a tap
 * that is no neighbour in the world is cut whatever its normal and plane are.  An addition detected by symbol; PTGetVersion is
 * unchanged.
 *
 * The rule (bit-exact; lmfilter_rule.h is its one definition and states it in full: the kernels, the host twin and
 * tests/lmfilter_ref.py evaluate it; only + - * /, sqrtf, fabsf, comparisons and max; every fp32 operator is one IEEE binary32
 * operation, left to right).  In short:
 *  1. Entry i at texel texels[i]: e = rgb, l = luminance3(e), S = (float)samples, v = max((m2 - S*l*l) / (S - 1), 0) / S, the
 *     variance of the mean luminance.  An entry with a non-finite rgb, m2, position or normal (or a NaN v) is bad: its 16 input
 *     bytes are its output and it is never a tap.  Texel indices must be unique and < width * height: the twin refuses
 *     otherwise, the device skips an index out of range and lets one of several duplicates win, as PTResolveLightmap does.
 *  2. Footprint h2_p: the smallest |P_q - P_p|^2 > 0 over the covered, not bad 4-neighbours (left, right, up, down), else 0.  A
 *     texel with h2 == 0 is isolated: it keeps its e bit for bit and may still be a tap of others.
 *  3. Position cut: the tap at the offset (ox, oy) is admitted when |P_q - P_p|^2 <= (sigmaPosition * sigmaPosition) * h2_p *
 *     (float)(ox*ox + oy*oy); the offset (0, 0) always is.  This is what stops chart-to-chart bleeding.
 *  4. Level k = 0 ... iterations - 1, step s = 2^k: 5 x 5 taps at (dx, dy) * s, dy outer, dx inner, ascending, sums from 0 in that
 *     order; w = ((h[dx] * h[dy]) * w_n) * w_z * w_l with h = {1/16, 1/4, 3/8, 1/4, 1/16}; w_n = max(dot(N_p, N_q), 0) squared
 *     normalPower times; z = |dot(N_p, P_q - P_p)| / (sigmaPlane * sqrt(h2_p) * (float)s + 1e-12f), w_z = (1 / (1 + z*z))^2;
 *     x = |l_p - l_q| / (sigmaLuminance * sqrt(g_p) + 1e-6f), w_l = (1 / (1 + x*x))^2; g_p = the {1/4, 1/2, 1/4}^2 blur of v over
 *     the admitted taps of the 3 x 3 at step 1, divided by the weights it used, from the level's input.
 *     e' = sum(w * e_q) / sum(w); v' = sum(w*w * v_q) / (sum(w) * sum(w)); a texel whose sum(w) is not > 0 keeps (e, v).
 *  5. out[i].rgb = the final e; out[i].m2 = the final v: THE VARIANCE ESTIMATE OF THE FILTERED LUMINANCE, NOT A SUM OF SQUARES
 *     (a denoised list is not folded with further samples by m2).  iterations == 0: the input's rgb and the v of step 1.
 *     Nothing past `count` is written.
 *
 * PTDenoiseLightmap.  Device arrays (dTexels 4-byte, dRecv, dIrr and dOut 16-byte aligned); dOut may equal dIrr.  Stream-ordered
 * on the context's stream, does not synchronise, needs no scene.  Kernels: a scatter of the list into a state image (e, v) and
 * two guide images (P, h2) and (N, flags), the footprint, one launch per level between two state images, and a collect back
 * into the list.  Memory, in the context, grown on demand, kept across PTSetScene, freed by PTDestroy: 64 bytes per texel (two
 * 16-byte state images and 32 bytes of guides): 4.3 GB at 8192 x 8192.
 * Errors: PT_ERR_INVALID_ARG for a NULL context, params, or (count > 0) array; a misaligned pointer; a structSize below this
 * header's; samples outside 2 ... 2^24, iterations > 8, normalPower > 7; a sigma that is not finite and positive; a size outside
 * 1 ... 8192; count > width * height; a nonzero reserved word.  count == 0 returns PT_OK and launches nothing.  Arguments are
 * checked before the context is used.  No CPU fallback.
 * PTDenoiseLightmapHost: the host twin, no context, no GPU; returns 1, or 0 with PTGetBVHBuildError() set.
 * ===================================================================================================================== */
#define PT_LMFILTER_MAX_ITERATIONS   8u
#define PT_LMFILTER_MAX_NORMAL_POWER 7u
#define PT_LMFILTER_MAX_SAMPLES      16777216u

typedef struct PTLightmapDenoiseParams {
    uint32_t structSize;          /* sizeof(PTLightmapDenoiseParams) of the caller's header; members are only appended */
    uint32_t samples;             /* 2 ... 2^24: the total number of samples behind m2 */
    uint32_t iterations;          /* 0 ... 8 a-trous levels; suggested 5 */
    uint32_t normalPower;         /* 0 ... 7: the normal weight is the cosine squared that many times; suggested 5 */
    float    sigmaLuminance;      /* > 0, finite; suggested 4 */
    float    sigmaPosition;       /* > 0, finite; suggested 4 */
    float    sigmaPlane;          /* > 0, finite; suggested 1 */
    uint32_t reserved[5];         /* must be 0 */
} PTLightmapDenoiseParams;

#ifdef __cplusplus
static_assert(sizeof(PTLightmapDenoiseParams) == 48, "PTLightmapDenoiseParams is 48 bytes");
#else
_Static_assert(sizeof(PTLightmapDenoiseParams) == 48, "PTLightmapDenoiseParams is 48 bytes");
#endif

/* Device arrays, stream-ordered on the context's stream. */
PT_API int PTDenoiseLightmap(PTContext* ctx, const PTLightmapDenoiseParams* params, const uint32_t* dTexels, const PTReceiver* dRecv,
                             const PTIrradiance* dIrr, uint64_t count, uint32_t width, uint32_t height, PTIrradiance* dOut);
PT_API int PTDenoiseLightmapHost(const PTLightmapDenoiseParams* params, const uint32_t* texels, const PTReceiver* recv, const PTIrradiance* irr,
                                 uint64_t count, uint32_t width, uint32_t height, PTIrradiance* out);        /* host twin, no GPU */

/* =====================================================================================================================
 * Part 18: probe placement.  Part 16's probes sit on a regular grid, and in a real scene some of them land inside walls,
 * pillars and furniture.  A probe inside closed geometry sees no light: its coefficients are zero, its depth record holds
 * the inside of the object, and it darkens every point whose cell contains it.  A probe a few millimetres in front of a
 * wall wastes half of its sphere.  PTProbePlace is the short pass before the bake that fixes both: it traces a fixed set of
 * rays from each probe, counts the faces seen from behind, pushes the probe out of the object it is in or away from the
 * face it is too close to -- within its own cell --, and marks what stays buried; PTProbeGridIrradiancePlaced is Part 16's
 * lookup that honours the result.  An addition detected by symbol; PTGetVersion is unchanged.
 *
 * The rule (bit-exact; placement_rule.h is its one definition: the kernels, the host twins and tests/placement_ref.py
 * evaluate it; every fp32 operator below is one IEEE binary32 operation in the order written, no fma).
 *  - Limits.  lim[a] = maxOffset * spacing[a].  An offset o PASSES when |o[a]| <= lim[a] on every axis; a NaN fails.  A stored
 *    offset that does not pass is read as (0, 0, 0), whole.
 *  - One STEP for a probe {P, seed} whose stored offset reads o:
 *    1. O[a] = P[a] + o[a].  Sample j (0 <= j < samples) has Part 15's seeding and direction w_j for (seed, firstSample, j),
 *       word for word; every step uses the same directions.  Its ray is the PTRay {O, w_j, tmax = maxDistance, 0}, traced as a
 *       closest-hit query with PT_QUERY_SURFACE by Part 3's rules.
 *    2. Sample j is a HIT iff its PTRayHit.prim != 0xFFFFFFFF; only then is its PTRaySurface read (Part 3 leaves it
 *       untouched on a miss).  With n the record's normal: c = (w.x * n.x + w.y * n.y) + w.z * n.z.  The sample is BACK iff
 *       c > 0, otherwise FRONT: a NaN counts as front.
 *    3. back and front are the counts.  nearestBack is the back sample with the smallest (bits(t), j) in lexicographic order,
 *       bits(t) the uint32 pattern of the hit's t -- for the positive t a hit has, the order of the floats --; nearestFront
 *       the same among the front samples; farthestFront the front sample with the largest bits(t), the lowest j among equals.
 *       No floating-point sum is involved: counts, and exact selections.
 *    4. inside = (float)back > backfaceShare * (float)samples.
 *    5. The move (relocation steps only).  If inside: len = tNearestBack + minFrontDistance * 0.5f and
 *       cand[a] = o[a] + w_nb[a] * len -- through the nearest face seen from behind.  Else, if a front sample exists and
 *       tNearestFront < minFrontDistance: len = minFrontDistance - tNearestFront and cand[a] = o[a] - w_nf[a] * len --
 *       straight away from the nearest face.  Otherwise cand = o.  cand becomes the offset iff it passes the limits; a refused
 *       candidate leaves o as it was, bit for bit (what is stored is o as read: a stored offset that did not pass is
 *       stored back as 0).
 *  - PTProbePlace runs `iterations` relocation steps and then one more trace that only classifies: iterations + 1 traces;
 *    state (0 live, PT_PROBE_INSIDE) and the statistics describe the FINAL offset.  iterations == 0 classifies the grid
 *    positions.  It starts from o = 0 -- with PT_PLACE_KEEP_OFFSETS from the offsets already in dOut (read as above), which
 *    is how a caller places again after a geometry update.
 *  - PTProbePlaceStats (optional, one per probe, written by the last step only): the counts, the three sample indices
 *    (0xFFFFFFFF where there is none) and their t (0 where there is none).
 *  - The placed lookup is Part 16's with two changes.  A corner whose placement state has PT_PROBE_INSIDE is skipped exactly
 *    as a corner with tri == 0 is: it reads neither coefficients nor depth and adds nothing to sumW.  Otherwise step 4 (distance,
 *    direction, texel) uses Q[a] = Q_grid[a] + offset[a] (one add); tri stays the grid's.  With dPlacement == NULL the call IS
 *    PTProbeGridIrradiance, bit for bit (that path does not execute the add: (-0) + 0 would change a sign bit).
 *  - PTProbePlace: stream-ordered on the context's stream; no state set is involved, so it can run beside passes in flight.
 *    Chunks hold floor(2^20 / samples) whole probes, and a chunk goes through all its steps before the next one starts.  The
 *    rays, hit and surface records live in scratch the context keeps: 96 bytes per sample, 96 MB at most; growing it drains
 *    that stream.  PTStats moves as the iterations + 1 PTTraceRays(..., PT_QUERY_SURFACE) calls over the same rays move it.
 *  - Nothing past `count` is written.  Every device pointer is 16-byte aligned.
 *  - PT_ERR_INVALID_ARG for a NULL or misaligned pointer (dStats may be NULL), an unknown flag bit, a spacing that is not
 *    finite and positive, a maxDistance that is not finite, not positive or not below PT_FAR_PLANE, a minFrontDistance that is
 *    not finite and non-negative, a backfaceShare outside [0, 1], a maxOffset outside [0, 0.5), iterations > 16.
 *    PT_ERR_UNSUPPORTED for samples == 0 and samples > 65536.  PT_ERR_NO_SCENE for PTProbePlace before PTSetScene.
 *    count == 0 returns PT_OK and launches nothing.  Arguments are checked before the context is used.  No CPU fallback.
 *  - The host twins take no context and no GPU; they return 1, or 0 with PTGetBVHBuildError() set.  PTProbePlaceStepHost is
 *    ONE step over the hit and surface records of count x samples rays, entry-major, as PTTraceRaysHost returns them for the
 *    rays of step 1: inout[i].offset is read (as above) and, with move != 0, replaced; inout[i].state and stats[i] (stats may be
 *    NULL) describe the offset the records were traced from.  PTProbeGridIrradiancePlacedHost is PTProbeGridIrradiancePlaced.
 * ===================================================================================================================== */
#define PT_PROBE_INSIDE        1u /* PTProbePlacement.state: buried; the placed lookup leaves the probe out */
#define PT_PLACE_KEEP_OFFSETS  1u /* PTProbePlace flag: start from the offsets in dOut, not from 0 */
#define PT_PLACE_MAX_ITERATIONS 16u

typedef struct PTProbePlacement { /* 16 bytes: one 16-byte load */
    float    offset[3];           /* added to the grid position; |offset[a]| <= maxOffset * spacing[a] */
    uint32_t state;               /* 0 = live, PT_PROBE_INSIDE */
} PTProbePlacement;

typedef struct PTProbePlaceParams { /* 32 bytes; a host struct, passed by pointer */
    float    spacing[3];          /* the grid's spacing; finite, > 0 */
    float    maxDistance;         /* where a placement ray ends; finite, > 0, below PT_FAR_PLANE */
    float    minFrontDistance;    /* a probe closer than this to a face it sees from the front moves away; finite, >= 0 */
    float    backfaceShare;       /* [0, 1]: inside when more than this share of the samples are back */
    float    maxOffset;           /* [0, 0.5): the limit of an offset, a fraction of the spacing per axis */
    uint32_t iterations;          /* 0 ... 16 relocation steps */
} PTProbePlaceParams;

typedef struct PTProbePlaceStats { /* 32 bytes: two 16-byte stores */
    uint32_t back, front;         /* the counts of the last step */
    uint32_t nearestBack, nearestFront, farthestFront;       /* sample indices; 0xFFFFFFFF: none */
    float    tNearestBack, tNearestFront, tFarthestFront;    /* their t; 0: none */
} PTProbePlaceStats;

#ifdef __cplusplus
static_assert(sizeof(PTProbePlacement) == 16, "PTProbePlacement is 16 bytes");
static_assert(sizeof(PTProbePlaceParams) == 32, "PTProbePlaceParams is 32 bytes");
static_assert(sizeof(PTProbePlaceStats) == 32, "PTProbePlaceStats is 32 bytes");
#else
_Static_assert(sizeof(PTProbePlacement) == 16, "PTProbePlacement is 16 bytes");
_Static_assert(sizeof(PTProbePlaceParams) == 32, "PTProbePlaceParams is 32 bytes");
_Static_assert(sizeof(PTProbePlaceStats) == 32, "PTProbePlaceStats is 32 bytes");
#endif

/* Device pointers, stream-ordered on the context's stream. */
PT_API int PTProbePlace(PTContext* ctx, const PTProbe* dProbes, uint64_t count, uint32_t firstSample, uint32_t samples,
                        const PTProbePlaceParams* params, uint32_t flags, PTProbePlacement* dOut, PTProbePlaceStats* dStats /* may be NULL */);
/* Host arrays: staged through device buffers the context keeps and grows; synchronous. */
PT_API int PTProbePlaceHost(PTContext* ctx, const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples,
                            const PTProbePlaceParams* params, uint32_t flags, PTProbePlacement* out, PTProbePlaceStats* stats /* may be NULL */);
/* dSH, dDepth, dPlacement: one entry per probe of the grid; dQueries, dOut: count entries. */
PT_API int PTProbeGridIrradiancePlaced(PTContext* ctx, const PTProbeGrid* grid, const PTProbeCoeffs* dSH, const PTProbeDepthMap* dDepth,
                                       const PTProbePlacement* dPlacement /* NULL = PTProbeGridIrradiance */, const PTReceiver* dQueries,
                                       uint64_t count, PTIrradiance* dOut);
/* host twins, no GPU */
PT_API int PTProbePlaceStepHost(const PTProbe* probes, uint64_t count, uint32_t firstSample, uint32_t samples, const PTProbePlaceParams* params,
                                const PTRayHit* hits, const PTRaySurface* surfaces, int move, PTProbePlacement* inout,
                                PTProbePlaceStats* stats /* may be NULL */);
PT_API int PTProbeGridIrradiancePlacedHost(const PTProbeGrid* grid, const PTProbeCoeffs* sh, const PTProbeDepthMap* depth,
                                           const PTProbePlacement* placement /* NULL = PTProbeGridIrradianceHost */, const PTReceiver* queries,
                                           uint64_t count, PTIrradiance* out);

/* =====================================================================================================================
 * Part 19: adaptive gathers.  Part 13 gives every receiver the same `samples`, whether it sits in plain view of a point light
 * or in a corner only third-bounce light reaches.  PTGatherIrradianceAdaptive is the loop the render has for frames (Parts 6
 * and 7), for lists: gather a few samples of every entry, keep the entries whose mean luminance is still noisy, gather more of
 * those only, until none is left.  PTIrradiance.m2 carries what the decision needs, Part 13's seeding makes [a, a + n) the same
 * samples however it is cut into calls, and every round IS a PTGatherIrradiance over a compacted list -- no gather kernel knows
 * of this part.  An addition detected by symbol; PTGetVersion is unchanged.
 *
 * The rule (bit-exact; adaptive_gather_rule.h is its one definition: the kernels, the host twins and tests/adaptive_gather_ref.py
 * evaluate it; only + - * /, max and comparisons; every fp32 operator is one IEEE binary32 operation, left to right, no fma).
 *  1. Rounds.  Round 0 gathers the samples [firstSample, firstSample + minSamples) of every entry; round r >= 1 gathers
 *     [firstSample + minSamples + (r - 1) * addSamples, ... + addSamples) of the entries still active (uint32 arithmetic, as
 *     Part 13's seeding).  Each round is exactly PTGatherIrradiance over the active entries' 32 receiver bytes, copied unchanged
 *     (the seed travels with them).  An entry that is dropped stays dropped, so every active entry of a round holds the same
 *     count n.
 *  2. Select, for an active entry with accumulated (rgb, m2) and count n:  S = (float)n;  l = luminance3(rgb);
 *     v = max((m2 - S*l*l) / (S - 1), 0) / S  (Part 17's step 1, word for word);  d = max(l, darkFloor);
 *     noisy = v > (threshold * threshold) * (d * d).  In this order: an entry whose rgb or m2 is not finite stops as NON-FINITE;
 *     one that is not noisy (a NaN v compares false) stops BY THRESHOLD; one with n + addSamples > maxSamples stops BY MAXSAMPLES;
 *     every other entry stays active.  The next active list is the surviving entry indices in the order of the list they were
 *     selected from (ascending for the loop): a stable compaction, so the result does not depend on launch geometry.  The
 *     survivors' receivers go beside them in the same order.
 *  3. Fold of a round's result (rgb_new, m2_new) of m samples into (rgb, m2) of n samples:
 *     rgb' = (rgb * (float)n + rgb_new * (float)m) / (float)(n + m) per channel;  m2' = m2 + m2_new;  n' = n + m  (the
 *     running-mean form of Part 7).  n == 0 writes: the round's result is the entry, bit for bit.
 *  4. Result.  out[i] is the accumulated PTIrradiance, counts[i] = n_i.  The loop ends when the active list is empty.
 *  5. Equalise (optional): what lets the denoiser and any other consumer that assumes ONE `samples` take the list.  For a chosen
 *     samplesEq (2 ... 2^24), with l and v as in step 2 from (rgb, m2, n_i):  out.rgb = rgb;
 *     out.m2 = S*l*l + (v*S) * (S - 1)  with S = (float)samplesEq, so that Part 17's step 1 at samples = samplesEq recovers the
 *     entry's own variance of the mean.  An entry with a non-finite rgb or m2, or with n_i outside 2 ... 2^24, passes through byte
 *     for byte.  THIS IS A REWRITE OF m2, NOT NEW STATISTICS: an equalised list is not folded with further samples.
 * Like every variance-led stop, the decision uses the very samples it stops on, so among equally noisy entries those whose
 * first samples happen to agree stop first: the estimate is slightly biased towards stopping early.  minSamples is the guard.
 * Because a gather of an entry does not depend on its neighbours in the list (Part 13), (out[i], counts[i]) equals what steps 2
 * and 3 make of PTGatherIrradiance results for the same receiver over the same sample ranges, bit for bit.
 *
 * PTGatherIrradianceAdaptive: the whole loop.  Each round enqueues the gather as Part 13 does (the same chunks, state sets and
 * PTStats accounting), folds, selects, and reads the survivor and stop counts back (32 bytes): one synchronisation per round; it
 * returns synchronised.  dCounts and outStats may be NULL.  Working memory in the context, grown on demand, kept across
 * PTSetScene, freed by PTDestroy: 56 bytes per entry (two index lists of 4, one compacted receiver list of 32, one round-result
 * list of 16) and 16 bytes per 256 entries.  PTGatherIrradianceAdaptiveHost: host arrays, staged like PTGatherIrradianceHost.
 * The steps, for callers that drive rounds themselves, on device arrays, stream-ordered on the context's stream (no scene needed):
 *  - PTSelectReceivers: step 2 over the list dActive[0 .. activeCount) (NULL: every entry 0 .. activeCount - 1) with the count n;
 *    dAcc and dRecv hold entryCount entries and are read through the index; an index >= entryCount is left out (and counted
 *    nowhere).  Writes the survivors to dOutActive / dOutRecv (activeCount entries each; nothing past the survivor count is
 *    written; neither may alias an input), their number to *survivors and, if given, stopped[3] = by threshold, by maxSamples,
 *    non-finite.  Synchronises (the counts are read back).
 *  - PTFoldIrradiance: step 3; dNew[k] (m samples) folds into dAcc[dActive[k]] (n samples; n == 0 writes), and dCounts (may be
 *    NULL) gets n + m there.  Indices are unique; n + m <= 2^24.
 *  - PTEqualiseIrradiance: step 5; dOut may equal dIrr.
 * Errors: PT_ERR_INVALID_ARG for a NULL or misaligned pointer (indices and counts 4 bytes, the rest 16), a structSize below this
 * header's, a nonzero reserved word, minSamples outside 2 ... 65536, addSamples outside 1 ... 65536, maxSamples outside
 * minSamples ... 2^24, a threshold that is not finite and > 0, a darkFloor that is not finite and >= 0, n outside 2 ... 2^24
 * (select), m outside 1 ... 65536 or n + m > 2^24 (fold), samplesEq outside 2 ... 2^24, activeCount > entryCount, more than 2^31
 * entries, (PTGatherIrradianceAdaptiveHost) a nonzero PTReceiver.reserved; the offending number is in PTGetLastError.
 * PT_ERR_UNSUPPORTED for schedules 0 and 4 and MaxRayBounces > 8191, PT_ERR_NO_SCENE before PTSetScene (the loop only).
 * count == 0 returns PT_OK and launches nothing.  Arguments are checked before the context is used.  Nothing past `count` is
 * written.  No CPU fallback.  The host twins take no context and no GPU; they return 1, or 0 with PTGetBVHBuildError() set, and
 * also refuse an index >= entryCount.
 * ===================================================================================================================== */
#define PT_ADAPTIVE_GATHER_MAX_TOTAL   16777216u    /* 2^24: every count is exact in fp32 */
#define PT_ADAPTIVE_GATHER_MAX_ENTRIES 2147483648u  /* 2^31 */

typedef struct PTAdaptiveGather { /* a host struct, passed by pointer */
    uint32_t structSize;          /* sizeof(PTAdaptiveGather) of the caller's header; members are only appended */
    uint32_t firstSample;         /* first sample index of the call */
    uint32_t minSamples;          /* 2 ... PT_GATHER_MAX_SAMPLES: round 0 */
    uint32_t addSamples;          /* 1 ... PT_GATHER_MAX_SAMPLES: every later round */
    uint32_t maxSamples;          /* minSamples ... 2^24: no entry gets more */
    float    threshold;           /* finite, > 0: the relative standard error of the mean luminance to reach */
    float    darkFloor;           /* finite, >= 0: below this luminance the error is measured against darkFloor */
    uint32_t reserved[5];         /* must be 0 */
} PTAdaptiveGather;

typedef struct PTAdaptiveGatherStats {
    uint32_t rounds;              /* gathers run */
    uint32_t maxCount;            /* the largest counts[i] */
    uint64_t samples;             /* samples gathered over all entries and rounds (the paths PTStats counted) */
    uint64_t stoppedThreshold;    /* entries stopped by threshold, */
    uint64_t stoppedMaxSamples;   /*   by maxSamples, */
    uint64_t stoppedNonFinite;    /*   as non-finite: the three add up to count */
} PTAdaptiveGatherStats;

#ifdef __cplusplus
static_assert(sizeof(PTAdaptiveGather) == 48, "PTAdaptiveGather is 48 bytes");
static_assert(sizeof(PTAdaptiveGatherStats) == 40, "PTAdaptiveGatherStats is 40 bytes");
#else
_Static_assert(sizeof(PTAdaptiveGather) == 48, "PTAdaptiveGather is 48 bytes");
_Static_assert(sizeof(PTAdaptiveGatherStats) == 40, "PTAdaptiveGatherStats is 40 bytes");
#endif

/* Device pointers; returns synchronised. */
PT_API int PTGatherIrradianceAdaptive(PTContext* ctx, const PTFrameParams* params, const PTAdaptiveGather* adaptive, const PTReceiver* dRecv,
                                      uint64_t count, PTIrradiance* dOut, uint32_t* dCounts /* may be NULL */,
                                      PTAdaptiveGatherStats* outStats /* host, may be NULL */);
/* Host arrays: staged through device buffers the context keeps and grows; synchronous. */
PT_API int PTGatherIrradianceAdaptiveHost(PTContext* ctx, const PTFrameParams* params, const PTAdaptiveGather* adaptive, const PTReceiver* recv,
                                          uint64_t count, PTIrradiance* out, uint32_t* counts /* may be NULL */,
                                          PTAdaptiveGatherStats* outStats /* may be NULL */);
/* the steps: device arrays, stream-ordered on the context's stream */
PT_API int PTSelectReceivers(PTContext* ctx, const PTAdaptiveGather* adaptive, uint32_t n, const uint32_t* dActive /* NULL = every entry */,
                             uint64_t activeCount, const PTIrradiance* dAcc, const PTReceiver* dRecv, uint64_t entryCount, uint32_t* dOutActive,
                             PTReceiver* dOutRecv, uint64_t* survivors /* host */, uint64_t* stopped /* host, 3 words, may be NULL */);
PT_API int PTFoldIrradiance(PTContext* ctx, const uint32_t* dActive /* NULL = every entry */, uint64_t activeCount, const PTIrradiance* dNew,
                            uint32_t m, uint32_t n, uint64_t entryCount, PTIrradiance* dAcc, uint32_t* dCounts /* may be NULL */);
PT_API int PTEqualiseIrradiance(PTContext* ctx, const PTIrradiance* dIrr, const uint32_t* dCounts, uint64_t count, uint32_t samplesEq,
                                PTIrradiance* dOut);
/* host twins, no GPU */
PT_API int PTSelectReceiversHost(const PTAdaptiveGather* adaptive, uint32_t n, const uint32_t* active /* NULL = every entry */, uint64_t activeCount,
                                 const PTIrradiance* acc, const PTReceiver* recv, uint64_t entryCount, uint32_t* outActive, PTReceiver* outRecv,
                                 uint64_t* survivors, uint64_t* stopped /* 3 words, may be NULL */);
PT_API int PTFoldIrradianceHost(const uint32_t* active /* NULL = every entry */, uint64_t activeCount, const PTIrradiance* fresh, uint32_t m,
                                uint32_t n, uint64_t entryCount, PTIrradiance* acc, uint32_t* counts /* may be NULL */);
PT_API int PTEqualiseIrradianceHost(const PTIrradiance* irr, const uint32_t* counts, uint64_t count, uint32_t samplesEq, PTIrradiance* out);

/* =====================================================================================================================
 * Part 20: reflection probes.  Lightmaps (Part 14) and SH probes (Parts 15, 16) carry cosine-convolved light: they are diffuse.
 * What a glossy or metallic object that moves through the baked scene reads is a reflection probe: a radiance map around a point,
 * prefiltered once per roughness level, so that one fetch answers "what does a surface of roughness r reflect from direction R".
 * The host hands over positions and a sample range; the directions, the paths, the fold, the GGX prefilter and the lookup run on
 * the GPU.  An addition beside the reference's ABI, detected by symbol; PTGetVersion is unchanged.
 *
 * Layout.  A probe's map has `levels` levels; level k is an (R >> k) x (R >> k) octahedral image of 16-byte PTReflectionTexel,
 * texel index v * Rk + u with Rk = R >> k; the levels are concatenated in ascending k, the probes' maps are concatenated.  R =
 * `res` is a power of two in [8, 256]; 2 <= levels <= log2(R) - 1, so the coarsest level is at least 4 x 4 (a 2 x 2 level has all
 * four centres on the equator and cannot tell up from down).  Level k stands for roughness rho_k = (float)k / (float)(levels - 1).
 * A base map (what the capture writes, what the prefilter reads) is level 0 alone: R * R texels per probe.
 *
 * The rule (bit-exact; reflection_rule.h is its one definition: the kernels, the host twins and tests/reflection_ref.py evaluate
 * it; every fp32 operator below is one IEEE binary32 operation in the order written, no fma).
 *  1. Texel directions.  direction(R, u, v, su, sv): a = (((float)u + su) / (float)R) * 2.0f - 1.0f, b likewise from v and sv.
 *     z = (1.0f - |a|) - |b|.  If z < 0: x = (1.0f - |b|) * sgn(a), y = (1.0f - |a|) * sgn(b), with sgn(0) = +1; otherwise x = a,
 *     y = b.  len = sqrt((x * x + y * y) + z * z); d = (x / len, y / len, z / len).  A centre has su = sv = 0.5f.
 *     oct_coords(D): s = (|D.x| + |D.y|) + |D.z|, a = D.x / s, b = D.y / s; if D.z < 0: a' = (1.0f - |b|) * sgn(a),
 *     b' = (1.0f - |a|) * sgn(b).  D need not be of unit length.
 *  2. Capture.  Slot (i * R * R + t) * samples + j is sample j of texel t = v * R + u of probe i.  Seeding (uint32 arithmetic):
 *     s = seed_i; pt_rng_next(&s); s += t; pt_rng_next(&s); s += firstSample + j.  Two draws r1, r2 (pt_random_float) give the
 *     direction d = direction(R, u, v, r1, r2): a jittered point of the texel.  (float)u + r1 may round up to u + 1 (r1 lies in
 *     [0, 1]): the direction then lies on the texel's edge, never beyond it.  The ray is the PTRadianceRay {P_i, d, the RNG state
 *     after the two draws, 0}, and the path is PTTraceRadiance's (Part 8) under `params` with SamplesPerPass forced to 1: L_j is
 *     the path's colour.  The texel is rgb[c] = (the sum over ascending j of L_j[c], from +0.0f) / (float)samples, and aux = the
 *     sum over ascending j of lum_j * lum_j with lum = (L.r * 0.299f + L.g * 0.587f) + L.b * 0.114f, unscaled (a later fold of
 *     two sample ranges can use it).  Samples are independent: PTReflectionRays writes the rays alone and needs no scene.
 *  3. Prefilter.  Level 0 is the base, copied bit for bit.  For level k >= 1: alpha = rho_k * rho_k; a2 = alpha * alpha;
 *     g = a2 - 1.0f.  Output texel o has the centre direction n at R >> k.  It walks the base texels s = 0 ... R * R - 1 in
 *     ascending order: l, len = s's centre at R and J = 1.0f / ((len * len) * len), the octahedral map's solid-angle Jacobian;
 *     c = (n.x * l.x + n.y * l.y) + n.z * l.z; s is skipped unless c > 0; h = (1.0f + c) * 0.5f; t = h * g + 1.0f;
 *     w = (c * J) / (t * t); acc[ch] = acc[ch] + w * base[s].rgb[ch]; sw = sw + w, all from +0.0f.  Then rgb = acc / sw and
 *     aux = sw.  This is the GGX split-sum prefilter with N = V = R in the distribution's rational form: no exp, no pow.  One
 *     lane owns one output texel, so no cross-lane fold enters the rule.  A NaN or Inf in an unskipped base texel propagates.
 *  4. Lookup of the query {position P, roughness, direction, probe}, in this order:
 *     a. probe >= probeCount yields zeros (aux too) and reads nothing.
 *     b. D = direction, used as given.
 *     c. Box projection, only with dBoxes != NULL (dProbes then gives the probes' positions Q) and only if
 *        bmin[a] <= P[a] <= bmax[a] on all three axes: t = +inf; for each axis in x, y, z with D[a] > 0,
 *        t = min(t, (bmax[a] - P[a]) / D[a]); with D[a] < 0, t = min(t, (bmin[a] - P[a]) / D[a]).  If t is finite and > 0:
 *        v[a] = (P[a] + D[a] * t) - Q[a]; r = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); if r > 0, D = v / r.  Otherwise D
 *        keeps its bits.
 *     d. (a, b) = oct_coords(D).
 *     e. r = roughness > 0 ? roughness : 0 (a NaN lands on 0); r = r < 1 ? r : 1; lam = r * (float)(levels - 1);
 *        k0 = min((uint32_t)lam, levels - 2); f = lam - (float)k0.
 *     f. In each of the levels k0 and k0 + 1, bilinear: x = (a * 0.5f + 0.5f) * (float)Rk - 0.5f; x0 = floor(x) (held to
 *        [-1, Rk - 1], which every a in [-1, 1] gives anyway); fx = x - x0; y likewise from b.  The taps (x0 + dx, y0 + dy), dy
 *        outer, go through the octahedral wrap: a tap with x outside [0, Rk) becomes x' = x < 0 ? -1 - x : 2 * Rk - 1 - x and
 *        y' = Rk - 1 - y; then the same test and rule run on y, mirroring x.  Every lerp is p + f * (q - p) -- equal taps give
 *        their value exactly --: first along x in both rows, then along y.
 *     g. rgb = A + f * (B - A) with A from level k0 and B from level k0 + 1; aux = 1.0f.
 *
 * Device pointers are 16-byte aligned; the calls are stream-ordered on the context's stream and nothing past `count` is written.
 * PTReflectionCapture walks the list in slabs of whole texels of at most 2^22 slots through scratch the context keeps and grows
 * (48 bytes per slot: the ray and its radiance; kept across PTSetScene, freed by PTDestroy): per slab the rays, PTTraceRadiance's
 * launch sequences over them (chunks of 2^21 on successive state sets, joined by the context's stream), the fold.
 * PTStats: paths grows by count * res * res * samples; pixel counters do not move.  With profiling on, every radiance chunk is
 * one entry of PTGetTimings.  PTReflectionPrefilter and PTReflectionLookup need no scene.
 * Errors: PT_ERR_INVALID_ARG for a NULL or misaligned pointer, a res or levels outside the ranges above, boxes without probes,
 * dOutMaps overlapping dBase; PT_ERR_UNSUPPORTED for schedules 0 and 4, samples == 0, samples > 65536 and MaxRayBounces > 8191;
 * PT_ERR_NO_SCENE for the capture before PTSetScene.  count == 0 returns PT_OK and launches nothing.  Arguments are checked
 * before the context is used.  No CPU fallback.
 * The host twins take no context and no GPU; they return 1, or 0 with PTGetBVHBuildError() set.  PTReflectionDirectionsHost
 * writes PTReflectionRays' entries; PTReflectionFoldHost folds count * res * res * samples PTRadiance entries, slot-major, into
 * base texels; PTReflectionPrefilterHost and PTReflectionLookupHost are the device calls.
 * ===================================================================================================================== */
typedef struct PTReflectionTexel {  /* 16 bytes */
    float    rgb[3];
    float    aux;                 /* base: sum of squared luminances; level k >= 1: the weight sum; a lookup: 1 */
} PTReflectionTexel;

typedef struct PTReflectionQuery {  /* 32 bytes: two 16-byte loads */
    float    position[3];         /* read only by the box projection */
    float    roughness;           /* clamped to [0, 1] */
    float    direction[3];        /* the reflection direction, used as given */
    uint32_t probe;               /* index into the maps */
} PTReflectionQuery;

typedef struct PTReflectionBox {    /* 32 bytes: the box a probe's map stands for */
    float    bmin[3];
    float    pad0;
    float    bmax[3];
    float    pad1;
} PTReflectionBox;

#ifdef __cplusplus
static_assert(sizeof(PTReflectionTexel) == 16, "PTReflectionTexel is 16 bytes");
static_assert(sizeof(PTReflectionQuery) == 32, "PTReflectionQuery is 32 bytes");
static_assert(sizeof(PTReflectionBox) == 32, "PTReflectionBox is 32 bytes");
#else
_Static_assert(sizeof(PTReflectionTexel) == 16, "PTReflectionTexel is 16 bytes");
_Static_assert(sizeof(PTReflectionQuery) == 32, "PTReflectionQuery is 32 bytes");
_Static_assert(sizeof(PTReflectionBox) == 32, "PTReflectionBox is 32 bytes");
#endif

/* dRays: count * res * res * samples entries, slot-major. */
PT_API int PTReflectionRays(PTContext* ctx, const PTFrameParams* params, const PTProbe* dProbes, uint64_t count, uint32_t res, uint32_t firstSample,
                            uint32_t samples, PTRadianceRay* dRays);
/* dOutBase: count * res * res base texels. */
PT_API int PTReflectionCapture(PTContext* ctx, const PTFrameParams* params, const PTProbe* dProbes, uint64_t count, uint32_t res, uint32_t firstSample,
                               uint32_t samples, PTReflectionTexel* dOutBase);
/* Host arrays: staged through device buffers the context keeps and grows; synchronous. */
PT_API int PTReflectionCaptureHost(PTContext* ctx, const PTFrameParams* params, const PTProbe* probes, uint64_t count, uint32_t res, uint32_t firstSample,
                                   uint32_t samples, PTReflectionTexel* outBase);
/* dBase: count base maps; dOutMaps: count whole maps, which must not overlap dBase. */
PT_API int PTReflectionPrefilter(PTContext* ctx, const PTReflectionTexel* dBase, uint64_t count, uint32_t res, uint32_t levels, PTReflectionTexel* dOutMaps);
/* dMaps: probeCount whole maps; dProbes, dBoxes: probeCount entries or NULL (boxes need probes); dQueries, dOut: count entries. */
PT_API int PTReflectionLookup(PTContext* ctx, const PTReflectionTexel* dMaps, uint64_t probeCount, uint32_t res, uint32_t levels, const PTProbe* dProbes,
                              const PTReflectionBox* dBoxes, const PTReflectionQuery* dQueries, uint64_t count, PTReflectionTexel* dOut);
/* host twins, no GPU */
PT_API int PTReflectionDirectionsHost(const PTProbe* probes, uint64_t count, uint32_t res, uint32_t firstSample, uint32_t samples, PTRadianceRay* rays);
PT_API int PTReflectionFoldHost(const PTRadiance* radiance, uint64_t count, uint32_t res, uint32_t samples, PTReflectionTexel* out);
PT_API int PTReflectionPrefilterHost(const PTReflectionTexel* base, uint64_t count, uint32_t res, uint32_t levels, PTReflectionTexel* outMaps);
PT_API int PTReflectionLookupHost(const PTReflectionTexel* maps, uint64_t probeCount, uint32_t res, uint32_t levels, const PTProbe* probes,
                                  const PTReflectionBox* boxes, const PTReflectionQuery* queries, uint64_t count, PTReflectionTexel* out);

/* =====================================================================================================================
 * Part 21: shading from the bakes.  Parts 13 to 20 bake diffuse and glossy light; this part uses it: the first hit of a ray is
 * shaded from a probe volume (Parts 16, 18) and reflection probes (Part 20) with the split-sum approximation -- a view of the
 * scene lit by the bakes, a way to check a bake by eye, a preview while the path tracer converges.  An addition beside the
 * reference's ABI, detected by symbol; PTGetVersion is unchanged.
 *
 * Left out: transmission, clearcoat, sheen, anisotropy and alpha cut-outs are ignored (every hit is opaque, the specular lobe
 * isotropic GGX over a Lambert base); one reflection probe per point, no blend; a miss is black; lights are seen only through the
 * bakes.
 *
 * The rule (bit-exact; shade_rule.h is its one definition: the kernels, the host twins and tests/shade_ref.py evaluate it; every
 * fp32 operator below is one IEEE binary32 operation in the order written, no fma; only + - * /, sqrt and comparisons).
 *  1. The DFG table: res x res entries {A, B} of two floats, res in {16, 32, 64}, entry j * res + i.
 *     mu = ((float)i + 0.5f) / (float)res is N.V; rho = ((float)j + 0.5f) / (float)res is perceptual roughness; alpha = rho * rho
 *     (Part 20's level roughness); a2 = alpha * alpha.  V = (sqrt(1.0f - mu * mu), 0, mu).
 *     smith_g(c, alpha): a = alpha * alpha; b = c * c; (2.0f * c) / (c + sqrt((a + b) - a * b)) -- the render's.
 *     Sample (p, q), p radial and q azimuth, both 0 ... 63: xi = ((float)p + 0.5f) / 64.0f;
 *     c2 = (1.0f - xi) / (1.0f + (a2 - 1.0f) * xi); s = sqrt(1.0f - c2); H = (s * C[q], s * S[q], sqrt(c2)), where C[q] and S[q]
 *     are float literals: cos and sin of 2 pi (q + 0.5) / 64 in float64, rounded to float.  vh = V.x * H.x + V.z * H.z;
 *     L.z = (2.0f * vh) * H.z - V.z; nl = L.z.  The sample counts only if nl > 0 and vh > 0: G = smith_g(mu, alpha) *
 *     smith_g(nl, alpha); gv = (G * vh) / (H.z * mu); m = 1.0f - vh; m2 = m * m; Fc = (m2 * m2) * m; a = a + (1.0f - Fc) * gv;
 *     b = b + Fc * gv.  Lane q sums its 64 radial samples in ascending p from +0.0f; the 64 lane partials are folded by Part 15's
 *     tree (h = 32, 16, ..., 1: v[l] = v[l] + v[l + h] for l < h); A = a / 4096.0f, B = b / 4096.0f.
 *  2. Terms of entry i from its ray, hit and surface record.  prim == 0xFFFFFFFF (a miss): material, terms and receiver are all
 *     zero bits but material.flags = PT_SHADE_MISS and material.materialIndex = 0xFFFFFFFF; the query is zero but probe =
 *     0xFFFFFFFF.  Otherwise the material record is what the render's material fetch returns for the hit (textures included):
 *     baseColor, metallic, emission, roughness (the render's alpha, >= 0.001), occlusion, opacity, the material index, flags 0.
 *     A surface record whose materialIndex is not below the scene's material count is taken as a miss.
 *     len = sqrt((D.x * D.x + D.y * D.y) + D.z * D.z); Vd = (-D) / len, per component.  d = (N.x * Vd.x + N.y * Vd.y) + N.z * Vd.z
 *     with N = PTRaySurface.normal; if d < 0, N = -N and d is taken again from the new N.  nDotV = max(d, 1e-4f).
 *     R = (2.0f * d) * N - Vd.  diffuse = baseColor * (1.0f - metallic); f0 = 0.04f + metallic * (baseColor - 0.04f);
 *     rho = sqrt(roughness); emission and occlusion are copied.  The receiver is {position, seed 0, N, 0}; the query is
 *     {position, rho, R, probe}.
 *     Probe choice.  d2_k = (v.x * v.x + v.y * v.y) + v.z * v.z with v = position - probe_k.  With boxes: among the probes k, in
 *     ascending k, with bmin_k[a] <= position[a] <= bmax_k[a] on all three axes, the first one, then any with d2_k < the best so
 *     far (a tie keeps the lower index).  If none was found, or without boxes: the same over all probes.  probeCount == 0 gives
 *     0xFFFFFFFF, which Part 20 step 4a answers with zeros.
 *  3. Compose.  An entry whose terms have nDotV > 0 false (a miss) gives {0, 0, 0, 0}.  Otherwise, on each table axis with
 *     v = nDotV (x) and v = rho (y): x = v * (float)res - 0.5f; x = x > 0 ? x : 0 (a NaN lands on 0); x = x < (float)(res - 1) ? x :
 *     (float)(res - 1); x0 = min((uint32_t)x, res - 2); fx = x - (float)x0.  (A, B) = the lerp along y of the lerps along x of the
 *     entries (x0, y0), (x0 + 1, y0) and (x0, y0 + 1), (x0 + 1, y0 + 1); every lerp is p + f * (q - p).  Per channel c:
 *     out[c] = emission[c] + occlusion * ((diffuse[c] * E[c]) * 0.31830988618379067f + spec[c] * (f0[c] * A + B)), E the
 *     PTIrradiance's rgb and spec the PTReflectionTexel's; out[3] = 1.0f.
 *  4. PTShadeBaked is steps 2 and 3 around Part 16's lookup (Part 18's when dPlacement is given) of the receiver and Part 20's
 *     lookup of the query, one lane per entry, nothing in between stored: it equals PTShadeSurfaces, PTProbeGridIrradiancePlaced,
 *     PTReflectionLookup and PTShadeCompose bit for bit.
 *  5. PTShadeBakedFrame: for pixel (x, y) the ray of Part 4's guides at one sample per pixel -- origin CamToWorld * (0, 0, 0, 1),
 *     direction normalize(CamToWorld * (CamInvProj * (u, v, 0, 1)).xyz0) with u = ((float)x + 0.5f) / (float)W * 2.0f - 1.0f, v
 *     likewise from y and H, tmax PT_FAR_PLANE --, PTTraceRays(PT_QUERY_CLOSEST | PT_QUERY_SURFACE), PTShadeBaked; pixel y * W + x
 *     of dOut.  dOutRays (may be NULL) receives the W * H PTRay entries.  The rays, hits and surface records go through scratch the
 *     context keeps and grows (96 bytes per pixel; kept across PTSetScene, freed by PTDestroy).
 *
 * Device pointers are 16-byte aligned (the DFG table 8); the calls are stream-ordered on the context's stream and nothing past
 * `count` is written.  Errors: PT_ERR_INVALID_ARG for a NULL or misaligned pointer, a DFG res outside {16, 32, 64}, a map res or
 * levels outside Part 20's ranges, a grid Part 16 refuses, PT_GRID_VISIBILITY without depth, boxes without probes;
 * PT_ERR_NO_SCENE for PTShadeSurfaces, PTShadeBaked and PTShadeBakedFrame before PTSetScene.  count == 0 returns PT_OK and
 * launches nothing.  Arguments are checked before the context is used.  No CPU fallback.
 * The host twins take no context and no GPU; they return 1, or 0 with PTGetBVHBuildError() set.  PTShadeTermsHost is step 2 after
 * the material fetch: it takes the material records PTShadeSurfaces returned.
 * ===================================================================================================================== */
#define PT_SHADE_MISS 1u            /* PTShadeMaterial.flags */

typedef struct PTShadeDFG {         /* 8 bytes: scale and bias of F0 */
    float    a, b;
} PTShadeDFG;

typedef struct PTShadeMaterial {    /* 48 bytes: three 16-byte stores */
    float    baseColor[3]; float    metallic;
    float    emission[3];  float    roughness;       /* the render's alpha */
    float    occlusion;    float    opacity;  uint32_t materialIndex;  uint32_t flags;       /* PT_SHADE_MISS */
} PTShadeMaterial;

typedef struct PTShadeTerms {       /* 48 bytes: three 16-byte loads */
    float    diffuse[3];   float    rho;             /* perceptual roughness */
    float    f0[3];        float    nDotV;           /* >= 1e-4 on a hit, 0 on a miss */
    float    emission[3];  float    occlusion;
} PTShadeTerms;

typedef struct PTShadeInputs {      /* 120 bytes; a host struct, passed by pointer */
    PTProbeGrid grid;                           /* Part 16; flags and normalBias as PTProbeGridIrradiance reads them */
    const PTProbeCoeffs*     dSH;
    const PTProbeDepthMap*   dDepth;            /* may be NULL without PT_GRID_VISIBILITY */
    const PTProbePlacement*  dPlacement;        /* may be NULL: Part 16's lookup */
    const PTReflectionTexel* dMaps;             /* probeCount whole maps; may be NULL with probeCount == 0 */
    const PTProbe*           dProbes;           /* probeCount entries; may be NULL with probeCount == 0 */
    const PTReflectionBox*   dBoxes;            /* may be NULL: no box rule in the choice, no box projection */
    const PTShadeDFG*        dDFG;              /* dfgRes * dfgRes entries */
    uint32_t probeCount, res, levels;           /* Part 20's layout */
    uint32_t dfgRes;
} PTShadeInputs;

#ifdef __cplusplus
static_assert(sizeof(PTShadeDFG) == 8, "PTShadeDFG is 8 bytes");
static_assert(sizeof(PTShadeMaterial) == 48, "PTShadeMaterial is 48 bytes");
static_assert(sizeof(PTShadeTerms) == 48, "PTShadeTerms is 48 bytes");
static_assert(sizeof(PTShadeInputs) == 120, "PTShadeInputs is 120 bytes");
#else
_Static_assert(sizeof(PTShadeDFG) == 8, "PTShadeDFG is 8 bytes");
_Static_assert(sizeof(PTShadeMaterial) == 48, "PTShadeMaterial is 48 bytes");
_Static_assert(sizeof(PTShadeTerms) == 48, "PTShadeTerms is 48 bytes");
_Static_assert(sizeof(PTShadeInputs) == 120, "PTShadeInputs is 120 bytes");
#endif

/* dOut: res * res entries. */
PT_API int PTBakeDFG(PTContext* ctx, uint32_t res, PTShadeDFG* dOut);
/* dRays, dHits, dSurface: what PTTraceRays(PT_QUERY_CLOSEST | PT_QUERY_SURFACE) read and wrote; dProbes, dBoxes: probeCount entries
 * or NULL (boxes need probes); each output has count entries or is NULL. */
PT_API int PTShadeSurfaces(PTContext* ctx, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count, const PTProbe* dProbes,
                           const PTReflectionBox* dBoxes, uint32_t probeCount, PTShadeMaterial* dOutMaterial, PTShadeTerms* dOutTerms,
                           PTReceiver* dOutReceivers, PTReflectionQuery* dOutQueries);
/* dOut: count float4 entries. */
PT_API int PTShadeCompose(PTContext* ctx, const PTShadeTerms* dTerms, const PTIrradiance* dIrradiance, const PTReflectionTexel* dReflection, uint64_t count,
                          const PTShadeDFG* dDFG, uint32_t dfgRes, float* dOut);
PT_API int PTShadeBaked(PTContext* ctx, const PTShadeInputs* inputs, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count,
                        float* dOut);
/* dOut: OutputWidth * OutputHeight float4 entries; dOutRays: as many PTRay entries, or NULL. */
PT_API int PTShadeBakedFrame(PTContext* ctx, const PTFrameParams* params, const PTShadeInputs* inputs, float* dOut, PTRay* dOutRays);
/* host twins, no GPU */
PT_API int PTBakeDFGHost(uint32_t res, PTShadeDFG* out);
PT_API int PTShadeTermsHost(const PTShadeMaterial* materials, const PTRay* rays, const PTRaySurface* surface, uint64_t count, const PTProbe* probes,
                            const PTReflectionBox* boxes, uint32_t probeCount, PTShadeTerms* outTerms, PTReceiver* outReceivers,
                            PTReflectionQuery* outQueries);
PT_API int PTShadeComposeHost(const PTShadeTerms* terms, const PTIrradiance* irradiance, const PTReflectionTexel* reflection, uint64_t count,
                              const PTShadeDFG* dfg, uint32_t dfgRes, float* out);

/* =====================================================================================================================
 * Part 22: first hits shaded from baked lightmaps.  Part 21 reads diffuse light from the probe volume only; here a static surface
 * reads its lightmap (Parts 13, 14, 17, 19 bake it) and everything else falls back to the volume.  The caller binds up to
 * PT_LIGHTMAP_MAX_BINDINGS lightmaps to spans of primitives; a hit inside a span reads four texels of the image instead of up to
 * eight probes.  An addition beside the reference's ABI, detected by symbol; PTGetVersion is unchanged; PTShadeInputs keeps its
 * 120 bytes, PTShadeBaked and PTShadeBakedFrame their bits.
 *
 * Left out: taps from a neighbouring chart of the same atlas (chart padding and PTResolveLightmap's dilate are the caller's
 * answer, as for every lightmapped renderer); directional (SH) lightmaps; several atlases blended; PTGroup wrappers; PTPresent of
 * the result.
 *
 * The rule (bit-exact; lightmap_lookup_rule.h is its one definition: the kernels, the host twin and tests/lightmap_lookup_ref.py
 * evaluate it; only + - * /, floorf and comparisons, every operator one IEEE binary32 operation in the order written, no fma).
 * Entry i reads its ray, its PTRayHit and its PTRaySurface, exactly what PTShadeSurfaces reads.
 *  1. No lightmap.  A miss as Part 21 step 2 defines it (prim == 0xFFFFFFFF, or a materialIndex not below the scene's material
 *     count) has none.  d is Part 21 step 2's d BEFORE the flip: Vd = (-D) / len, d = (N.x * Vd.x + N.y * Vd.y) + N.z * Vd.z with
 *     N = PTRaySurface.normal.  A hit with d < 0 is seen from behind: it matches only bindings with PT_LIGHTMAP_TWO_SIDED.
 *  2. Binding choice.  In ascending k, binding k matches when (uint32_t)(hit.prim - firstPrim) < primCount, and instance ==
 *     0xFFFFFFFF or instance == surface.instance, and the side rule holds.  The first match wins; none: PT_LIGHTMAP_NONE.
 *  3. UV.  p = hit.prim - firstPrim; corner k is (dUvs[6p + 2k], dUvs[6p + 2k + 1]), without dUvs uv0, uv1, uv2 of attribute
 *     record hit.prim.  b1 = hit.u, b2 = hit.v, w0 = 1.0f - b1 - b2; U = (u0 * w0 + u1 * b1) + u2 * b2, V likewise (Part 14's
 *     interpolation form).
 *  4. Footprint.  x = U * (float)width - 0.5f, y = V * (float)height - 0.5f.  Unless x > -1.0f && x < (float)width, and the same
 *     of y and height, nothing is found (a NaN lands here).  xf = floorf(x), x0 = (int32_t)xf, fx = x - xf; likewise y.  The taps
 *     are c00 = (x0, y0), c10 = (x0 + 1, y0), c01 = (x0, y0 + 1), c11 = (x0 + 1, y0 + 1).  A tap is valid when it lies inside the
 *     image and its texel's w > 0.0f (covered 1.0, dilated 0.5; a cleared texel, a negative or a NaN w is not).
 *  5. Filter, clamped to what is valid.  Row 0: both taps valid: r0 = c00 + fx * (c10 - c00) per channel; one: that tap; none: the
 *     row is invalid.  Row 1 likewise from c01, c11.  Both rows valid: E = r0 + fy * (r1 - r0); one: that row; none: nothing is
 *     found.  A constant image comes back exactly and no empty texel darkens a chart border; an invalid tap's rgb enters no
 *     arithmetic.
 *  6. Found: PTIrradiance {E.rgb, m2 = 0.0f} and the binding's index.  Otherwise zero bits and PT_LIGHTMAP_NONE.
 *  7. PTShadeLightmapped is PTShadeBaked with one change: where steps 1 to 6 find a lightmap, E is the lightmap's and the volume
 *     lookup is not executed for that entry; elsewhere E is Part 16's lookup (Part 18's with dPlacement).  It equals
 *     PTShadeSurfaces, PTProbeGridIrradiance[Placed], PTLightmapLookup, "the lightmap's irradiance where binding !=
 *     PT_LIGHTMAP_NONE, else the volume's", PTReflectionLookup and PTShadeCompose bit for bit; with nothing bound it equals
 *     PTShadeBaked.  PTShadeLightmappedFrame is PTShadeBakedFrame's three steps with that kernel (the same scratch): it equals
 *     PTTraceRays followed by PTShadeLightmapped over its rays.
 *
 * PTBindLightmaps validates on the host, copies the records into a table the context owns (the caller's array is not referenced
 * after the call returns) and is stream-ordered on the context's stream.  count == 0 unbinds; PTSetScene unbinds (the spans name
 * a scene); geometry, instance and material updates keep the table (primitive indices do not move).  The images and UV arrays
 * stay the caller's and must outlive their use.  With nothing bound PTLightmapLookup answers "not found" for every entry.
 * Errors: PT_ERR_NO_SCENE before PTSetScene; PT_ERR_INVALID_ARG for a NULL context, NULL bindings with count > 0, count >
 * PT_LIGHTMAP_MAX_BINDINGS, a NULL or misaligned dImage, a misaligned dUvs, a size outside 1 ... PT_CHART_MAX_SIZE, primCount
 * == 0 or a span past the scene's attribute count, an instance that is neither 0xFFFFFFFF nor below the scene's instance count
 * (a flat scene has none), an unknown flag bit, a nonzero reserved word; a refused call leaves the previous table bound.  The
 * other calls check their pointers as Part 21's do, and `inputs` exactly as PTShadeBaked checks it.  No CPU fallback.
 * PTLightmapLookupHost is the twin: no context, no GPU, the bindings' pointers are host pointers; attrs may be NULL when every
 * binding has dUvs; it returns 1, or 0 with PTGetBVHBuildError() set (the same refusals, spans against attrCount, instances
 * unchecked).
 * ===================================================================================================================== */
#define PT_LIGHTMAP_TWO_SIDED    1u          /* PTLightmapBinding.flags */
#define PT_LIGHTMAP_MAX_BINDINGS 64u
#define PT_LIGHTMAP_NONE         0xFFFFFFFFu

typedef struct PTLightmapBinding {  /* 48 bytes; a host struct, and the same bytes sit in the device table */
    uint32_t firstPrim, primCount;  /* a span of TriangleAttributes indices: a BLAS's triAttributeOffset and triangleCount, or 0 and
                                       the scene's whole count on a flat scene */
    uint32_t instance;              /* 0xFFFFFFFF: any instance (and the only legal value on a flat scene) */
    uint32_t flags;                 /* PT_LIGHTMAP_TWO_SIDED */
    uint32_t width, height;         /* 1 ... PT_CHART_MAX_SIZE */
    uint32_t reserved[2];           /* must be 0 */
    const void*  dImage;            /* width * height RGBA float32 as PTResolveLightmap writes it: w > 0 marks a filled texel; 16-byte aligned */
    const float* dUvs;              /* 6 floats per primitive of the span, PTRasterizeChart's layout, 8-byte aligned; NULL: uv0 .. uv2 of
                                       the attribute record */
} PTLightmapBinding;

#ifdef __cplusplus
static_assert(sizeof(PTLightmapBinding) == 48, "PTLightmapBinding is 48 bytes");
#else
_Static_assert(sizeof(PTLightmapBinding) == 48, "PTLightmapBinding is 48 bytes");
#endif

PT_API int PTBindLightmaps(PTContext* ctx, const PTLightmapBinding* bindings, uint32_t count);
/* dRays, dHits, dSurface: as PTShadeSurfaces takes them; dOut: count entries; dOutBinding: count words, or NULL. */
PT_API int PTLightmapLookup(PTContext* ctx, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface, uint64_t count, PTIrradiance* dOut,
                            uint32_t* dOutBinding);
PT_API int PTShadeLightmapped(PTContext* ctx, const PTShadeInputs* inputs, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface,
                              uint64_t count, float* dOut);
PT_API int PTShadeLightmappedFrame(PTContext* ctx, const PTFrameParams* params, const PTShadeInputs* inputs, float* dOut, PTRay* dOutRays);
/* host twin, no GPU */
PT_API int PTLightmapLookupHost(const PTLightmapBinding* bindings, uint32_t bindingCount, const PTTriangleAttributes* attrs, uint64_t attrCount,
                                uint32_t materialCount, const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces, uint64_t count,
                                PTIrradiance* out, uint32_t* outBinding);

/* =====================================================================================================================
 * Part 23: lightmap UVs.  Parts 14 to 22 rasterise, gather, filter, resolve, bind and shade from lightmap UVs that are the
 * caller's; this part makes them: PTUnwrapCharts cuts one BLAS of the CURRENT scene into charts by facing, PTPackChartsHost
 * places the few hundred chart rectangles in an atlas on the host, PTEmitChartUVs writes the (T, 6) float array that
 * PTRasterizeChart and PTLightmapBinding.dUvs take.  Per-triangle work runs in kernels; no vertex and no UV crosses the bus.  An
 * addition beside the reference's ABI, detected by symbol; PTGetVersion is unchanged.
 *
 * The rule (csrc/unwrap_rule.h has it in full; charts are decided on bits and integers, so any order of evaluation gives the
 * same bytes).
 *  - Corners.  Primitive p has corners c0, c1, c2: rows 3p .. 3p + 2 of dVertices -- 3 PTFloat4 per primitive in primIdx order,
 *    the array PTUpdateGeometryDevice takes; the library does not check that it is what the BLAS holds --, or with NULL v0,
 *    v0 + e1, v0 + e2 per component of the current triangle record of p.  Every component has + 0.0f applied, so -0 and +0 are
 *    one value.  The NULL form welds less (v0 + e1 need not be the float the neighbour stores): a few more charts, a valid atlas.
 *  - Class.  g = cross3(c1 - c0, c2 - c0).  p is excluded when a corner component is not finite or dot3(g, g) is 0 or not
 *    finite.  Otherwise a = the axis of largest |g| (a later axis wins only by >) and cls = 2 a + (g[a] < 0).
 *  - Charts.  Two included primitives of one class are linked when they share an edge: the same unordered pair of corner
 *    values, all 96 bits per corner equal; an edge of three or more primitives links all of one class.  A chart is a connected
 *    component; its label is its lowest primIdx; charts are listed in ascending label; chartOfPrim[p] is the chart's place in
 *    that list, PT_UNWRAP_NO_CHART for an excluded p.
 *  - Extents.  U = c[(a + 1) % 3], V = c[(a + 2) % 3]; umin, vmin, umax, vmax over the chart's corners (fp32 min / max, exact).
 *  - Size and packing (PTPackChartsHost).  w = (uint32)ceilf((umax - umin) * texelsPerUnit) + 1 + 2 * padding, h likewise; a
 *    product that is not finite or above 8192 does not fit.  Charts in the order h descending, w descending, label (firstPrim,
 *    then place in the list) ascending go on shelves: x = y = shelf = 0; w > width fails; x + w > width opens a shelf (y += shelf;
 *    x = 0; shelf = 0); the first chart of a shelf sets shelf = h; y + h > height fails; the origin is (x, y); x += w.
 *    *rowsUsed = y + shelf whenever every width fits -- also when the height does not, so that a caller can rescale; 0 otherwise.
 *  - UVs.  u_k = ((((U_k - umin) * texelsPerUnit) + (float)(ox + padding)) + 0.5f) / (float)width, v_k with V, vmin, oy,
 *    height; every operator one binary32 operation.  umin lands on a texel centre: an axis-aligned a x b rectangle covers
 *    exactly (floor(a tpu) + 1)(floor(b tpu) + 1) texels under PTRasterizeChart's inclusive edges.  Mirrored charts stay
 *    mirrored.  An excluded primitive, and one whose chartOfPrim is not below chartCount, gets six quiet NaNs (0x7FC00000):
 *    PTRasterizeChart leaves it out.
 *  - Not done: overlap detection inside a chart (a surface that winds over itself while keeping one facing projects onto
 *    itself; the lowest primitive owns the texel), mean-plane or conformal parameterisation (a face tilted 45 degrees gets 0.71 of
 *    the density, the worst case 0.58), merging, rotation, welding by tolerance, per-instance scale.
 *
 * PTUnwrapCharts.  The BLAS is named as in Part 14 (the three offsets, triangleCount); reserved must be 0.  dVertices 16-byte,
 * dChartOfPrim 4-byte, dCharts 16-byte aligned.  On the context's stream; *chartCount is read back, so THE CALL SYNCHRONISES
 * WITH THE CONTEXT STREAM (several times: once per sweep of the component search).  dChartOfPrim == NULL and dCharts == NULL:
 * only the count (and the stats).  count > capacity: PT_ERR_INVALID_ARG with *chartCount set and nothing written.  The steps:
 * corners and class; vertex identity by three stable radix sorts over the z, y and x words, run heads and a scan; edge keys (lo
 * id, hi id, class) in 64 bits, sorted, equal neighbours linked; components by hooking roots with atomicMin and full path
 * compression until a sweep changes nothing (at most 64 sweeps, PT_ERR_HIP past that); heads compacted; extents by integer
 * atomicMin / atomicMax on order-preserving keys.  stats (may be NULL): excluded primitives, linked edges (pairs of equal
 * neighbours in the sorted edge list), single-triangle charts, sweeps (the one that found no change included; the only figure
 * that depends on the order the hooks arrive in, so two calls may differ in it; the host twin reports 0).  Memory, in the
 * context, grown on demand, kept across PTSetScene, freed by PTDestroy: 148 bytes per triangle and the sort's temporary storage.
 * PTEmitChartUVs.  dChartOfPrim as PTUnwrapCharts wrote it; dCharts and dOrigins (x, y per chart; 8-byte aligned) are the
 * mesh's slice of whatever list was packed, chartCount its length: several meshes share an atlas by packing their concatenated
 * records once and emitting each mesh with its slice.  dUvs: 6 floats per primitive, 8-byte aligned.  Stream-ordered on the
 * context's stream, not synchronising.
 * Errors: Part 14's (no scene, NULL or misaligned pointers, only one of dChartOfPrim and dCharts, offsets that name no BLAS, a
 * triangleCount that is not the BLAS's, a nonzero reserved field), plus a size outside 1 ... 8192, padding above 16,
 * texelsPerUnit not finite or <= 0, a triangleCount T with 2 * bits(3 T) + 3 > 64 (bits(n): the width of n - 1).
 * The host twins (no context, no GPU; 1, or 0 with PTGetBVHBuildError() set): tris = the BLAS's 3 * triangleCount rows as
 * PTReadGeometry returns them (may be NULL with vertices), vertices = 3 * triangleCount rows or NULL; the desc's offsets are not
 * read.  PTPackChartsHost is a pure host function; origins: 2 * chartCount words.
 * ===================================================================================================================== */
#define PT_UNWRAP_NO_CHART    0xFFFFFFFFu
#define PT_UNWRAP_MAX_PADDING 16u
#define PT_UNWRAP_MAX_SWEEPS  64u

typedef struct PTUnwrapDesc {
    uint32_t structSize;          /* sizeof(PTUnwrapDesc) of the caller's header; members are only appended */
    int32_t  bvhOffset, triOffset, triAttributeOffset;
    int32_t  triangleCount;
    uint32_t reserved[7];         /* must be 0 */
} PTUnwrapDesc;

typedef struct PTUnwrapChart {    /* 32 bytes */
    uint32_t firstPrim;           /* the label: the chart's lowest primIdx */
    uint32_t cls;                 /* 2 * axis + (facing the negative direction) */
    uint32_t triCount;
    uint32_t reserved;            /* 0 */
    float    umin, vmin, umax, vmax;
} PTUnwrapChart;

typedef struct PTUnwrapStats {
    uint32_t excluded, linkedEdges, singleCharts, sweeps;
} PTUnwrapStats;

#ifdef __cplusplus
static_assert(sizeof(PTUnwrapDesc) == 48 && sizeof(PTUnwrapChart) == 32 && sizeof(PTUnwrapStats) == 16, "Part 23 struct sizes");
#else
_Static_assert(sizeof(PTUnwrapDesc) == 48 && sizeof(PTUnwrapChart) == 32 && sizeof(PTUnwrapStats) == 16, "Part 23 struct sizes");
#endif

/* Device arrays, on the context's stream; synchronises (the count). */
PT_API int PTUnwrapCharts(PTContext* ctx, const PTUnwrapDesc* desc, const PTFloat4* dVerticesOrNull, uint32_t* dChartOfPrim, PTUnwrapChart* dCharts,
                          uint32_t capacity, uint32_t* chartCount, PTUnwrapStats* statsOrNull);
/* Device arrays, stream-ordered on the context's stream. */
PT_API int PTEmitChartUVs(PTContext* ctx, const PTUnwrapDesc* desc, const PTFloat4* dVerticesOrNull, const uint32_t* dChartOfPrim,
                          const PTUnwrapChart* dCharts, const int32_t* dOrigins, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding,
                          float texelsPerUnit, float* dUvs);
/* host twins, no GPU */
PT_API int PTUnwrapChartsHost(const PTUnwrapDesc* desc, const PTFloat4* tris, const PTFloat4* verticesOrNull, uint32_t* chartOfPrim, PTUnwrapChart* charts,
                              uint32_t capacity, uint32_t* chartCount, PTUnwrapStats* statsOrNull);
PT_API int PTPackChartsHost(const PTUnwrapChart* charts, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float texelsPerUnit,
                            int32_t* origins, uint32_t* rowsUsed);
PT_API int PTEmitChartUVsHost(const PTUnwrapDesc* desc, const PTFloat4* tris, const PTFloat4* verticesOrNull, const uint32_t* chartOfPrim,
                              const PTUnwrapChart* charts, const int32_t* origins, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding,
                              float texelsPerUnit, float* uvs);

/* =====================================================================================================================
 * Part 24: direct light at first hits.  Parts 21 and 22 see the scene's analytic lights only through the bakes: a light moved
 * with PTUpdateLights, a skinned character's shadow, a point light's highlight on metal and a shadow edge sharper than a
 * lightmap texel are all missing from their frames.  This part is the other half of mixed lighting: sky, emissive surfaces and
 * bounced light stay in the bakes, the point, spot and rectangle lights are evaluated at every first hit with shadow rays, every
 * frame.  An addition beside the reference's ABI, detected by symbol; PTGetVersion is unchanged.
 *
 * Left out: sky for misses; the Disney lobes Part 21 leaves out; directional lights (they light nothing in the render either); a
 * bounded shadow ray; the indirect light of the analytic lights (bake with the lights muted, or accept it twice); PTGroup
 * wrappers; PTPresent of the result.
 *
 * The rule (bit-exact; csrc/direct_rule.h is its one definition: the kernels, the host twins and tests/direct_ref.py evaluate
 * it; every fp32 operator below is one IEEE binary32 operation in the order written, no fma; only + - * /, sqrt, saturate,
 * |x|, comparisons and pt_random_float).  dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; normalize(v) = v * (1.0f /
 * sqrt(dot(v, v))) per component -- the render's; max(x, y) below is "y > x ? y : x" read left to right as written.
 *  1. Inputs.  Entry i has its PTRay (direction D), the PTShadeTerms and the PTReceiver PTShadeSurfaces writes for it: position
 *     P, and N already turned towards the viewer.
 *  2. Miss.  An entry whose terms have nDotV > 0 false is a miss: all its pairs are skipped, its result is four zero words.
 *  3. Hit.  Vd is Part 21 step 2's: len = sqrt((D.x * D.x + D.y * D.y) + D.z * D.z); Vd = (-D) / len.  alpha = rho * rho (Part
 *     20's level roughness, the alpha the DFG table was integrated with); alpha = minAlpha > alpha ? minAlpha : alpha; a2 = alpha *
 *     alpha.  O = P + N * PT_EPSILON: per component b = N * PT_EPSILON, then P + b.
 *  4. Pairs.  The lights of the current scene in ascending index; a point light contributes 1 pair, a spot light 1, a rectangle
 *     light S * S with k = b * S + a (a = k % S, b = k / S); any other type none.  pairsPerEntry is the sum; pair (i, l, k) has
 *     index i * pairsPerEntry + offset_l + k.
 *  5. Light sample at scatterPos = O, with the light's derived rows n = normalize(cross(u, v)) (rectangle) or normalize(u)
 *     (spot) and nn = normalize(n), as PTSetScene and PTUpdateLights derive them.
 *     Point and spot: q = O - position; lsDistance = sqrt(dot(q, q)); L = -(q * (1.0f / lsDistance)) per component -- the
 *     render's -normalize(O - position); the render takes a spot light's distance from position - O, whose squares are the same
 *     bits.
 *     Rectangle: r1 = ((float)a + x1) / (float)S, r2 = ((float)b + x2) / (float)S; p = (position + u * r1) + v * r2; q = p - O;
 *     lsDistance = sqrt(dot(q, q)); L = q / lsDistance; lsNormal = n.  With PT_DIRECT_CENTERED x1 = x2 = 0.5f and nothing is
 *     drawn.  Otherwise the entry's state is s = seed; pt_rng_next(&s); s += (uint32_t)i; and x1, then x2, are drawn with
 *     pt_random_float(&s) for every pair of every rectangle light in ascending pair index, whether or not the pair ends up
 *     counting: no draw depends on visibility or on the material.
 *     falloff: lsDistance > range gives 0; otherwise r = lsDistance / range and falloff = saturate((1.0f / (1.0f + (25.0f * r)
 *     * r)) * saturate((1.0f - r) * 5.0f)).  Rectangle and spot: cosTheta = dot(normalize(-L), nn).  Rectangle: cosTheta < 0
 *     gives falloff 0.  Spot, with v.x and v.y the cosines of the outer and inner cone: cosTheta < v.x gives 0; v.x < cosTheta <
 *     v.y gives falloff = falloff * ((cosTheta - v.x) / (v.y - v.x)).  Li = emission * falloff.
 *  6. BRDF at L, isotropic GGX over Lambert, the model the bakes are composed with.  nl = dot(N, L); a pair with nl > 0 false is
 *     skipped.  H = Vd + L; len = sqrt(dot(H, H)); a len that is not > 0 leaves the specular term out (f = diffuse *
 *     0.31830988618379067f).  Otherwise H = H / len; nh = max(0, dot(N, H)); vh = max(0, dot(Vd, H)) (a NaN lands on 0);
 *     t = (nh * nh) * (a2 - 1.0f) + 1.0f; D = a2 / ((3.14159265f * t) * t); G = smith_g(nDotV, alpha) * smith_g(nl, alpha) with
 *     Part 21's smith_g; m = 1.0f - vh; Fc = ((m * m) * (m * m)) * m; F[c] = f0[c] + (1.0f - f0[c]) * Fc; sp = (D * G) / ((4.0f *
 *     nl) * nDotV); f[c] = diffuse[c] * 0.31830988618379067f + F[c] * sp.
 *  7. Weight and contribution.  w = 1.0f for a point or spot light; for a rectangle light w = ((area * |dot(lsNormal, L)|) /
 *     (lsDistance * lsDistance)) / (float)(S * S).  c[ch] = ((Li[ch] * f[ch]) * nl) * w.  A pair counts only if all three c are
 *     finite and at least one is > 0.  A pair that does not count has origin and direction 0, tmax = 0 (Part 3's miss without a
 *     walk) and zero contribution.  The shadow ray of a pair that counts is {O, L, tmax = PT_FAR_PLANE, 0}: the render's shadow
 *     ray, which has no far end (Part 15 says why and what follows), traced as PT_QUERY_ANY_HIT by Part 3's rules.
 *  8. Sum.  direct[ch] starts at +0.0f; in ascending pair index direct[ch] = direct[ch] + c[ch] for every pair that counts (at
 *     least one c > 0) and whose PTRayHit.prim == 0xFFFFFFFF.  The result is {direct.rgb, 1.0f}.
 *
 * PTDirectLight equals PTShadeSurfaces, PTDirectRays, PTTraceRays(PT_QUERY_ANY_HIT) and PTDirectAccumulate bit for bit, with the
 * walks inside the kernel and nothing per pair stored; it adds nothing to PTStats at any stats level.  PTShadeMixed equals
 * PTShadeLightmapped plus PTDirectLight, one add per channel (w is PTShadeLightmapped's).  PTShadeMixedFrame equals
 * PTShadeLightmappedFrame's rays and query followed by PTShadeMixed; entry i = y * W + x (the same scratch).  A scene without
 * HAS_LIGHTS has pairsPerEntry == 0: PTDirectLight writes {0, 0, 0, 1} for hits and PTShadeMixed equals PTShadeLightmapped.
 * The light arrays seen are the current generation's (Part 5's ordering).
 *
 * Device pointers are 16-byte aligned; the calls are stream-ordered on the context's stream and nothing past `count` is
 * written; count == 0 returns PT_OK and launches nothing.  count * pairsPerEntry is at most 2^31 per PTDirectRays /
 * PTDirectAccumulate call.  Errors are Part 21's and 22's (NULL or misaligned pointers, PT_ERR_NO_SCENE before PTSetScene, the
 * refusals of `inputs`), plus PT_ERR_INVALID_ARG for strata outside 1 ... PT_DIRECT_MAX_STRATA, an unknown flag, a nonzero
 * reserved word, a minAlpha that is not finite or is negative, a zero structSize (or one below this header's).
 * PTDirectAccumulate reads no scene: pairsPerEntry is the caller's, PTDirectPairCount's for the rays it accumulates.  No CPU
 * fallback.
 * The host twins take no context and no GPU; lights: lightCount PTLight records; they return 1, or 0 with
 * PTGetBVHBuildError() set.
 * ===================================================================================================================== */
#define PT_DIRECT_CENTERED   1u     /* PTDirectParams.flags: no jitter, every stratum sampled at its centre; no RNG draw */
#define PT_DIRECT_MAX_STRATA 4u     /* per axis: up to 16 shadow rays per rectangle light */

typedef struct PTDirectParams {
    uint32_t structSize;            /* sizeof(PTDirectParams) of the caller's header; members are only appended */
    uint32_t strata;                /* S: a rectangle light is sampled on an S x S grid, 1 ... PT_DIRECT_MAX_STRATA */
    uint32_t seed;
    uint32_t flags;
    float    minAlpha;              /* the specular lobe's alpha is max(alpha, minAlpha); 0 leaves it alone; finite, >= 0 */
    uint32_t reserved[3];           /* must be 0 */
} PTDirectParams;

#ifdef __cplusplus
static_assert(sizeof(PTDirectParams) == 32, "PTDirectParams is 32 bytes");
#else
_Static_assert(sizeof(PTDirectParams) == 32, "PTDirectParams is 32 bytes");
#endif

PT_API int PTDirectPairCount(PTContext* ctx, uint32_t strata, uint32_t* outPairsPerEntry);
/* steps 2-7: dOutRays and dOutContrib have count * pairsPerEntry entries (PTRay; float4 with w = 0) */
PT_API int PTDirectRays(PTContext* ctx, const PTDirectParams* params, const PTRay* dRays, const PTShadeTerms* dTerms, const PTReceiver* dRecv,
                        uint64_t count, PTRay* dOutRays, float* dOutContrib);
/* step 8 over what PTTraceRays(PT_QUERY_ANY_HIT) wrote for dOutRays; dOut: count float4 entries */
PT_API int PTDirectAccumulate(PTContext* ctx, const PTShadeTerms* dTerms, const float* dContrib, const PTRayHit* dPairHits, uint64_t count,
                              uint32_t pairsPerEntry, float* dOut);
/* the hot path: material fetch, terms, steps 2-8 with the walks inside the kernel; nothing per pair is stored */
PT_API int PTDirectLight(PTContext* ctx, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface,
                         uint64_t count, float* dOut);
/* PTShadeLightmapped's result with direct.rgb added per channel (one add each); w is PTShadeLightmapped's */
PT_API int PTShadeMixed(PTContext* ctx, const PTShadeInputs* inputs, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits,
                        const PTRaySurface* dSurface, uint64_t count, float* dOut);
PT_API int PTShadeMixedFrame(PTContext* ctx, const PTFrameParams* params, const PTShadeInputs* inputs, const PTDirectParams* direct, float* dOut,
                             PTRay* dOutRays);
/* host twins, no GPU */
PT_API int PTDirectPairCountHost(const void* lights, uint32_t lightCount, uint32_t strata, uint32_t* outPairsPerEntry);
PT_API int PTDirectRaysHost(const PTDirectParams* params, const void* lights, uint32_t lightCount, const PTRay* rays, const PTShadeTerms* terms,
                            const PTReceiver* receivers, uint64_t count, PTRay* outRays, float* outContrib);
PT_API int PTDirectAccumulateHost(const PTShadeTerms* terms, const float* contrib, const PTRayHit* pairHits, uint64_t count,
                                  uint32_t pairsPerEntry, float* out);

/* =====================================================================================================================
 * Part 25: direct light over many lights.  Part 24's fused calls walk every light of the scene for every entry; with a few
 * hundred local lights almost every pair falls to lsDistance > range.  This part adds a uniform grid over the lights and three
 * calls that offer each wave only the lights the grid lists for its lanes' cells.  Step 7 of Part 24 says that a pair which
 * does not count contributes nothing and gets no walk, so leaving it out changes no bit: PTDirectLightCulled,
 * PTShadeMixedCulled and PTShadeMixedFrameCulled give PTDirectLight's, PTShadeMixed's and PTShadeMixedFrame's bits.  An addition
 * detected by symbol; PTGetVersion, PTDirectParams, its flags and its refusals are unchanged.
 *
 * Left out: a spot's cone beyond its half-space; a hierarchical or screen-space structure; culling inside PTDirectRays /
 * PTDirectAccumulate; PTGroup wrappers.
 *
 * The rule (csrc/light_grid_rule.h is its one definition, written out operator by operator there; the kernels, the host twin
 * and tests/light_grid_ref.py evaluate it).  The grid is dims[0] x dims[1] x dims[2] cubes of cellSize from origin.
 *  1. The cell of a point X: per axis t = (X[a] - origin[a]) / cellSize; inside iff t >= 0 and t < (float)dims[a]; i[a] =
 *     (uint32_t)t; cell = (i.z * dims.y + i.y) * dims.x + i.x.  A point outside on any axis (a NaN is outside) gets cell index
 *     `cells`, the overflow cell, whose list is every light 0 ... L-1: such points are correct, merely not culled.
 *  2. A cell lists light l unless a test proves that no pair of l counts at any point step 1 maps to the cell: the type has no
 *     pairs (directional, unknown); every emission channel is 0; the squared distance from the light's centre C to the cell's
 *     box, inflated by `pad`, exceeds (R * (1 + 2^-10))^2 -- C = position and R = range, for a rectangle C = position + u / 2 + v
 *     / 2 and R = range + (|u| + |v|) / 2 --; or, for a rectangle and for a spot whose outer cosine v.x >= 0, the inflated box
 *     lies behind the plane through position with the light's derived normal by more than R * (1 + 2^-10) * 2^-16 (the margin
 *     covers the rounding of the cosine the pair rule decides by).  Every comparison culls only when it is
 *     TRUE, so a NaN or an infinity anywhere keeps the light listed.  pad = cellSize * 2^-10 + (|origin[a]| + cellSize *
 *     dims[a]) * 2^-20 per axis covers the rounding of step 1 and of the box corners (DESIGN.md 5.30 derives it).
 *     Nothing is assumed of the materials: a light with a negative emission channel stays listed.
 *  3. Storage: offsets, cells + 2 words -- the list of cell c is indices[offsets[c] ... offsets[c + 1]), the overflow cell's comes
 *     last and offsets[cells + 1] is the total --; indices, the lights of each list in ascending index; rectBefore, L + 1 words,
 *     the number of rectangle lights with a smaller index.
 *
 * PTBuildLightGrid builds the grid for the CURRENT generation of the light arrays on the context's stream, into memory the
 * context owns: one lane per cell, three launches (count, scan, emit), no atomics -- the same input gives the same bytes.  It
 * reads the 4-byte total back once between scan and emit (one stream synchronisation) to size the index buffer; a call that has to
 * grow one of the context's grid buffers (the first build, more cells, more lights) drains the stream once more before it frees
 * the smaller one; everything else is stream-ordered.  PTUpdateLights and PTSetScene make the grid stale: the culled calls refuse a stale or absent grid with
 * PT_ERR_INVALID_ARG ("no light grid" / "the light grid is stale") and never read a grid built for other lights.  A scene without
 * HAS_LIGHTS builds a grid whose lists are all empty.
 *
 * The culled calls.  After Part 24's steps 1-3 a lane takes the cell of its O (step 3's, the point the light sample uses); a
 * miss and a lane past `count` hold an empty list.  The wave visits the union of its lanes' lists in ascending light index and
 * every lane evaluates its pair with every visited light, exactly as PTDirectLight does: a lane whose cell does not list the
 * light gets a pair that does not count.  Without PT_DIRECT_CENTERED, when the loop goes from light a to light b every lane
 * advances its state by 2 * S * S * (rectBefore[b] - rectBefore[a + 1]) calls of pt_rng_next, the draws PTDirectLight makes for the
 * rectangle lights in between; the draws past the last visited light are dropped, nothing reads the state afterwards.
 *
 * Errors: Part 24's, plus PT_ERR_INVALID_ARG for a grid whose structSize is 0 (or below this header's), a dim outside 1 ... 256,
 * more than 2^20 cells, a cellSize that is not finite and > 0, a nonzero reserved word; PT_ERR_NO_SCENE before PTSetScene.
 * PTReadLightGrid and PTLightGridInfo synchronise the context's stream.  PTBuildLightGridHost takes no context and no GPU;
 * lights: lightCount PTLight records; it returns 1, or 0 with PTGetBVHBuildError() set.
 * ===================================================================================================================== */
#define PT_LIGHT_GRID_MAX_DIM   256u
#define PT_LIGHT_GRID_MAX_CELLS (1u << 20)

typedef struct PTLightGridParams {
    uint32_t structSize;            /* sizeof(PTLightGridParams) of the caller's header; members are only appended */
    float    origin[3];             /* the corner of cell (0, 0, 0) */
    float    cellSize;              /* finite, > 0 */
    uint32_t dims[3];               /* 1 ... PT_LIGHT_GRID_MAX_DIM each; their product at most PT_LIGHT_GRID_MAX_CELLS */
    uint32_t reserved;              /* must be 0 */
} PTLightGridParams;

typedef struct PTLightGridStats {
    uint32_t structSize;
    uint32_t built;                 /* 1: a grid exists (it may be stale) */
    uint32_t cells;                 /* without the overflow cell */
    uint32_t lightCount;            /* L of the lights it was built for */
    uint32_t longest;               /* the longest list among cells 0 ... cells - 1 */
    uint32_t stale;                 /* 1: the lights changed since the build */
    uint64_t entries;               /* offsets[cells + 1]: all lists, the overflow cell's included */
    uint64_t generation;            /* the light generation the grid was built for: PTSetScene and PTUpdateLights each start one */
} PTLightGridStats;

#ifdef __cplusplus
static_assert(sizeof(PTLightGridParams) == 36 && sizeof(PTLightGridStats) == 40, "PTLightGridParams is 36 bytes, PTLightGridStats 40");
#else
_Static_assert(sizeof(PTLightGridParams) == 36 && sizeof(PTLightGridStats) == 40, "PTLightGridParams is 36 bytes, PTLightGridStats 40");
#endif

PT_API int PTBuildLightGrid(PTContext* ctx, const PTLightGridParams* params);
/* host pointers: offsets cells + 2 words, rectBefore L + 1 words, indices indexCapacity words (NULL with 0: none are copied);
 * any of the three may be NULL.  PT_ERR_INVALID_ARG when indices is given and indexCapacity is below the total */
PT_API int PTReadLightGrid(PTContext* ctx, uint32_t* offsets, uint32_t* indices, uint64_t indexCapacity, uint32_t* rectBefore);
PT_API int PTLightGridInfo(PTContext* ctx, PTLightGridStats* out);
/* PTDirectLight, PTShadeMixed and PTShadeMixedFrame through the grid: the same arguments, the same bits */
PT_API int PTDirectLightCulled(PTContext* ctx, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits, const PTRaySurface* dSurface,
                               uint64_t count, float* dOut);
PT_API int PTShadeMixedCulled(PTContext* ctx, const PTShadeInputs* inputs, const PTDirectParams* params, const PTRay* dRays, const PTRayHit* dHits,
                              const PTRaySurface* dSurface, uint64_t count, float* dOut);
PT_API int PTShadeMixedFrameCulled(PTContext* ctx, const PTFrameParams* params, const PTShadeInputs* inputs, const PTDirectParams* direct, float* dOut,
                                   PTRay* dOutRays);
/* host twin, no GPU.  offsets: cells + 2 words; rectBefore: lightCount + 1 words; indices: indexCapacity words, written only when
 * the total fits (NULL with 0: count only); *outTotal (may be NULL): the total */
PT_API int PTBuildLightGridHost(const PTLightGridParams* params, const void* lights, uint32_t lightCount, uint32_t* offsets, uint32_t* indices,
                                uint64_t indexCapacity, uint32_t* rectBefore, uint64_t* outTotal);

/* Text of the last error on the calling thread ("" if none). */
PT_API const char* PTGetLastError(void);
/* Library/ABI version: (major << 16) | minor. */
PT_API int PTGetVersion(void);

#ifdef __cplusplus
}
#endif

#endif /* PTMI_PLUGIN_H */
