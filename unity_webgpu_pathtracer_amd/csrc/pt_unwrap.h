// pt_unwrap.h — launchers of the unwrap kernels (pt_unwrap.hip; include/ptmi_plugin.h Part 23).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ptmi_plugin.h"

// Bytes of the context's work array per triangle (the sort's temporary storage and 4 bytes per 256 corners come on top):
//   48  corners        3 float4: the corner values, + 0.0f applied
//    4  cls            the class, or 0xFF
//   48  sort           two key and two value arrays of 3 words each for the vertex sort; afterwards the edge keys (both key
//                      arrays together) and the two edge value arrays
//   12  vertex ids     one per corner
//   24  sorted keys    the edge keys after their sort
//   12  label, triangles per label, a head's place in the chart list
constexpr size_t kUnwrapBytesPerTriangle = 148u;

struct PTUnwrapArgs {
    const float4* tris;         // the BLAS's first triangle row (e2, e1, v0 + primIdx per record)
    const float4* vertices;     // the caller's 3 rows per primitive, or null: the records
    uint32_t triCount;
    // the work array, carved by pt_unwrap_carve
    float4*   corners;
    uint32_t* cls;
    uint32_t *keyA, *keyB, *valA, *valB;     // 3 T words each; keyA and keyB are adjacent
    uint32_t* vid;
    uint64_t *edgeKey, *edgeKeySorted;      // edgeKey = keyA
    uint32_t *label, *triOfLabel, *place;
    uint32_t* blockBase;        // one word per 256 corners
    uint32_t* small;            // kUnwrapSmallWords words: see pt_unwrap.hip
    void*     sortTemp;
    size_t    sortTempBytes;
};
constexpr uint32_t kUnwrapSmallWords = 8u + PT_UNWRAP_MAX_SWEEPS;
// words of `small`: 0 excluded, 1 linked edges, 2 single-triangle charts, 3 vertices, 4 charts, 8 + s: sweep s changed a label

size_t pt_unwrap_work_bytes(uint32_t triCount);                              // 0: the sort's size query failed
void pt_unwrap_carve(void* base, uint32_t triCount, PTUnwrapArgs& A);
// corners, classes, vertex ids, sorted edge keys; labels are their own
hipError_t pt_launch_unwrap_edges(const PTUnwrapArgs& A, hipStream_t stream);
// sweep s of the component search: hook, then compress; A.small[8 + s] != 0 afterwards when a label changed
hipError_t pt_launch_unwrap_sweep(const PTUnwrapArgs& A, uint32_t s, hipStream_t stream);
// triangles per label, heads counted and scanned: A.small[4] = the charts, A.small[2] = the single-triangle ones
hipError_t pt_launch_unwrap_count(const PTUnwrapArgs& A, hipStream_t stream);
// the chart records and chartOfPrim; the caller has checked the capacity against A.small[4]
hipError_t pt_launch_unwrap_charts(const PTUnwrapArgs& A, uint32_t* chartOfPrim, PTUnwrapChart* charts, uint32_t chartCount, hipStream_t stream);
hipError_t pt_launch_unwrap_emit(const float4* tris, const float4* vertices, uint32_t triCount, const uint32_t* chartOfPrim, const PTUnwrapChart* charts,
                                 const int32_t* origins, uint32_t chartCount, uint32_t width, uint32_t height, uint32_t padding, float tpu, float* uvs,
                                 hipStream_t stream);
