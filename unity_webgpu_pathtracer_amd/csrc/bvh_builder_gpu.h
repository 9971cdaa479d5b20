// bvh_builder_gpu.h — the device CWBVH builder's pipeline (bvh_builder_gpu.hip) for callers that own the stream and the memory:
// PTBuildBVHDevice's handle-table wrapper (build_cwbvh_device) and the in-place rebuild (pt_api_geometry.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace ptbvh {

// bytes of the work arrays for n triangles, rocprim's temporary storage included (0: n out of range or a failed size query)
size_t device_build_work_bytes(uint32_t n);

enum DeviceBuildStatus { kBuildOk = 0, kBuildNonFinite, kBuildOverCapacity, kBuildFailed };

struct DeviceBuildResult {
    uint32_t nodeCount = 0;                 // K: wide nodes of the tree, whether or not they fit
    std::vector<uint32_t> levelStart;       // levels + 1 boundaries: level d is nodes levelStart[d] ... levelStart[d + 1] - 1
    uint32_t badVertex = 0;                 // kBuildNonFinite: the first vertex that is not finite
};

// The pipeline on `stream`: bounds, keys, sort, hierarchy, fit, one level launch per tree level.  dVerts: 3 * n vertices on the
// device; nodes / tris: where node 0 and row 0 of the tree go (indices inside the tree are relative to them); nodeCapacity: nodes
// that may be written at `nodes` -- a tree of more nodes is counted to its end (kBuildOverCapacity, nodeCount = K) but no node past
// the capacity is written; all 3 * n rows at `tris` are written.  work: device_build_work_bytes(n) bytes, 256-aligned.
// checkFinite: read the bounds kernel's flag back before anything else is launched (kBuildNonFinite; only the bounds pass has
// run).  Synchronises with `stream` once per tree level (one counter) and for the flags.  kBuildFailed: err has the message.
// kernelsDone (may be null): recorded behind the last level launch, before the final read-back of the counters.
DeviceBuildStatus device_build_cwbvh(hipStream_t stream, const float4* dVerts, uint32_t n, uint4* nodes, float4* tris, uint32_t nodeCapacity,
                                     void* work, bool checkFinite, DeviceBuildResult& out, std::string& err, hipEvent_t kernelsDone = nullptr);

} // namespace ptbvh
