// pt_tlas.h — GPU TLAS build behind PTUpdateInstances (pt_tlas.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ptmi_layouts.h"

// Device workspace of one instance count n, carved by the host from one allocation (pt_tlas_work_bytes).
struct PTTlasWork {
    uint32_t n;
    float4* box;        // 2n: aabbMin, aabbMax of instance i at 2i, 2i + 1
    uint32_t* idx;      // n: the primitive index list, partitioned in place as Tlas::build partitions it
    uint32_t* tmpIdx;   // n: cooperative partition output
    uint32_t* tmpR;     // n: right flag (bit 31) + count of right elements before (cooperative partition)
    uint32_t* rf;       // n: position of the k-th front right element
    uint32_t* lb;       // n: position of the k-th back left element (from the top)
    float4* nb0;        // 2n, indexed by breadth-first node id: mn.xyz, first index slot (bits)
    float4* nb1;        // 2n: mx.xyz, instance count (bits)
    uint32_t* nlt;      // 2n: left edges on the path from the root (tinybvh's taskCount at the node)
    uint32_t* nchild;   // 2n: breadth-first id of the left child (right = +1), 0xFFFFFFFF for a leaf
    uint32_t* nsplit;   // 2n: 1 when the node split
    uint32_t* nleft;    // 2n: left child's instance count
    float4* sp;         // 4 x 2n: left min, left max, right min, right max of a split
    uint32_t* nsize;    // 2n: subtree node count
    uint32_t* npre;     // 2n: depth-first (preorder) position = index in the BuildTLAS layout
    uint32_t* levels;   // 2n + 1: first breadth-first id of every level, then the node count
    uint32_t* big;      // n: the nodes of a level built by the whole workgroup
    uint32_t* ctrl;     // 4: [0] = node count
    PTBlasInstance* input;  // n: the update's instance records (host variant: staged copy)
};

size_t pt_tlas_work_bytes(uint32_t n);
PTTlasWork pt_tlas_carve(void* base, uint32_t n);

// Builds the TLAS of `in` (n records, device memory) and writes, all in stream order:
//   rawTlas: (2n - 1) PTTlasNode in BuildTLAS's depth-first layout, unreachable nodes zero, then the n instance indices
//   bfs: the same nodes renumbered breadth-first ((2n - 1) x 64 bytes, padding zero)
//   instByLeaf: n x 96 bytes (worldToLocal, offsets row, instance index of every index slot)
//   instances: the localToWorld / worldToLocal of every PTGpuInstance record (offsets rows are kept)
hipError_t pt_launch_tlas_update(const PTTlasWork& W, const PTBlasInstance* in, float* rawTlas, float* bfs, float* instByLeaf,
                                 float* instances, hipStream_t stream);
