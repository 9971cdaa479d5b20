// pt_quality.h — the tree-quality measure on the device behind PTMeasureGeometry (pt_quality.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// bytes of `work` for a BLAS of nodeCount nodes: the two results, then one partial sum per workgroup of 256 nodes
size_t pt_quality_work_bytes(uint32_t nodeCount);
// pt_geometry_quality over order[0 ... nodeCount) (absolute node indices, the root first), then the fold, on `stream`.
// Afterwards work[0] = the sum of halfArea * weight over every occupied slot, work[1] = the root's half area.
hipError_t pt_launch_geometry_quality(const uint4* nodes, const uint32_t* order, uint32_t nodeCount, double* work, hipStream_t stream);
