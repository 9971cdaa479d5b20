// pt_lightmap.h — launchers of the lightmap kernels (pt_lightmap.hip; include/ptmi_plugin.h Part 14).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ptmi_plugin.h"

// One chart: a BLAS of the current scene, an atlas size and the context's work arrays.
struct PTChartArgs {
    const float4* tris;         // the BLAS's first triangle row (e2, e1, v0 + primIdx per record)
    const float4* attrs;        // the BLAS's first attribute record (8 rows each), indexed by primIdx
    const float*  uvs;          // the caller's 6 floats per primitive, or null: the records' uv0 .. uv2
    const float4* instance;     // the PTGpuInstance record (9 rows) whose transform places the receivers, or null: identity
    uint32_t triCount, width, height, seedBase;
    uint32_t* owner;            // width * height words: the lowest primIdx that covers the texel, or 0xFFFFFFFF
    uint32_t* recOfPrim;        // triCount words: the record that carries primitive p
    uint32_t* large;            // 1 + triCount words: a counter, then the records whose box is left to pt_lm_coverage_large
    uint32_t* blockBase;        // one word per 256-texel block: its covered texels, then (after the scan) those of the blocks before it
    uint64_t* total;            // the covered texels of the chart
};

size_t pt_lm_blocks(uint32_t width, uint32_t height);                       // 256-texel blocks of an atlas
// owner map (cleared first), per-block counts, scan: everything but the emit.  *A.total is valid when the stream has run this.
hipError_t pt_launch_lm_coverage(const PTChartArgs& A, hipStream_t stream);
// texels[i], recv[i] for the covered texels in ascending texel index; the caller has checked the capacity against *A.total
hipError_t pt_launch_lm_emit(const PTChartArgs& A, uint32_t* texels, PTReceiver* recv, hipStream_t stream);
// image (width * height float4) = scatter of irr by texels, then `dilate` passes through `other`; the result ends in image
hipError_t pt_launch_lm_resolve(const uint32_t* texels, const PTIrradiance* irr, uint64_t count, uint32_t width, uint32_t height, uint32_t dilate,
                                float4* image, float4* other, hipStream_t stream);
