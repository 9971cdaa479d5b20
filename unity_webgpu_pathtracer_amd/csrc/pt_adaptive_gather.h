// pt_adaptive_gather.h — launchers of the adaptive gather's kernels (pt_adaptive_gather.hip; include/ptmi_plugin.h Part 19).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ptmi_plugin.h"

// One select: step 2 over active[0 .. activeCount) (NULL: every entry), then the stable compaction of the survivors.
struct PTAgSelectArgs {
    const uint32_t* active;         // NULL: entry k is index k
    const float4* acc;              // entryCount accumulated entries, read through the index
    const float4* recv;             // entryCount receivers, two float4 each, read through the index
    uint32_t activeCount, entryCount;
    uint32_t n, addSamples, maxSamples;
    float threshold2, darkFloor;    // threshold2 = threshold * threshold
    uint32_t* blockCounts;          // 4 x blocks words: the survivors of every 256-entry block (then their exclusive prefix), and the
                                    // block's entries stopped by threshold, by maxSamples, as non-finite
    uint64_t* totals;               // 4 words: survivors, stopped by threshold, by maxSamples, as non-finite
    uint32_t* outActive;            // activeCount entries; only the survivors are written
    float4* outRecv;                // likewise, two float4 each
};

size_t pt_ag_blocks(uint64_t activeCount);                                  // 256-entry blocks
// count, scan and emit; activeCount > 0, the arguments checked by the caller
hipError_t pt_launch_ag_select(const PTAgSelectArgs& A, hipStream_t stream);
// step 3: fresh[k] (m samples) into acc[active[k]] (n samples; 0 writes); counts (may be NULL) gets n + m
hipError_t pt_launch_ag_fold(const uint32_t* active, uint32_t activeCount, uint32_t entryCount, const PTIrradiance* fresh, uint32_t m, uint32_t n,
                             PTIrradiance* acc, uint32_t* counts, hipStream_t stream);
// step 5; out may equal irr
hipError_t pt_launch_ag_equalise(const PTIrradiance* irr, const uint32_t* counts, uint32_t count, uint32_t samplesEq, PTIrradiance* out, hipStream_t stream);
