// pt_direct.h — launchers of the direct-light kernels (pt_direct.hip; include/ptmi_plugin.h Part 24).
#pragma once
#include "pt_device.h"

struct PTLightGridDevice;           // pt_light_grid.h

// pt_launch.h's pt_resident_wave_caps of pt_direct_light (caps[0]) and pt_direct_light_tlas (caps[1]); a slab row is the ray
// queries' (pt_resident_wave_slab_bytes)
hipError_t pt_direct_grid_caps(int device, uint32_t caps[2]);
hipError_t pt_direct_culled_grid_caps(int device, uint32_t caps[2]);      // likewise pt_direct_light_grid and pt_direct_light_grid_tlas (Part 25)
// first: the list index of entry 0 of this launch (the entry's RNG state is made from the list index)
hipError_t pt_launch_direct_rays(const DScene& S, const PTDirectParams& P, uint32_t pairsPerEntry, const PTRay* rays, const PTShadeTerms* terms,
                                 const PTReceiver* receivers, uint32_t count, uint32_t first, PTRay* outRays, float4* outContrib, hipStream_t stream);
hipError_t pt_launch_direct_accumulate(const PTShadeTerms* terms, const float4* contrib, const PTRayHit* pairHits, uint32_t count, uint32_t pairsPerEntry,
                                       float4* out, hipStream_t stream);
// add: out[i].rgb = out[i].rgb + direct.rgb for a hit and nothing else is written (PTShadeMixed's second launch); otherwise out[i]
// = {direct.rgb, 1} for a hit and zeros for a miss.  slab holds >= gridCap waves.  lightGrid: a grid built for the scene's current
// lights launches the culled kernels (the same bits), null the ones that walk every light
hipError_t pt_launch_direct_light(const DScene& S, const PTDirectParams& P, const PTRay* rays, const PTRayHit* hits, const PTRaySurface* surfaces,
                                  uint32_t count, uint32_t first, float4* out, bool add, uint2* slab, uint32_t gridCap, hipStream_t stream,
                                  const PTLightGridDevice* lightGrid = nullptr);
