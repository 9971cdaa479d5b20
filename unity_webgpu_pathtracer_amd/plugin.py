"""ctypes binding of libunity-webgpu-pathtracer-plugin.so — the reference-side view of the drop-in.

`TinyBVH` mirrors Assets/Scripts/util/TinyBVH.cs:15-50 name for name (the [DllImport] block of the C# host),
so parity tests read like calls made by BVHScene.cs.  The PT* render functions are bound on the same
library handle (include/ptmi_plugin.h, Part 2).

The library is the product: if it is missing it is built with hipcc (csrc/Makefile); if that fails the
import fails loudly.  There is no Python or CPU fallback for any of these entry points.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libunity-webgpu-pathtracer-plugin.so"      # Plugin/CMakeLists.txt:3 / TinyBVH.cs:8-12
LIB_PATH = os.environ.get("PT_PLUGIN") or os.path.join(_HERE, "lib", LIB_NAME)   # PT_PLUGIN: explicit build to load

# every export of include/ptmi_plugin.h: name -> (restype, argtypes)
vp, i32, u32p = C.c_void_p, C.c_int, C.POINTER(C.c_uint32)
sig = {
    # Part 1 (TinyBVH.cs)
    "BuildBVH": (i32, [vp, i32]), "DestroyBVH": (None, [i32]), "IsBVHReady": (i32, [i32]),
    "GetBVHPtr": (vp, [i32]), "GetBVH": (vp, [i32]),
    "GetCWBVHNodesSize": (i32, [i32]), "GetCWBVHTrisSize": (i32, [i32]),
    "GetCWBVHData": (i32, [i32, C.POINTER(vp), C.POINTER(vp)]),
    "PTBuildBVHDevice": (i32, [i32, vp, i32]), "PTGetBVHBuildError": (C.c_char_p, []), "PTGetBVHBuildMs": (C.c_double, [i32]),
    "PTRefitBVH": (i32, [i32, vp, i32]), "PTRefitBVHArrays": (i32, [vp, C.c_uint64, vp, C.c_uint64, vp, i32]),
    "BuildTLAS": (i32, [vp, i32]), "DestroyTLAS": (None, [i32]), "IsTLASReady": (i32, [i32]),
    "GetTLASNodesSize": (i32, [i32]), "GetTLASData": (i32, [i32, C.POINTER(vp), C.POINTER(vp)]),
    # Part 2 (render)
    "PTCreate": (i32, [i32, C.POINTER(vp)]), "PTDestroy": (i32, [vp]),
    "PTSetScene": (i32, [vp, C.POINTER(abi.PTSceneDesc)]),
    "PTSetTileOwnership": (i32, [vp, i32, i32]),
    "PTRenderPass": (i32, [vp, C.POINTER(abi.PTFrameParams)]),
    "PTFlipFrames": (i32, [vp]), "PTResetFrames": (i32, [vp]),
    "PTRenderPassTo": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, vp]),
    "PTRenderPassBatchTo": (i32, [vp, C.POINTER(abi.PTFrameParams), i32, vp, vp]),
    "PTRenderPassBatch": (i32, [vp, C.POINTER(abi.PTFrameParams), i32]),
    "PTGroupRenderPassBatch": (i32, [vp, C.POINTER(abi.PTFrameParams), i32]),
    "PTSynchronize": (i32, [vp]), "PTReadback": (i32, [vp, vp, C.c_uint64]),
    "PTGetFramePointer": (vp, [vp, i32]), "PTGetStream": (vp, [vp]),
    "PTSetStatsLevel": (i32, [vp, i32]), "PTGetStats": (i32, [vp, C.POINTER(abi.PTStats)]), "PTResetStats": (i32, [vp]),
    "PTGetRepackStats": (i32, [vp, C.POINTER(abi.PTRepackStats)]),
    "PTRepackPlanHost": (i32, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]),
    "PTSetProfiling": (i32, [vp, i32]), "PTGetTimings": (i32, [vp, C.POINTER(abi.PTTimings)]), "PTResetTimings": (i32, [vp]),
    "PTProcessMeshes": (i32, [vp, C.POINTER(abi.PTMeshDesc), C.c_uint32, C.c_uint32, vp, vp]),
    "PTCopyTextureData": (i32, [vp, C.POINTER(abi.PTTextureDesc), C.c_uint32, vp, C.c_uint64]),
    "PTPresent": (i32, [vp, C.POINTER(abi.PTPresentParams), vp, vp]),
    "PTPresentToHost": (i32, [vp, C.POINTER(abi.PTPresentParams), vp, C.c_uint64]),
    "PTSetSchedule": (i32, [vp, i32]), "PTGetSchedule": (i32, [vp]), "PTSetWavefrontIterations": (i32, [vp, i32]),
    "PTSetPassesInFlight": (i32, [vp, i32]), "PTGetPassesInFlight": (i32, [vp]), "PTSetSubFrames": (i32, [vp, i32]),
    "PTGetOwnedTileSlots": (i32, [vp, C.POINTER(abi.PTFrameParams), C.POINTER(C.c_uint64)]),
    "PTPackOwnedTiles": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, vp]),
    "PTUnpackTiles": (i32, [vp, C.POINTER(abi.PTFrameParams), i32, i32, vp, vp]),
    "PTCreateMulti": (i32, [C.POINTER(i32), i32, C.POINTER(vp)]), "PTGroupDestroy": (i32, [vp]), "PTGroupSize": (i32, [vp]),
    "PTGroupGetContext": (vp, [vp, i32]), "PTGroupSetScene": (i32, [vp, C.POINTER(abi.PTSceneDesc)]),
    "PTGroupRenderPass": (i32, [vp, C.POINTER(abi.PTFrameParams)]), "PTGroupFlipFrames": (i32, [vp]), "PTGroupResetFrames": (i32, [vp]),
    "PTGroupSynchronize": (i32, [vp]), "PTGroupReadback": (i32, [vp, vp, C.c_uint64]), "PTGroupGetAssembledFrame": (vp, [vp]),
    "PTGroupGetStats": (i32, [vp, C.POINTER(abi.PTStats)]), "PTGroupResetStats": (i32, [vp]),
    # Part 3 (ray queries)
    "PTTraceRays": (i32, [vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "PTTraceRaysHost": (i32, [vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    # Part 4 (guides and denoising)
    "PTRenderGuides": (i32, [vp, C.POINTER(abi.PTFrameParams), i32]),
    "PTDenoise": (i32, [vp, C.POINTER(abi.PTDenoiseParams), vp, vp]),
    "PTDenoiseToHost": (i32, [vp, C.POINTER(abi.PTDenoiseParams), vp, C.c_uint64]),
    "PTGetGuidePointer": (vp, [vp, i32]),
    # Part 5 (scene updates)
    "PTUpdateInstances": (i32, [vp, vp, C.c_uint32]), "PTUpdateInstancesDevice": (i32, [vp, vp, C.c_uint32]),
    "PTUpdateLights": (i32, [vp, vp, C.c_uint32]), "PTUpdateMaterials": (i32, [vp, vp, C.c_uint32]),
    "PTReadTLAS": (i32, [vp, vp, C.c_uint64, vp, C.c_uint64, u32p]),
    # Part 6 (variance across passes)
    "PTAccumulateMoments": (i32, [vp, C.POINTER(abi.PTFrameParams), i32]),
    "PTAccumulateMomentsTo": (i32, [vp, C.POINTER(abi.PTFrameParams), i32, vp, vp]),
    "PTGetMomentsInfo": (i32, [vp, u32p, C.POINTER(C.c_uint64), u32p, u32p]),
    "PTGetMomentsPointer": (vp, [vp, i32]),
    "PTMeasureNoise": (i32, [vp, C.POINTER(abi.PTNoiseParams), vp, C.POINTER(abi.PTNoiseStats)]),
    "PTGetNoiseTilePointer": (vp, [vp]),
    "PTDenoiseMoments": (i32, [vp, C.POINTER(abi.PTDenoiseParams), vp, vp]),
    "PTDenoiseMomentsToHost": (i32, [vp, C.POINTER(abi.PTDenoiseParams), vp, C.c_uint64]),
    # Part 7 (adaptive sampling)
    "PTAdaptiveBegin": (i32, [vp, C.POINTER(abi.PTFrameParams), C.c_uint32]), "PTAdaptiveEnd": (i32, [vp]),
    "PTSetActiveBlocks": (i32, [vp, u32p, C.c_uint32, u32p]),
    "PTSelectActiveBlocks": (i32, [vp, C.POINTER(abi.PTAdaptiveSelect), u32p]),
    "PTGetActiveBlocks": (i32, [vp, u32p, C.c_uint32, u32p]), "PTGetBlockSamples": (i32, [vp, u32p, C.c_uint64]),
    "PTRenderPassActive": (i32, [vp, C.POINTER(abi.PTFrameParams), i32]),
    "PTRenderPassActiveTo": (i32, [vp, C.POINTER(abi.PTFrameParams), i32, vp, vp]),
    "PTAccumulateMomentsActive": (i32, [vp, C.POINTER(abi.PTFrameParams), i32]),
    "PTAccumulateMomentsActiveTo": (i32, [vp, C.POINTER(abi.PTFrameParams), i32, vp, vp]),
    # Part 8 (radiance queries)
    "PTCameraRays": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, vp]),
    "PTTraceRadiance": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, vp]),
    "PTTraceRadianceHost": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, vp]),
    # Part 9 (geometry updates)
    "PTUpdateGeometry": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, i32, vp]),
    "PTUpdateGeometryDevice": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, i32, vp]),
    "PTReadGeometry": (i32, [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64]),
    # Part 10 (geometry rebuilds and tree quality)
    "PTRebuildGeometry": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, i32, vp]),
    "PTRebuildGeometryDevice": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, i32, vp]),
    "PTMeasureGeometry": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(abi.PTGeometryQuality)]),
    "PTMeasureBVHArrays": (i32, [vp, C.c_uint64, vp, C.c_uint64, i32, C.POINTER(abi.PTGeometryQuality)]),
    # Part 11 (skinned geometry)
    "PTSetSkin": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, i32, C.POINTER(abi.PTSkinDesc)]),
    "PTSkinGeometry": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "PTSkinGeometryDevice": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "PTSkinVerticesHost": (i32, [C.POINTER(abi.PTSkinDesc), i32, vp, vp, vp, C.POINTER(C.c_float)]),
    # Part 12 (morph targets)
    "PTSetMorph": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, i32, C.POINTER(abi.PTMorphDesc)]),
    "PTMorphGeometry": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "PTMorphGeometryDevice": (i32, [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "PTMorphVerticesHost": (i32, [C.POINTER(abi.PTMorphDesc), C.POINTER(abi.PTSkinDesc), i32, vp, vp, vp, vp, C.POINTER(C.c_float)]),
    "PTMorphLayoutHost": (C.c_uint64, [vp, vp, C.c_uint32, vp, vp, vp]),
    # Part 13 (irradiance gathers)
    "PTGatherIrradiance": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    "PTGatherIrradianceHost": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    "PTGatherRays": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    # Part 14 (lightmap charts)
    "PTRasterizeChart": (i32, [vp, C.POINTER(abi.PTChartDesc), vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "PTRasterizeChartHost": (i32, [C.POINTER(abi.PTChartDesc), vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "PTResolveLightmap": (i32, [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "PTResolveLightmapHost": (i32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    # Part 15 (SH light probes)
    "PTProbeSH": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "PTProbeSHHost": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "PTProbeRays": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    "PTProbeIrradiance": (i32, [vp, vp, C.c_uint64, vp, C.c_uint64, vp]),
    "PTProbeDirectionsHost": (i32, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    "PTProbeProjectHost": (i32, [vp, vp, C.c_uint64, C.c_uint32, vp]),
    "PTProbeIrradianceHost": (i32, [vp, C.c_uint64, vp, C.c_uint64, vp]),
    # Part 16 (probe volumes)
    "PTProbeDepth": (i32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float, vp]),
    "PTProbeDepthHost": (i32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float, vp]),
    "PTProbeGridIrradiance": (i32, [vp, C.POINTER(abi.PTProbeGrid), vp, vp, vp, C.c_uint64, vp]),
    "PTProbeDepthProjectHost": (i32, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_float, vp]),
    "PTProbeGridIrradianceHost": (i32, [C.POINTER(abi.PTProbeGrid), vp, vp, vp, C.c_uint64, vp]),
    # Part 17 (the lightmap denoiser)
    "PTDenoiseLightmap": (i32, [vp, C.POINTER(abi.PTLightmapDenoiseParams), vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    "PTDenoiseLightmapHost": (i32, [C.POINTER(abi.PTLightmapDenoiseParams), vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    # Part 18 (probe placement)
    "PTProbePlace": (i32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(abi.PTProbePlaceParams), C.c_uint32, vp, vp]),
    "PTProbePlaceHost": (i32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(abi.PTProbePlaceParams), C.c_uint32, vp, vp]),
    "PTProbeGridIrradiancePlaced": (i32, [vp, C.POINTER(abi.PTProbeGrid), vp, vp, vp, vp, C.c_uint64, vp]),
    "PTProbePlaceStepHost": (i32, [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(abi.PTProbePlaceParams), vp, vp, i32, vp, vp]),
    "PTProbeGridIrradiancePlacedHost": (i32, [C.POINTER(abi.PTProbeGrid), vp, vp, vp, vp, C.c_uint64, vp]),
    # Part 19 (adaptive gathers)
    "PTGatherIrradianceAdaptive": (i32, [vp, C.POINTER(abi.PTFrameParams), C.POINTER(abi.PTAdaptiveGather), vp, C.c_uint64, vp, vp,
                                         C.POINTER(abi.PTAdaptiveGatherStats)]),
    "PTGatherIrradianceAdaptiveHost": (i32, [vp, C.POINTER(abi.PTFrameParams), C.POINTER(abi.PTAdaptiveGather), vp, C.c_uint64, vp, vp,
                                             C.POINTER(abi.PTAdaptiveGatherStats)]),
    "PTSelectReceivers": (i32, [vp, C.POINTER(abi.PTAdaptiveGather), C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64),
                                C.POINTER(C.c_uint64)]),
    "PTFoldIrradiance": (i32, [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp]),
    "PTEqualiseIrradiance": (i32, [vp, vp, vp, C.c_uint64, C.c_uint32, vp]),
    "PTSelectReceiversHost": (i32, [C.POINTER(abi.PTAdaptiveGather), C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64)]),
    "PTFoldIrradianceHost": (i32, [vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp]),
    "PTEqualiseIrradianceHost": (i32, [vp, vp, C.c_uint64, C.c_uint32, vp]),
    # Part 20 (reflection probes)
    "PTReflectionRays": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "PTReflectionCapture": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "PTReflectionCaptureHost": (i32, [vp, C.POINTER(abi.PTFrameParams), vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "PTReflectionPrefilter": (i32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    "PTReflectionLookup": (i32, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64, vp]),
    "PTReflectionDirectionsHost": (i32, [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "PTReflectionFoldHost": (i32, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    "PTReflectionPrefilterHost": (i32, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    "PTReflectionLookupHost": (i32, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64, vp]),
    # Part 21 (shading from the bakes)
    "PTBakeDFG": (i32, [vp, C.c_uint32, vp]),
    "PTShadeSurfaces": (i32, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, vp]),
    "PTShadeCompose": (i32, [vp, vp, vp, vp, C.c_uint64, vp, C.c_uint32, vp]),
    "PTShadeBaked": (i32, [vp, C.POINTER(abi.PTShadeInputs), vp, vp, vp, C.c_uint64, vp]),
    "PTShadeBakedFrame": (i32, [vp, C.POINTER(abi.PTFrameParams), C.POINTER(abi.PTShadeInputs), vp, vp]),
    "PTBakeDFGHost": (i32, [C.c_uint32, vp]),
    "PTShadeTermsHost": (i32, [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp]),
    "PTShadeComposeHost": (i32, [vp, vp, vp, C.c_uint64, vp, C.c_uint32, vp]),
    # Part 22 (first hits shaded from baked lightmaps)
    "PTBindLightmaps": (i32, [vp, C.POINTER(abi.PTLightmapBinding), C.c_uint32]),
    "PTLightmapLookup": (i32, [vp, vp, vp, vp, C.c_uint64, vp, vp]),
    "PTShadeLightmapped": (i32, [vp, C.POINTER(abi.PTShadeInputs), vp, vp, vp, C.c_uint64, vp]),
    "PTShadeLightmappedFrame": (i32, [vp, C.POINTER(abi.PTFrameParams), C.POINTER(abi.PTShadeInputs), vp, vp]),
    "PTLightmapLookupHost": (i32, [C.POINTER(abi.PTLightmapBinding), C.c_uint32, vp, C.c_uint64, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp]),
    # Part 23 (lightmap UVs)
    "PTUnwrapCharts": (i32, [vp, C.POINTER(abi.PTUnwrapDesc), vp, vp, vp, C.c_uint32, u32p, C.POINTER(abi.PTUnwrapStats)]),
    "PTEmitChartUVs": (i32, [vp, C.POINTER(abi.PTUnwrapDesc), vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp]),
    "PTUnwrapChartsHost": (i32, [C.POINTER(abi.PTUnwrapDesc), vp, vp, vp, vp, C.c_uint32, u32p, C.POINTER(abi.PTUnwrapStats)]),
    "PTPackChartsHost": (i32, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp, u32p]),
    "PTEmitChartUVsHost": (i32, [C.POINTER(abi.PTUnwrapDesc), vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp]),
    # Part 24 (direct light at first hits)
    "PTDirectPairCount": (i32, [vp, C.c_uint32, u32p]),
    "PTDirectRays": (i32, [vp, C.POINTER(abi.PTDirectParams), vp, vp, vp, C.c_uint64, vp, vp]),
    "PTDirectAccumulate": (i32, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp]),
    "PTDirectLight": (i32, [vp, C.POINTER(abi.PTDirectParams), vp, vp, vp, C.c_uint64, vp]),
    "PTShadeMixed": (i32, [vp, C.POINTER(abi.PTShadeInputs), C.POINTER(abi.PTDirectParams), vp, vp, vp, C.c_uint64, vp]),
    "PTShadeMixedFrame": (i32, [vp, C.POINTER(abi.PTFrameParams), C.POINTER(abi.PTShadeInputs), C.POINTER(abi.PTDirectParams), vp, vp]),
    "PTDirectPairCountHost": (i32, [vp, C.c_uint32, C.c_uint32, u32p]),
    "PTDirectRaysHost": (i32, [C.POINTER(abi.PTDirectParams), vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp]),
    "PTDirectAccumulateHost": (i32, [vp, vp, vp, C.c_uint64, C.c_uint32, vp]),
    # Part 25 (direct light over many lights: the light grid)
    "PTBuildLightGrid": (i32, [vp, C.POINTER(abi.PTLightGridParams)]),
    "PTReadLightGrid": (i32, [vp, vp, vp, C.c_uint64, vp]),
    "PTLightGridInfo": (i32, [vp, C.POINTER(abi.PTLightGridStats)]),
    "PTDirectLightCulled": (i32, [vp, C.POINTER(abi.PTDirectParams), vp, vp, vp, C.c_uint64, vp]),
    "PTShadeMixedCulled": (i32, [vp, C.POINTER(abi.PTShadeInputs), C.POINTER(abi.PTDirectParams), vp, vp, vp, C.c_uint64, vp]),
    "PTShadeMixedFrameCulled": (i32, [vp, C.POINTER(abi.PTFrameParams), C.POINTER(abi.PTShadeInputs), C.POINTER(abi.PTDirectParams), vp, vp]),
    "PTBuildLightGridHost": (i32, [C.POINTER(abi.PTLightGridParams), vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]),
    "PTGetLastError": (C.c_char_p, []), "PTGetVersion": (i32, []),
}
EXPORTED_SYMBOLS = list(sig)

_lib = None


def build_library(verbose: bool = False):
    """Compile every HIP/C++ source of the plugin for gfx950 (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc")], stdout=out)
    return LIB_PATH


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build_library()
    # PyTorch-ROCm ships its own libamdhip64 under the same SONAME as /opt/rocm's.  Whichever loads first serves the whole
    # process; torch only finds its GPUs through its own copy, so a host that hands torch buffers to PTRenderPassTo must
    # let torch load first.  (The plugin itself is happy with either copy; a host without torch is unaffected.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError here = the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib




class PluginError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"plugin error {code}: {message}")
        self.code = code


def check(rc):
    if rc != abi.PT_OK:
        raise PluginError(rc, load_library().PTGetLastError().decode())
    return rc


HIP_MEMCPY_H2D, HIP_MEMCPY_D2H = 1, 2          # hipMemcpyKind
_hip = None


def hip_memcpy(dst: int, src: int, nbytes: int, kind: int):
    """hipMemcpy through the HIP runtime the plugin itself linked (found among the process's mapped files): synchronous
    copies to or from device pointers the plugin hands out (PTGetGuidePointer, PTGetFramePointer)."""
    global _hip
    if _hip is None:
        load_library()
        with open("/proc/self/maps") as f:
            paths = {l.split()[-1] for l in f if "libamdhip64.so" in l}
        if not paths:
            raise RuntimeError("the HIP runtime is not loaded")
        _hip = C.CDLL(sorted(paths)[0])
        _hip.hipMemcpy.restype = C.c_int
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = _hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), nbytes, kind)
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed: {rc}")


class TinyBVH:
    """Static mirror of the C# `TinyBVH` class (Assets/Scripts/util/TinyBVH.cs): same names, same meaning."""

    @staticmethod
    def BuildBVH(verticesPtr, count):
        return load_library().BuildBVH(verticesPtr, count)

    @staticmethod
    def DestroyBVH(index):
        load_library().DestroyBVH(index)

    @staticmethod
    def IsBVHReady(index):
        return bool(load_library().IsBVHReady(index))

    @staticmethod
    def GetBVHPtr(index):
        return load_library().GetBVHPtr(index)

    @staticmethod
    def GetCWBVHNodesSize(index):
        return load_library().GetCWBVHNodesSize(index)

    @staticmethod
    def GetCWBVHTrisSize(index):
        return load_library().GetCWBVHTrisSize(index)

    @staticmethod
    def GetCWBVHData(index):
        """-> (ok, bvhNodes IntPtr, bvhTris IntPtr), like the C# `out IntPtr` pair."""
        n, t = C.c_void_p(), C.c_void_p()
        ok = load_library().GetCWBVHData(index, C.byref(n), C.byref(t))
        return bool(ok), n.value, t.value

    @staticmethod
    def BuildTLAS(instances, instanceCount):
        return load_library().BuildTLAS(instances, instanceCount)

    @staticmethod
    def DestroyTLAS(index):
        load_library().DestroyTLAS(index)

    @staticmethod
    def IsTLASReady(index):
        return bool(load_library().IsTLASReady(index))

    @staticmethod
    def GetTLASNodesSize(index):
        return load_library().GetTLASNodesSize(index)

    @staticmethod
    def GetTLASData(index):
        n, i = C.c_void_p(), C.c_void_p()
        ok = load_library().GetTLASData(index, C.byref(n), C.byref(i))
        return bool(ok), n.value, i.value


def build_cwbvh(vertices: np.ndarray, device: int = None, timing: dict = None):
    """What BVHScene.OnCompleteReadback does with the plugin (BVHScene.cs:629-659): BuildBVH, read the sizes,
    fetch the borrowed pointers, copy the bytes out (Utilities.UploadFromPointer), DestroyBVH.
    device = None: BuildBVH (CPU, byte-identical to the reference plugin); device = k: PTBuildBVHDevice on HIP device k
    (same format, a different tree).  timing (optional dict) receives {"build_ms": ...}.
    Returns (nodes uint8[], tris uint8[])."""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    assert v.ndim == 2 and v.shape[1] == 4 and v.shape[0] % 3 == 0
    lib = load_library()
    if device is None:
        h = TinyBVH.BuildBVH(v.ctypes.data_as(C.c_void_p), v.shape[0] // 3)
        if h < 0:
            raise PluginError(h, "BuildBVH failed")
    else:
        h = lib.PTBuildBVHDevice(device, v.ctypes.data_as(C.c_void_p), v.shape[0] // 3)
        if h < 0:
            raise PluginError(h, "PTBuildBVHDevice failed: " + lib.PTGetBVHBuildError().decode())
    if timing is not None:
        timing["build_ms"] = float(lib.PTGetBVHBuildMs(h))
    try:
        nb, tb = TinyBVH.GetCWBVHNodesSize(h), TinyBVH.GetCWBVHTrisSize(h)
        ok, pn, pt = TinyBVH.GetCWBVHData(h)
        assert ok
        nodes = np.ctypeslib.as_array(C.cast(pn, C.POINTER(C.c_uint8)), shape=(nb,)).copy()
        tris = np.ctypeslib.as_array(C.cast(pt, C.POINTER(C.c_uint8)), shape=(tb,)).copy()
    finally:
        TinyBVH.DestroyBVH(h)
    return nodes, tris


def refit_cwbvh(handle_or_arrays, vertices: np.ndarray):
    """CWBVH refit on the host (include/ptmi_plugin.h Part 1): same topology, boxes and triangle records of `vertices`
    ((3 * triangles, 4) float32 in the primitive order the tree was built from).
    handle (int): PTRefitBVH refits the handle in place (GetCWBVHData then returns the refitted arrays); returns None.
    (nodes uint8[], tris uint8[]) as build_cwbvh returns them: PTRefitBVHArrays on copies; returns the refitted (nodes, tris)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    assert v.ndim == 2 and v.shape[1] == 4 and v.shape[0] % 3 == 0
    lib = load_library()
    if isinstance(handle_or_arrays, (int, np.integer)):
        if not lib.PTRefitBVH(int(handle_or_arrays), v.ctypes.data, v.shape[0] // 3):
            raise PluginError(abi.PT_ERR_INVALID_ARG, "PTRefitBVH failed: " + lib.PTGetBVHBuildError().decode())
        return None
    nodes, tris = (np.array(a, dtype=np.uint8, copy=True).reshape(-1) for a in handle_or_arrays)
    if not lib.PTRefitBVHArrays(nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes, v.ctypes.data, v.shape[0] // 3):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTRefitBVHArrays failed: " + lib.PTGetBVHBuildError().decode())
    return nodes, tris


def measure_cwbvh(arrays, triangle_count: int) -> dict:
    """Tree quality on the host (PTMeasureBVHArrays, include/ptmi_plugin.h Part 10): arrays = (nodes uint8[], tris uint8[]) as
    build_cwbvh returns them (zero nodes may be appended).  Returns nodeCapacity, nodeCount, triangleCount, levels, rootHalfArea
    and sahCost; raises PluginError for anything that is not a CWBVH of triangle_count triangles."""
    nodes, tris = (np.ascontiguousarray(np.asarray(a).view(np.uint8).reshape(-1)) for a in arrays)
    lib = load_library()
    q = abi.geometry_quality()
    if not lib.PTMeasureBVHArrays(nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes, int(triangle_count), C.byref(q)):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTMeasureBVHArrays failed: " + lib.PTGetBVHBuildError().decode())
    return q.as_dict()


def skin_desc(rest_vertices, joints, weights, joint_count: int, rest_attrs=None):
    """A PTSkinDesc over numpy arrays: rest_vertices (3T, 4) float32, joints (3T, 4) uint16, weights (3T, 4) float32, rest_attrs T
    abi.TRI_ATTR records or None.  Returns (desc, triangle count, the arrays the desc borrows -- keep them alive while it is used)."""
    v = np.ascontiguousarray(rest_vertices, dtype=np.float32)
    j = np.ascontiguousarray(joints, dtype=np.uint16)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    assert v.ndim == 2 and v.shape[1] == 4 and v.shape[0] % 3 == 0 and j.shape == v.shape and w.shape == v.shape
    a = None if rest_attrs is None else np.ascontiguousarray(rest_attrs)
    assert a is None or a.nbytes == v.shape[0] // 3 * 128
    d = abi.skin_desc()
    d.jointCount = int(joint_count)
    d.restVertices, d.joints, d.weights = v.ctypes.data, j.ctypes.data, w.ctypes.data
    d.restAttrs = None if a is None else a.ctypes.data
    return d, v.shape[0] // 3, (v, j, w, a)


def joint_palette(joint_matrices) -> np.ndarray:
    """(J, 3, 4) or (J, 12) -> C-contiguous float32 (J, 12): the rows of each joint's 3x4 matrix."""
    m = np.ascontiguousarray(joint_matrices, dtype=np.float32)
    assert m.ndim in (2, 3) and m.size % 12 == 0 and m.shape[1:] in ((3, 4), (12,)), m.shape
    return m.reshape(-1, 12)


def skin_vertices(rest_vertices, joints, weights, joint_matrices, rest_attrs=None):
    """Linear-blend skinning on the host (PTSkinVerticesHost, include/ptmi_plugin.h Part 11): the kernels' rule, byte for byte.
    joint_matrices: (J, 3, 4) or (J, 12).  Returns (vertices (3T, 4) float32, attrs or None, bounds (2, 3) float32: min, max);
    raises PluginError for a joint index >= J or non-finite weights, rest vertices or matrices."""
    m = joint_palette(joint_matrices)
    d, ntri, keep = skin_desc(rest_vertices, joints, weights, m.shape[0], rest_attrs)
    out = np.empty((ntri * 3, 4), np.float32)
    out_attrs = None if keep[3] is None else np.empty(keep[3].shape, keep[3].dtype)
    bounds = (C.c_float * 6)()
    lib = load_library()
    if not lib.PTSkinVerticesHost(C.byref(d), ntri, m.ctypes.data, out.ctypes.data, None if out_attrs is None else out_attrs.ctypes.data, bounds):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTSkinVerticesHost failed: " + lib.PTGetBVHBuildError().decode())
    return out, out_attrs, np.array(bounds, np.float32).reshape(2, 3)


def morph_csr(deltas):
    """Dense deltas (K, 3T, 3) float32 -> one CSR stream (offsets (3T + 1,) uint32, entries abi.MORPH_ENTRY[]): every corner lists, in
    ascending target order, the targets whose delta is not exactly (+0, +0, +0) -- compared as bit patterns, so a triple with a -0
    stays listed (acc + w * -0 can differ from acc in the sign of a zero).  Dropping the +0 triple never changes a position under
    finite weights; a normal or tangent corner left with no entry is copied instead of renormalised (include/ptmi_plugin.h Part 12)."""
    d = np.ascontiguousarray(deltas, dtype=np.float32)
    assert d.ndim == 3 and d.shape[2] == 3, d.shape
    listed = (d.view(np.uint32) != 0).any(axis=2).T                  # (3T, K): the bit patterns, so that -0 is listed
    offsets = np.zeros(d.shape[1] + 1, np.uint32)
    offsets[1:] = np.cumsum(listed.sum(axis=1))
    corner, target = np.nonzero(listed)                                # row-major: by corner, then ascending target
    entries = np.zeros(len(corner), abi.MORPH_ENTRY)
    entries["dx"], entries["dy"], entries["dz"] = d[target, corner, 0], d[target, corner, 1], d[target, corner, 2]
    entries["target"] = target
    return offsets, entries


def morph_stream(stream, corners: int):
    """A stream as PTMorphDesc takes it: None, a dense (K, 3T, 3) array (morph_csr) or an (offsets, entries) tuple -> (offsets, entries) or None"""
    if stream is None:
        return None
    if isinstance(stream, tuple):
        off, ent = np.ascontiguousarray(stream[0], dtype=np.uint32), np.ascontiguousarray(stream[1], dtype=abi.MORPH_ENTRY)
    else:
        off, ent = morph_csr(stream)
    assert off.shape == (corners + 1,), (off.shape, corners)
    return off, ent


def morph_desc(rest_vertices, target_count: int, position, normal=None, tangent=None, rest_attrs=None):
    """A PTMorphDesc over numpy arrays: rest_vertices (3T, 4) float32; position / normal / tangent each a dense (K, 3T, 3) array or an
    (offsets, entries) CSR tuple (normal and tangent may be None); rest_attrs T abi.TRI_ATTR records or None.  Returns (desc,
    triangle count, the arrays the desc borrows -- keep them alive while it is used)."""
    v = np.ascontiguousarray(rest_vertices, dtype=np.float32)
    assert v.ndim == 2 and v.shape[1] == 4 and v.shape[0] % 3 == 0
    a = None if rest_attrs is None else np.ascontiguousarray(rest_attrs)
    assert a is None or a.nbytes == v.shape[0] // 3 * 128
    streams = [morph_stream(s, v.shape[0]) for s in (position, normal, tangent)]
    assert streams[0] is not None, "the position stream is required (it may be empty)"
    d = abi.morph_desc()
    d.targetCount = int(target_count)
    d.restVertices = v.ctypes.data
    d.restAttrs = None if a is None else a.ctypes.data
    for name, s in zip(("position", "normal", "tangent"), streams):
        if s is not None:
            setattr(d, name + "Offsets", s[0].ctypes.data)
            setattr(d, name + "Entries", s[1].ctypes.data if len(s[1]) else None)
    return d, v.shape[0] // 3, (v, a, streams)


def morph_vertices(rest_vertices, position, weights, normal=None, tangent=None, rest_attrs=None, skin=None, joint_matrices=None, target_count=None):
    """Morph targets, then the skin, on the host (PTMorphVerticesHost, include/ptmi_plugin.h Part 12): the kernels' rule, byte for byte.
    weights: (K,) float32.  skin: (joints (3T, 4) uint16, weights (3T, 4) float32) with joint_matrices (J, 3, 4) or (J, 12), or both None.
    target_count: the morph's (default: the number of weights).
    Returns (vertices (3T, 4) float32, attrs or None, bounds (2, 3) float32: min, max); raises PluginError for a refused array."""
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    d, ntri, keep = morph_desc(rest_vertices, len(w) if target_count is None else target_count, position, normal, tangent, rest_attrs)
    if len(w) != d.targetCount or any(not isinstance(s, tuple) and s is not None and len(s) != len(w) for s in (position, normal, tangent)):
        raise PluginError(abi.PT_ERR_INVALID_ARG, f"{len(w)} weights do not match the targets")
    m = sd = keep2 = None
    if joint_matrices is not None:
        m = joint_palette(joint_matrices)
        if skin is not None:
            sd, _, keep2 = skin_desc(rest_vertices, skin[0], skin[1], m.shape[0])
    out = np.empty((ntri * 3, 4), np.float32)
    out_attrs = None if keep[1] is None else np.empty(keep[1].shape, keep[1].dtype)
    bounds = (C.c_float * 6)()
    lib = load_library()
    if not lib.PTMorphVerticesHost(C.byref(d), None if sd is None else C.byref(sd), ntri, w.ctypes.data, None if m is None else m.ctypes.data,
                                   out.ctypes.data, None if out_attrs is None else out_attrs.ctypes.data, bounds):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTMorphVerticesHost failed: " + lib.PTGetBVHBuildError().decode())
    return out, out_attrs, np.array(bounds, np.float32).reshape(2, 3)


def morph_layout(offsets, entries):
    """PTSetMorph's device layout of one CSR stream (PTMorphLayoutHost): -> (count (n,) uint32, sliceBase (ceil(n / 64) + 1,) uint32,
    stored entries abi.MORPH_ENTRY[]).  Slot s of corner c is stored[sliceBase[c // 64] + 64 * s + c % 64], applied only if s < count[c]."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    ent = np.ascontiguousarray(entries, dtype=abi.MORPH_ENTRY)
    n = len(off) - 1
    lib = load_library()
    stored = lib.PTMorphLayoutHost(off.ctypes.data, ent.ctypes.data, n, None, None, None)
    if stored >= 1 << 32:
        raise PluginError(abi.PT_ERR_INVALID_ARG, "the stored entries do not fit 32 bits")
    count, base, out = np.zeros(n, np.uint32), np.zeros((n + 63) // 64 + 1, np.uint32), np.zeros(stored, abi.MORPH_ENTRY)
    lib.PTMorphLayoutHost(off.ctypes.data, ent.ctypes.data, n, count.ctypes.data, base.ctypes.data, out.ctypes.data if stored else None)
    return count, base, out


def rasterize_chart(tris, attrs, width: int, height: int, uvs=None, local_to_world=None, world_to_local=None, seed: int = 0):
    """A lightmap chart on the host (PTRasterizeChartHost, include/ptmi_plugin.h Part 14): the kernels' rule, byte for byte.
    tris: the BLAS's triangle rows, (3T, 4) float32 or their bytes, as PTReadGeometry returns them; attrs: its T abi.TRI_ATTR records;
    uvs: (T, 6) float32 lightmap UVs by primitive, None = the records' uv0 .. uv2; local_to_world, world_to_local: 16 floats each in
    PTGpuInstance's memory order, or both None.  Returns (texels (n,) uint32 ascending, receivers (n, 8) float32 PTReceiver rows)."""
    t = np.ascontiguousarray(np.asarray(tris).view(np.uint8).reshape(-1))
    a = np.ascontiguousarray(attrs)
    ntri = t.nbytes // 48
    assert t.nbytes == ntri * 48 and a.nbytes == ntri * 128, (t.nbytes, a.nbytes)
    u = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(ntri, 6)
    m = [None if x is None else np.ascontiguousarray(x, dtype=np.float32).reshape(16) for x in (local_to_world, world_to_local)]
    ptr = lambda x: None if x is None else x.ctypes.data
    d = abi.chart_desc(width, height, ntri, seed=seed)
    lib = load_library()
    count = C.c_uint64()
    if not lib.PTRasterizeChartHost(C.byref(d), t.ctypes.data, a.ctypes.data, ptr(u), ptr(m[0]), ptr(m[1]), None, None, 0, C.byref(count)):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTRasterizeChartHost failed: " + lib.PTGetBVHBuildError().decode())
    texels, recv = np.empty(count.value, np.uint32), np.empty((count.value, 8), np.float32)
    if not lib.PTRasterizeChartHost(C.byref(d), t.ctypes.data, a.ctypes.data, ptr(u), ptr(m[0]), ptr(m[1]), texels.ctypes.data, recv.ctypes.data,
                                    count.value, C.byref(count)):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTRasterizeChartHost failed: " + lib.PTGetBVHBuildError().decode())
    return texels, recv


def resolve_lightmap(texels, irradiance, width: int, height: int, dilate: int = 2) -> np.ndarray:
    """Scatter and dilate on the host (PTResolveLightmapHost, include/ptmi_plugin.h Part 14): texels (n,) uint32, irradiance (n, 4)
    float32 PTIrradiance rows -> (height, width, 4) float32: rgb and w = 1 on the list's texels, 0.5 on dilated ones, 0 elsewhere.
    Raises PluginError for an index >= width * height or dilate > 16."""
    t = np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1)
    e = np.ascontiguousarray(irradiance, dtype=np.float32).reshape(-1, 4)
    assert len(t) == len(e), (t.shape, e.shape)
    image = np.empty((max(int(height), 0), max(int(width), 0), 4), np.float32)
    lib = load_library()
    if not lib.PTResolveLightmapHost(t.ctypes.data, e.ctypes.data, len(t), int(width), int(height), int(dilate), image.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTResolveLightmapHost failed: " + lib.PTGetBVHBuildError().decode())
    return image


def lightmap_denoise_params(samples: int, iterations: int = 5, denoise=None) -> abi.PTLightmapDenoiseParams:
    """The parameters of a lightmap denoise: `denoise` is None, a number of levels, a ready PTLightmapDenoiseParams, or a dict of
    abi.lightmap_denoise_params' keywords that overrides `iterations` and the suggested values."""
    if isinstance(denoise, abi.PTLightmapDenoiseParams):
        return denoise
    kw = {"iterations": iterations}
    if isinstance(denoise, dict):
        kw.update(denoise)
    elif denoise is not None:
        kw["iterations"] = int(denoise)
    return abi.lightmap_denoise_params(kw.pop("samples", samples), **kw)


def denoise_lightmap(texels, receivers, irradiance, width: int, height: int, samples: int, iterations: int = 5, params=None) -> np.ndarray:
    """The lightmap denoiser on the host (PTDenoiseLightmapHost, include/ptmi_plugin.h Part 17): the kernels' rule, byte for byte.
    texels (n,) uint32 unique texel indices, receivers (n, 8) float32 PTReceiver rows, irradiance (n, 4) float32 PTIrradiance rows of
    `samples` samples.  params: a dict of abi.lightmap_denoise_params' keywords, or a PTLightmapDenoiseParams.  Returns (n, 4)
    float32: the filtered rgb and the variance estimate of the filtered luminance.  Raises PluginError for what the twin refuses."""
    t = np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1)
    r = np.ascontiguousarray(receivers, dtype=np.float32).reshape(-1, 8)
    e = np.ascontiguousarray(irradiance, dtype=np.float32).reshape(-1, 4)
    assert len(t) == len(r) == len(e), (t.shape, r.shape, e.shape)
    p = lightmap_denoise_params(samples, iterations, params)
    out = np.empty((len(t), 4), np.float32)
    lib = load_library()
    if not lib.PTDenoiseLightmapHost(C.byref(p), t.ctypes.data, r.ctypes.data, e.ctypes.data, len(t), int(width), int(height), out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTDenoiseLightmapHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def adaptive_gather_params(adaptive, **defaults) -> abi.PTAdaptiveGather:
    """The parameters of an adaptive gather: `adaptive` is a number (the threshold), a ready PTAdaptiveGather, or a dict of
    abi.adaptive_gather's keywords; `defaults` fill what a number or a dict leaves out."""
    if isinstance(adaptive, abi.PTAdaptiveGather):
        return adaptive
    kw = dict(defaults)
    if isinstance(adaptive, dict):
        kw.update(adaptive)
    else:
        kw["threshold"] = float(adaptive)
    return abi.adaptive_gather(**kw)


def _active_list(active, entries):
    if active is None:
        return None, entries
    a = np.ascontiguousarray(active, dtype=np.uint32).reshape(-1)
    return a, len(a)


def select_receivers(accumulated, receivers, n: int, adaptive, active=None):
    """Step 2 of an adaptive gather on the host (PTSelectReceiversHost, include/ptmi_plugin.h Part 19): the kernels' rule, byte for
    byte.  accumulated (e, 4) float32 PTIrradiance rows of `n` samples each, receivers (e, 8) float32 PTReceiver rows, active (a,)
    uint32 indices into them (None: every entry); adaptive: what adaptive_gather_params takes.  Returns (indices (s,) uint32 of the
    entries that go on, in the list's order, their receivers (s, 8), stopped (3,) uint64: by threshold, by max_samples, non-finite).
    Raises PluginError for what the twin refuses."""
    acc = np.ascontiguousarray(accumulated, dtype=np.float32).reshape(-1, 4)
    recv = np.ascontiguousarray(receivers, dtype=np.float32).reshape(-1, 8)
    assert len(acc) == len(recv), (acc.shape, recv.shape)
    act, count = _active_list(active, len(acc))
    a = adaptive_gather_params(adaptive)
    out_active, out_recv = np.empty(count, np.uint32), np.empty((count, 8), np.float32)
    survivors, stopped = C.c_uint64(), (C.c_uint64 * 3)()
    lib = load_library()
    if not lib.PTSelectReceiversHost(C.byref(a), int(n), None if act is None else act.ctypes.data, count, acc.ctypes.data, recv.ctypes.data, len(acc),
                                     out_active.ctypes.data, out_recv.ctypes.data, C.byref(survivors), stopped):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTSelectReceiversHost failed: " + lib.PTGetBVHBuildError().decode())
    return out_active[:survivors.value].copy(), out_recv[:survivors.value].copy(), np.array(list(stopped), np.uint64)


def fold_irradiance(accumulated, n: int, fresh, m: int, active=None, counts=None):
    """Step 3 of an adaptive gather on the host (PTFoldIrradianceHost, Part 19) -- and the fold of two bakes of the same receivers
    over disjoint sample ranges: accumulated (e, 4) float32 PTIrradiance rows of `n` samples, fresh (a, 4) rows of `m` samples for the
    entries active names ((a,) uint32 unique indices; None: every entry).  n == 0 writes.  Returns the folded (e, 4) rows -- the
    running mean of rgb, the sum of m2 --, and with counts ((e,) uint32) also the counts with n + m at the folded entries."""
    acc = np.array(accumulated, dtype=np.float32, order="C").reshape(-1, 4)
    new = np.ascontiguousarray(fresh, dtype=np.float32).reshape(-1, 4)
    act, count = _active_list(active, len(acc))
    assert len(new) == count, (new.shape, count)
    cnt = None if counts is None else np.array(counts, dtype=np.uint32).reshape(-1)
    assert cnt is None or len(cnt) == len(acc), (cnt.shape, acc.shape)
    lib = load_library()
    if not lib.PTFoldIrradianceHost(None if act is None else act.ctypes.data, count, new.ctypes.data, int(m), int(n), len(acc), acc.ctypes.data,
                                    None if cnt is None else cnt.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTFoldIrradianceHost failed: " + lib.PTGetBVHBuildError().decode())
    return acc if cnt is None else (acc, cnt)


def equalise_irradiance(irradiance, counts, samples_eq: int) -> np.ndarray:
    """Step 5 of an adaptive gather on the host (PTEqualiseIrradianceHost, Part 19): rewrites m2 of every (n, 4) PTIrradiance row of
    counts[i] samples so that a consumer that assumes `samples_eq` samples everywhere -- the lightmap denoiser -- recovers the entry's
    own variance of the mean.  Not new statistics: an equalised list is not folded further."""
    e = np.ascontiguousarray(irradiance, dtype=np.float32).reshape(-1, 4)
    cnt = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    assert len(e) == len(cnt), (e.shape, cnt.shape)
    out = np.empty_like(e)
    lib = load_library()
    if not lib.PTEqualiseIrradianceHost(e.ctypes.data, cnt.ctypes.data, len(e), int(samples_eq), out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTEqualiseIrradianceHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def probe_rows(positions, seeds=None) -> np.ndarray:
    """(n, 4) float32 PTProbe rows -- position xyz, seed bits -- from (n, 3) positions; seeds None = the probe index."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    n = pos.shape[0]
    rows = np.empty((n, 4), np.float32)
    rows[:, 0:3] = pos
    sd = np.arange(n, dtype=np.uint32) if seeds is None else np.ascontiguousarray(np.asarray(seeds).astype(np.uint32)).reshape(n)
    rows[:, 3] = sd.view(np.float32)
    return rows


def probe_directions(positions, spp: int, first_sample: int = 0, seeds=None) -> np.ndarray:
    """The sample rays of SH light probes on the host (PTProbeDirectionsHost, include/ptmi_plugin.h Part 15): (n * spp, 8) float32
    PTRadianceRay rows, entry-major -- origin xyz, direction xyz, RNG state bits, 0 -- bit for bit what PTProbeRays writes."""
    rows = probe_rows(positions, seeds)
    rays = np.empty((rows.shape[0] * max(int(spp), 0), 8), np.float32)
    lib = load_library()
    if not lib.PTProbeDirectionsHost(rows.ctypes.data, rows.shape[0], first_sample & 0xFFFFFFFF, int(spp), rays.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTProbeDirectionsHost failed: " + lib.PTGetBVHBuildError().decode())
    return rays


def probe_project(directions, colours):
    """Project per-sample radiance onto SH bands 0 to 2 on the host (PTProbeProjectHost): directions, colours (n, spp, 3) float32 ->
    sh (n, 9, 3) float32 and m2 (n,), by the kernels' lane partials and fold tree; no delta lights (they need a scene)."""
    d = np.ascontiguousarray(directions, dtype=np.float32)
    c = np.ascontiguousarray(colours, dtype=np.float32)
    assert d.ndim == 3 and d.shape[2] == 3 and d.shape == c.shape, (d.shape, c.shape)
    n, spp = d.shape[0], d.shape[1]
    out = np.empty((n, 28), np.float32)
    lib = load_library()
    if not lib.PTProbeProjectHost(d.ctypes.data, c.ctypes.data, n, spp, out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTProbeProjectHost failed: " + lib.PTGetBVHBuildError().decode())
    return out[:, :27].reshape(n, 9, 3).copy(), out[:, 27].copy()


def probe_query_rows(normals, probes) -> np.ndarray:
    """(q, 4) float32 PTProbeQuery rows -- normal xyz, probe index bits"""
    nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    rows = np.empty((nrm.shape[0], 4), np.float32)
    rows[:, 0:3] = nrm
    rows[:, 3] = np.ascontiguousarray(np.asarray(probes).astype(np.uint32)).reshape(nrm.shape[0]).view(np.float32)
    return rows


def probe_coeff_rows(sh, m2=None) -> np.ndarray:
    """(n, 28) float32 PTProbeCoeffs rows from sh (n, 9, 3) and m2 (n,) (None: zeros)"""
    s = np.ascontiguousarray(sh, dtype=np.float32).reshape(-1, 27)
    rows = np.zeros((s.shape[0], 28), np.float32)
    rows[:, :27] = s
    if m2 is not None:
        rows[:, 27] = np.asarray(m2, np.float32).reshape(-1)
    return rows


def probe_irradiance(sh, normals, probes) -> np.ndarray:
    """Irradiance from probe coefficients on the host (PTProbeIrradianceHost): sh (n, 9, 3), normals (q, 3) unit, probes (q,)
    indices -> (q, 4) float32 PTIrradiance rows (m2 = 0); an index >= n gives zeros."""
    rows, q = probe_coeff_rows(sh), probe_query_rows(normals, probes)
    out = np.empty((q.shape[0], 4), np.float32)
    lib = load_library()
    if not lib.PTProbeIrradianceHost(rows.ctypes.data, rows.shape[0], q.ctypes.data, q.shape[0], out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTProbeIrradianceHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def probe_grid_desc(origin, spacing, counts, wrap: bool = True, visibility: bool = True, normal_bias: float = 0.0) -> abi.PTProbeGrid:
    """The PTProbeGrid (include/ptmi_plugin.h Part 16) of a regular lattice: probe (ix, iy, iz) at origin + i * spacing, x fastest."""
    g = abi.PTProbeGrid()
    for a in range(3):
        g.origin[a], g.spacing[a], g.counts[a] = float(origin[a]), float(spacing[a]), int(counts[a])
    g.flags = (abi.PT_GRID_WRAP if wrap else 0) | (abi.PT_GRID_VISIBILITY if visibility else 0)
    g.normalBias = float(normal_bias)
    return g


def probe_grid_positions(grid: abi.PTProbeGrid) -> np.ndarray:
    """The rule's fp32 position Q of every probe of a grid: Q[a] = origin[a] + (float)i_a * spacing[a], one float32 multiply and
    one add.  Returns (nx * ny * nz, 3) float32, x fastest, as probe_sh() and probe_depth() take them."""
    axes = [(np.float32(grid.origin[a]) + np.arange(grid.counts[a], dtype=np.uint32).astype(np.float32) * np.float32(grid.spacing[a])).astype(np.float32)
            for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.float32)


def receiver_rows(positions, normals) -> np.ndarray:
    """(n, 8) float32 PTReceiver rows -- position xyz, seed 0, normal xyz, 0 -- for a lookup, which ignores the seed"""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    assert pos.shape == nrm.shape, (pos.shape, nrm.shape)
    rows = np.zeros((pos.shape[0], 8), np.float32)
    rows[:, 0:3], rows[:, 4:7] = pos, nrm
    return rows


def probe_depth_project(positions, distances, max_distance: float, first_sample: int = 0, seeds=None) -> np.ndarray:
    """The octahedral depth records of probes on the host (PTProbeDepthProjectHost, include/ptmi_plugin.h Part 16): distances
    (n, spp) float32, the closest-hit t of every sample's ray (max_distance on a miss); the directions are made from the seeds.
    Returns (n, 64, 2) float32: per texel the weighted mean distance and mean squared distance, bit for bit what PTProbeDepth
    writes for the same distances."""
    rows = probe_rows(positions, seeds)
    d = np.ascontiguousarray(distances, dtype=np.float32)
    assert d.ndim == 2 and d.shape[0] == rows.shape[0], (d.shape, rows.shape)
    out = np.empty((rows.shape[0], 64, 2), np.float32)
    lib = load_library()
    if not lib.PTProbeDepthProjectHost(rows.ctypes.data, rows.shape[0], first_sample & 0xFFFFFFFF, d.shape[1], d.ctypes.data, max_distance, out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTProbeDepthProjectHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def probe_placement_rows(offsets=None, states=None, n: int = None) -> np.ndarray:
    """(n, 4) float32 PTProbePlacement rows -- offset xyz, state bits -- from (n, 3) offsets and (n,) states (None: zeros)"""
    if offsets is None:
        rows = np.zeros((int(n), 4), np.float32)
    else:
        off = np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1, 3)
        rows = np.zeros((off.shape[0], 4), np.float32)
        rows[:, 0:3] = off
    if states is not None:
        rows[:, 3] = np.ascontiguousarray(np.asarray(states).astype(np.uint32)).reshape(rows.shape[0]).view(np.float32)
    return rows


def probe_place_step(positions, hits, surfaces, params: abi.PTProbePlaceParams, move: bool = True, offsets=None, first_sample: int = 0, seeds=None):
    """One step of probe placement on the host (PTProbePlaceStepHost, include/ptmi_plugin.h Part 18).  hits (n * spp, 4) and
    surfaces (n * spp, 12) float32 are the PTRayHit and PTRaySurface rows, entry-major, that trace_rays(surface=True) returns for the
    rays {P + o, w_j, params.maxDistance}; offsets (n, 3): the stored offsets (None: zeros), read as the rule reads them.
    Returns (offsets (n, 3) float32, states (n,) uint32, stats (n,) records of abi.PLACE_STATS_DTYPE): with move the offsets after
    the step; states and stats describe the offsets the records were traced from."""
    rows = probe_rows(positions, seeds)
    n = rows.shape[0]
    h = np.ascontiguousarray(hits, dtype=np.float32).reshape(-1, 4)
    s = np.ascontiguousarray(surfaces, dtype=np.float32).reshape(-1, 12)
    assert h.shape[0] == s.shape[0] and (n == 0 or h.shape[0] % n == 0), (h.shape, s.shape, n)
    spp = h.shape[0] // n if n else 1
    pl = probe_placement_rows(offsets, None, n)
    assert pl.shape[0] == n, (pl.shape, n)
    stats = np.zeros(n, abi.PLACE_STATS_DTYPE)
    lib = load_library()
    if not lib.PTProbePlaceStepHost(rows.ctypes.data, n, first_sample & 0xFFFFFFFF, spp, C.byref(params), h.ctypes.data, s.ctypes.data, 1 if move else 0,
                                    pl.ctypes.data, stats.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTProbePlaceStepHost failed: " + lib.PTGetBVHBuildError().decode())
    return pl[:, 0:3].copy(), pl[:, 3].copy().view(np.uint32), stats


def probe_grid_irradiance(grid: abi.PTProbeGrid, sh, depth, positions=None, normals=None, receivers=None, placement=None) -> np.ndarray:
    """A probe volume's lookup on the host (PTProbeGridIrradianceHost): sh (n, 9, 3), depth (n, 64, 2) or None (without
    PT_GRID_VISIBILITY), n the grid's probes; positions and unit normals (q, 3), or ready-made (q, 8) PTReceiver rows.
    placement: None, or (n, 4) float32 PTProbePlacement rows (probe_placement_rows) for the placed lookup of Part 18
    (PTProbeGridIrradiancePlacedHost): a probe marked PT_PROBE_INSIDE is left out, a live one weighs in from its placed position.
    Returns (q, 4) float32: irradiance rgb and the support sumW."""
    rows = probe_coeff_rows(sh)
    recv = receiver_rows(positions, normals) if receivers is None else np.ascontiguousarray(receivers, dtype=np.float32).reshape(-1, 8)
    n = int(grid.counts[0]) * int(grid.counts[1]) * int(grid.counts[2])
    d = None
    if depth is not None:
        d = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1, 128)
    if 1 <= min(grid.counts) and max(grid.counts) <= abi.PT_GRID_MAX_AXIS:           # (the twin refuses other counts itself)
        assert rows.shape[0] == n and (d is None or d.shape[0] == n), (rows.shape, n)
    out = np.empty((recv.shape[0], 4), np.float32)
    lib = load_library()
    if placement is not None:
        pl = np.ascontiguousarray(placement, dtype=np.float32).reshape(-1, 4)
        assert pl.shape[0] == rows.shape[0], (pl.shape, rows.shape)
        if not lib.PTProbeGridIrradiancePlacedHost(C.byref(grid), rows.ctypes.data, None if d is None else d.ctypes.data, pl.ctypes.data, recv.ctypes.data,
                                                   recv.shape[0], out.ctypes.data):
            raise PluginError(abi.PT_ERR_INVALID_ARG, "PTProbeGridIrradiancePlacedHost failed: " + lib.PTGetBVHBuildError().decode())
        return out
    if not lib.PTProbeGridIrradianceHost(C.byref(grid), rows.ctypes.data, None if d is None else d.ctypes.data, recv.ctypes.data, recv.shape[0], out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTProbeGridIrradianceHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def reflection_texel_count(res: int, levels: int = 1) -> int:
    """Texels of one probe's map with `levels` levels (include/ptmi_plugin.h Part 20): level k is (res >> k) squared; levels = 1 is
    a base map."""
    return sum((int(res) >> k) ** 2 for k in range(int(levels)))


def reflection_directions(positions, res: int, spp: int, first_sample: int = 0, seeds=None) -> np.ndarray:
    """The sample rays of reflection probes on the host (PTReflectionDirectionsHost): (n * res * res * spp, 8) float32 PTRadianceRay
    rows, slot-major -- row (i * res * res + t) * spp + j is sample first_sample + j of texel t of probe i --, bit for bit what
    PTReflectionRays writes."""
    rows = probe_rows(positions, seeds)
    ok = abi.PT_REFLECTION_MIN_RES <= int(res) <= abi.PT_REFLECTION_MAX_RES           # (the twin refuses another res itself)
    rays = np.empty((rows.shape[0] * int(res) ** 2 * max(int(spp), 0) if ok else 0, 8), np.float32)
    lib = load_library()
    if not lib.PTReflectionDirectionsHost(rows.ctypes.data, rows.shape[0], int(res), first_sample & 0xFFFFFFFF, int(spp), rays.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTReflectionDirectionsHost failed: " + lib.PTGetBVHBuildError().decode())
    return rays


def reflection_fold(radiance, n: int, res: int) -> np.ndarray:
    """Fold per-sample radiance into base texels on the host (PTReflectionFoldHost): radiance (n * res * res * spp, 4) float32
    PTRadiance rows, slot-major -> (n, res * res, 4) float32: mean rgb and the sum of squared luminances."""
    r = np.ascontiguousarray(radiance, dtype=np.float32).reshape(-1, 4)
    texels = int(n) * int(res) ** 2
    assert texels > 0 and r.shape[0] % texels == 0, (r.shape, n, res)
    out = np.empty((int(n), int(res) ** 2, 4), np.float32)
    lib = load_library()
    if not lib.PTReflectionFoldHost(r.ctypes.data, int(n), int(res), r.shape[0] // texels, out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTReflectionFoldHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def reflection_prefilter(base, res: int, levels: int) -> np.ndarray:
    """The GGX prefilter on the host (PTReflectionPrefilterHost): base (n, res * res, 4) float32 -> (n, reflection_texel_count(res,
    levels), 4) float32, the levels in ascending order; level k stands for roughness k / (levels - 1)."""
    b = np.ascontiguousarray(base, dtype=np.float32)
    assert b.ndim == 3 and b.shape[2] == 4, b.shape
    ok = abi.PT_REFLECTION_MIN_RES <= int(res) <= abi.PT_REFLECTION_MAX_RES and 1 <= int(levels) <= 8
    if ok:
        assert b.shape[1] == int(res) ** 2, (b.shape, res)
    out = np.empty((b.shape[0], reflection_texel_count(res, levels) if ok else 1, 4), np.float32)
    lib = load_library()
    if not lib.PTReflectionPrefilterHost(b.ctypes.data, b.shape[0], int(res), int(levels), out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTReflectionPrefilterHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def reflection_query_rows(directions, roughness, probes, positions=None) -> np.ndarray:
    """(q, 8) float32 PTReflectionQuery rows -- position xyz (None: zeros), roughness, direction xyz, probe index bits"""
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    q = d.shape[0]
    rows = np.zeros((q, 8), np.float32)
    if positions is not None:
        rows[:, 0:3] = np.ascontiguousarray(positions, dtype=np.float32).reshape(q, 3)
    rows[:, 3] = np.broadcast_to(np.asarray(roughness, np.float32), (q,))
    rows[:, 4:7] = d
    rows[:, 7] = np.ascontiguousarray(np.broadcast_to(np.asarray(probes).astype(np.uint32), (q,))).view(np.float32)
    return rows


def reflection_box_rows(bmin, bmax) -> np.ndarray:
    """(n, 8) float32 PTReflectionBox rows -- bmin xyz, 0, bmax xyz, 0"""
    lo = np.ascontiguousarray(bmin, dtype=np.float32).reshape(-1, 3)
    rows = np.zeros((lo.shape[0], 8), np.float32)
    rows[:, 0:3], rows[:, 4:7] = lo, np.ascontiguousarray(bmax, dtype=np.float32).reshape(-1, 3)
    return rows


def reflection_lookup(maps, res: int, levels: int, directions=None, roughness=0.0, probes=0, positions=None, probe_positions=None, boxes=None,
                      queries=None) -> np.ndarray:
    """A reflection probe's lookup on the host (PTReflectionLookupHost): maps (n, reflection_texel_count(res, levels), 4) float32;
    directions (q, 3), roughness and probes one number or (q,), or ready-made (q, 8) PTReflectionQuery rows.  boxes: (n, 8)
    PTReflectionBox rows (reflection_box_rows) for the box projection, which then needs probe_positions (n, 3) and the queries'
    positions.  Returns (q, 4) float32: rgb and 1 (zeros for a probe index >= n)."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    assert m.ndim == 3 and m.shape[2] == 4, m.shape
    qr = reflection_query_rows(directions, roughness, probes, positions) if queries is None else np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 8)
    pr = None if probe_positions is None else probe_rows(probe_positions)
    bx = None if boxes is None else np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 8)
    assert (pr is None or pr.shape[0] == m.shape[0]) and (bx is None or bx.shape[0] == m.shape[0]), (m.shape, pr is None, bx is None)
    out = np.empty((qr.shape[0], 4), np.float32)
    lib = load_library()
    if not lib.PTReflectionLookupHost(m.ctypes.data if m.shape[0] else None, m.shape[0], int(res), int(levels), None if pr is None else pr.ctypes.data,
                                      None if bx is None else bx.ctypes.data, qr.ctypes.data, qr.shape[0], out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTReflectionLookupHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def bake_dfg(res: int = 32) -> np.ndarray:
    """The split-sum DFG table on the host (PTBakeDFGHost; include/ptmi_plugin.h Part 21): (res, res, 2) float32, row j = perceptual
    roughness (j + 0.5) / res, column i = N.V (i + 0.5) / res, {scale, bias} of F0.  res is 16, 32 or 64."""
    ok = int(res) in abi.PT_SHADE_DFG_RES                                     # (the twin refuses another res itself)
    out = np.empty((int(res), int(res), 2) if ok else (1, 1, 2), np.float32)
    lib = load_library()
    if not lib.PTBakeDFGHost(int(res), out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTBakeDFGHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def shade_terms(materials, rays, surfaces, probe_positions=None, boxes=None):
    """A hit's shading terms and lookup queries on the host (PTShadeTermsHost): materials (n, 12) float32 PTShadeMaterial rows as
    PathTracer.shade_surfaces returns them, rays (n, 8) PTRay rows, surfaces (n, 12) PTRaySurface rows; probe_positions (k, 3) or
    None (no probes), boxes (k, 8) PTReflectionBox rows or None.  Returns terms (n, 12), receivers (n, 8) and queries (n, 8),
    all float32."""
    m = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 12)
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    s = np.ascontiguousarray(surfaces, dtype=np.float32).reshape(-1, 12)
    n = m.shape[0]
    assert r.shape[0] == n and s.shape[0] == n, (m.shape, r.shape, s.shape)
    pr = None if probe_positions is None else probe_rows(probe_positions)
    bx = None if boxes is None else np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 8)
    assert bx is None or pr is None or bx.shape[0] == pr.shape[0], (bx.shape, pr.shape)
    terms, recv, queries = np.empty((n, 12), np.float32), np.empty((n, 8), np.float32), np.empty((n, 8), np.float32)
    lib = load_library()
    if not lib.PTShadeTermsHost(m.ctypes.data, r.ctypes.data, s.ctypes.data, n, None if pr is None or not pr.shape[0] else pr.ctypes.data,
                                None if bx is None else bx.ctypes.data, 0 if pr is None else pr.shape[0], terms.ctypes.data, recv.ctypes.data,
                                queries.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTShadeTermsHost failed: " + lib.PTGetBVHBuildError().decode())
    return terms, recv, queries


def shade_compose(terms, irradiance, reflection, dfg) -> np.ndarray:
    """The compose step on the host (PTShadeComposeHost): terms (n, 12), irradiance (n, 4), reflection (n, 4), the DFG table
    (res, res, 2), all float32.  Returns (n, 4) float32: rgb and 1 (zeros for a miss)."""
    t = np.ascontiguousarray(terms, dtype=np.float32).reshape(-1, 12)
    e = np.ascontiguousarray(irradiance, dtype=np.float32).reshape(-1, 4)
    s = np.ascontiguousarray(reflection, dtype=np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(dfg, dtype=np.float32)
    assert d.ndim == 3 and d.shape[0] == d.shape[1] and d.shape[2] == 2, d.shape
    n = t.shape[0]
    assert e.shape[0] == n and s.shape[0] == n, (t.shape, e.shape, s.shape)
    out = np.empty((n, 4), np.float32)
    lib = load_library()
    if not lib.PTShadeComposeHost(t.ctypes.data, e.ctypes.data, s.ctypes.data, n, d.ctypes.data, d.shape[0], out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTShadeComposeHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


def lightmap_bindings(bindings):
    """(a ctypes array of PTLightmapBinding or None, what it points into) from a list of dicts for the host twin: image (h, w, 4)
    float32, first_prim, prim_count, and optionally instance (None: any), uvs ((prim_count, 6) float32 or None: the attribute
    records'), two_sided.  The arrays are copied to 16-byte aligned memory."""
    def aligned(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        buf = np.empty(a.nbytes + 16, np.uint8)
        off = (-buf.ctypes.data) % 16
        out = buf[off:off + a.nbytes].view(np.float32).reshape(a.shape)
        out[...] = a
        return out
    if not bindings:
        return None, []
    table, keep = (abi.PTLightmapBinding * len(bindings))(), []
    for b, d in zip(table, bindings):
        image = aligned(d["image"])
        assert image.ndim == 3 and image.shape[2] == 4, image.shape
        uvs = None if d.get("uvs") is None else aligned(np.asarray(d["uvs"], np.float32).reshape(-1, 6))
        keep += [image, uvs]
        b.firstPrim, b.primCount = int(d["first_prim"]), int(d["prim_count"])
        b.instance = abi.PT_LIGHTMAP_NONE if d.get("instance") is None else int(d["instance"])
        b.flags = int(d.get("flags", abi.PT_LIGHTMAP_TWO_SIDED if d.get("two_sided") else 0))
        b.height, b.width = image.shape[0], image.shape[1]
        b.dImage = image.ctypes.data
        b.dUvs = None if uvs is None else uvs.ctypes.data
    return table, keep


def lightmap_lookup(bindings, tri_attrs, material_count: int, rays, hits, surfaces):
    """The lightmap lookup on the host (PTLightmapLookupHost; include/ptmi_plugin.h Part 22).  bindings: a list of dicts as
    lightmap_bindings takes them; tri_attrs: the scene's TRI_ATTRS records (or None when every binding has uvs) -- spans are
    checked against their count; rays (n, 8), hits (n, 4), surfaces (n, 12) float32 rows as PathTracer.trace_rays(surface=True)
    takes and returns them.  Returns (irradiance (n, 4) float32, binding (n,) uint32): rgb and 0 where a lightmap was found, zero
    bits and PT_LIGHTMAP_NONE elsewhere."""
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    h = np.ascontiguousarray(hits, dtype=np.float32).reshape(-1, 4)
    s = np.ascontiguousarray(surfaces, dtype=np.float32).reshape(-1, 12)
    n = r.shape[0]
    assert h.shape[0] == n and s.shape[0] == n, (r.shape, h.shape, s.shape)
    table, keep = lightmap_bindings(bindings)
    attrs = None if tri_attrs is None else np.ascontiguousarray(tri_attrs)
    assert attrs is None or attrs.dtype.itemsize == 128, attrs.dtype
    out, which = np.empty((n, 4), np.float32), np.empty(n, np.uint32)
    lib = load_library()
    if not lib.PTLightmapLookupHost(table, 0 if table is None else len(table), None if attrs is None else attrs.ctypes.data, 0 if attrs is None else attrs.shape[0],
                                    int(material_count), r.ctypes.data, h.ctypes.data, s.ctypes.data, n, out.ctypes.data, which.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTLightmapLookupHost failed: " + lib.PTGetBVHBuildError().decode())
    del keep
    return out, which


# ---- direct light at first hits on the host (include/ptmi_plugin.h Part 24)
def _light_rows(lights):
    return np.ascontiguousarray(lights, dtype=np.float32).reshape(-1, 16)


def direct_pair_count(lights, strata: int = 1) -> int:
    """PTDirectPairCountHost: the pairs one entry has with these lights -- (k, 16) float32 PTLight records --: 1 per point or spot
    light, strata * strata per rectangle light, none for any other type."""
    L = _light_rows(lights)
    n = C.c_uint32()
    lib = load_library()
    if not lib.PTDirectPairCountHost(L.ctypes.data if L.shape[0] else None, L.shape[0], int(strata), C.byref(n)):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTDirectPairCountHost failed: " + lib.PTGetBVHBuildError().decode())
    return n.value


def direct_rays(lights, rays, terms, receivers, strata: int = 1, seed: int = 0, centered: bool = False, min_alpha: float = 0.0, params=None):
    """The pairs' shadow rays and contributions on the host (PTDirectRaysHost): lights (k, 16) PTLight records, rays (n, 8) PTRay
    rows, terms (n, 12) and receivers (n, 8) as PathTracer.shade_surfaces returns them.  params: a ready PTDirectParams instead of
    the keywords.  Returns (pair rays (n * pairs, 8), contributions (n * pairs, 4)), float32; a pair that does not count has
    tmax = 0 and zero contribution."""
    L = _light_rows(lights)
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    t = np.ascontiguousarray(terms, dtype=np.float32).reshape(-1, 12)
    rc = np.ascontiguousarray(receivers, dtype=np.float32).reshape(-1, 8)
    n = r.shape[0]
    assert t.shape[0] == n and rc.shape[0] == n, (r.shape, t.shape, rc.shape)
    p = params if params is not None else abi.direct_params(strata, seed, centered, min_alpha)
    lib = load_library()
    lights_ptr = L.ctypes.data if L.shape[0] else None
    pairs = C.c_uint32()
    ok = lib.PTDirectPairCountHost(lights_ptr, L.shape[0], p.strata, C.byref(pairs))
    out_rays, contrib = np.empty((n * pairs.value, 8), np.float32), np.empty((n * pairs.value, 4), np.float32)
    if not ok or not lib.PTDirectRaysHost(C.byref(p), lights_ptr, L.shape[0], r.ctypes.data, t.ctypes.data, rc.ctypes.data, n, out_rays.ctypes.data,
                                          contrib.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTDirectRaysHost failed: " + lib.PTGetBVHBuildError().decode())
    return out_rays, contrib


def direct_accumulate(terms, contrib, pair_hits, pairs_per_entry: int) -> np.ndarray:
    """The sum over the visible pairs on the host (PTDirectAccumulateHost): terms (n, 12), contrib (n * pairs, 4) as direct_rays
    returns it, pair_hits (n * pairs, 4) PTRayHit rows of an any-hit query over the pair rays.  Returns (n, 4) float32: the direct
    light and 1, zeros for a miss."""
    t = np.ascontiguousarray(terms, dtype=np.float32).reshape(-1, 12)
    c = np.ascontiguousarray(contrib, dtype=np.float32).reshape(-1, 4)
    h = np.ascontiguousarray(pair_hits, dtype=np.float32).reshape(-1, 4)
    n = t.shape[0]
    assert c.shape[0] == n * pairs_per_entry and h.shape[0] == n * pairs_per_entry, (t.shape, c.shape, h.shape, pairs_per_entry)
    out = np.empty((n, 4), np.float32)
    lib = load_library()
    if not lib.PTDirectAccumulateHost(t.ctypes.data, c.ctypes.data, h.ctypes.data, n, int(pairs_per_entry), out.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTDirectAccumulateHost failed: " + lib.PTGetBVHBuildError().decode())
    return out


# ---- the light grid on the host (include/ptmi_plugin.h Part 25)
def build_light_grid(lights, origin=None, cell_size=None, dims=None, params=None):
    """PTBuildLightGridHost: the grid PathTracer.build_light_grid builds on the GPU, byte for byte.  lights: (k, 16) float32 PTLight
    records; the grid is dims[0] x dims[1] x dims[2] cubes of cell_size from origin (or a ready PTLightGridParams).  Returns
    (offsets (cells + 2,), indices (total,), rect_before (k + 1,)), uint32: the list of cell c is indices[offsets[c]:offsets[c + 1]],
    the overflow cell's -- every light -- comes last."""
    L = _light_rows(lights)
    p = params if params is not None else abi.light_grid_params(origin, cell_size, dims)
    lib = load_library()
    lights_ptr = L.ctypes.data if L.shape[0] else None
    cells = int(p.dims[0]) * int(p.dims[1]) * int(p.dims[2])
    ok = 0 < cells <= abi.PT_LIGHT_GRID_MAX_CELLS                       # else the call below refuses, with nothing written
    offsets, rect_before = np.zeros((cells if ok else 0) + 2, np.uint32), np.zeros(L.shape[0] + 1, np.uint32)
    total = C.c_uint64()
    if not lib.PTBuildLightGridHost(C.byref(p), lights_ptr, L.shape[0], offsets.ctypes.data, None, 0, rect_before.ctypes.data, C.byref(total)):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTBuildLightGridHost failed: " + lib.PTGetBVHBuildError().decode())
    indices = np.zeros(total.value, np.uint32)
    if not lib.PTBuildLightGridHost(C.byref(p), lights_ptr, L.shape[0], offsets.ctypes.data, indices.ctypes.data if total.value else None, total.value,
                                    rect_before.ctypes.data, None):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTBuildLightGridHost failed: " + lib.PTGetBVHBuildError().decode())
    return offsets, indices, rect_before


def build_tlas(instances: np.ndarray):
    inst = np.ascontiguousarray(instances)
    assert inst.dtype == abi.BLAS_INSTANCE
    n = inst.shape[0]
    h = TinyBVH.BuildTLAS(inst.ctypes.data_as(C.c_void_p), n)
    if h < 0:
        raise PluginError(h, "BuildTLAS failed")
    try:
        nb = TinyBVH.GetTLASNodesSize(h)
        ok, pn, pi = TinyBVH.GetTLASData(h)
        assert ok
        nodes = np.ctypeslib.as_array(C.cast(pn, C.POINTER(C.c_uint8)), shape=(nb,)).copy()
        idx = np.ctypeslib.as_array(C.cast(pi, C.POINTER(C.c_uint32)), shape=(n,)).copy()
    finally:
        TinyBVH.DestroyTLAS(h)
    return nodes, idx


# ---- lightmap UVs on the host (include/ptmi_plugin.h Part 23)
def _unwrap_sources(tris, vertices):
    """(tris bytes or None, vertices (3T, 4) or None, T) of the twins' two corner sources"""
    t = None if tris is None else np.ascontiguousarray(np.asarray(tris).view(np.uint8).reshape(-1))
    v = None if vertices is None else np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 4)
    assert t is not None or v is not None, "the triangle rows or the vertices"
    ntri = v.shape[0] // 3 if v is not None else t.nbytes // 48
    assert (v is None or v.shape[0] == ntri * 3) and (t is None or t.nbytes == ntri * 48), (ntri, None if t is None else t.nbytes)
    return t, v, ntri


def unwrap_charts(tris, vertices=None, return_stats: bool = False):
    """The charts of a mesh on the host (PTUnwrapChartsHost, include/ptmi_plugin.h Part 23): the kernels' rule, byte for byte.
    tris: the BLAS's triangle rows, (3T, 4) float32 or their bytes, as PTReadGeometry returns them (None with vertices);
    vertices: (3T, 4) float32 in primitive order, None = the records' v0, v0 + e1, v0 + e2.  Returns (chart_of_prim (T,) uint32 with
    abi.PT_UNWRAP_NO_CHART for excluded triangles, charts: records of abi.UNWRAP_CHART_DTYPE), and with return_stats a dict."""
    t, v, ntri = _unwrap_sources(tris, vertices)
    ptr = lambda x: None if x is None else x.ctypes.data
    lib = load_library()
    d = abi.unwrap_desc(ntri)
    count, st = C.c_uint32(), abi.PTUnwrapStats()
    if not lib.PTUnwrapChartsHost(C.byref(d), ptr(t), ptr(v), None, None, 0, C.byref(count), C.byref(st)):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTUnwrapChartsHost failed: " + lib.PTGetBVHBuildError().decode())
    of, charts = np.empty(ntri, np.uint32), np.zeros(count.value, abi.UNWRAP_CHART_DTYPE)
    if not lib.PTUnwrapChartsHost(C.byref(d), ptr(t), ptr(v), of.ctypes.data, charts.ctypes.data, count.value, C.byref(count), C.byref(st)):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTUnwrapChartsHost failed: " + lib.PTGetBVHBuildError().decode())
    return (of, charts, st.as_dict()) if return_stats else (of, charts)


def pack_charts(charts, width: int, height: int, texels_per_unit: float, padding: int = 2):
    """The shelf packer (PTPackChartsHost, include/ptmi_plugin.h Part 23; a pure host function).  charts: records of
    abi.UNWRAP_CHART_DTYPE -- of one mesh, or the concatenated records of several.  Returns (origins (n, 2) int32: x, y per chart,
    or None when the charts do not fit, rows_used: the rows the shelves take, set whenever every chart's width fits -- also past the
    height --, else 0).  Raises PluginError for a size, padding or density out of range."""
    c = np.ascontiguousarray(charts, dtype=abi.UNWRAP_CHART_DTYPE).reshape(-1)
    origins, rows = np.zeros((len(c), 2), np.int32), C.c_uint32()
    lib = load_library()
    if lib.PTPackChartsHost(c.ctypes.data if len(c) else None, len(c), int(width), int(height), int(padding), float(texels_per_unit),
                            origins.ctypes.data if len(c) else None, C.byref(rows)):
        return origins, rows.value
    msg = lib.PTGetBVHBuildError().decode()
    if "rows" in msg or "wider" in msg:
        return None, rows.value
    raise PluginError(abi.PT_ERR_INVALID_ARG, "PTPackChartsHost failed: " + msg)


def emit_chart_uvs(tris, chart_of_prim, charts, origins, width: int, height: int, texels_per_unit: float, padding: int = 2, vertices=None):
    """The lightmap UVs of a mesh on the host (PTEmitChartUVsHost, include/ptmi_plugin.h Part 23).  tris, vertices: as unwrap_charts
    takes them; chart_of_prim: its first result; charts, origins: the mesh's slice of what pack_charts placed.  Returns (T, 6)
    float32: u0 v0 u1 v1 u2 v2 per primitive, six NaNs for an excluded one."""
    t, v, ntri = _unwrap_sources(tris, vertices)
    of = np.ascontiguousarray(chart_of_prim, dtype=np.uint32).reshape(ntri)
    c = np.ascontiguousarray(charts, dtype=abi.UNWRAP_CHART_DTYPE).reshape(-1)
    o = np.ascontiguousarray(origins, dtype=np.int32).reshape(len(c), 2)
    ptr = lambda x: None if x is None or not x.size else x.ctypes.data
    uvs = np.empty((ntri, 6), np.float32)
    lib = load_library()
    d = abi.unwrap_desc(ntri)
    if not lib.PTEmitChartUVsHost(C.byref(d), ptr(t), ptr(v), of.ctypes.data, ptr(c), ptr(o), len(c), int(width), int(height), int(padding),
                                  float(texels_per_unit), uvs.ctypes.data):
        raise PluginError(abi.PT_ERR_INVALID_ARG, "PTEmitChartUVsHost failed: " + lib.PTGetBVHBuildError().decode())
    return uvs


def fit_chart_density(charts, width: int, height: int, padding: int = 2):
    """The largest density of 16 bisection steps at which pack_charts fits the charts into width x height: hi is the density at
    which the widest or tallest chart just fits (its side without padding and the texel that holds umin), then 16 halvings of
    [0, hi] keep the largest density that packs.  Returns (texels_per_unit, last_rejected: the smallest density tried that did not
    fit, or None).  Raises ValueError when nothing fits (an atlas smaller than the padding, or no chart with an extent)."""
    c = np.ascontiguousarray(charts, dtype=abi.UNWRAP_CHART_DTYPE).reshape(-1)
    du = float((c["umax"].astype(np.float64) - c["umin"]).max()) if len(c) else 0.0
    dv = float((c["vmax"].astype(np.float64) - c["vmin"]).max()) if len(c) else 0.0
    room_w, room_h = int(width) - 1 - 2 * int(padding), int(height) - 1 - 2 * int(padding)
    if room_w < 1 or room_h < 1 or max(du, dv) <= 0.0:
        raise ValueError("no density fits: the atlas is smaller than the padding, or no chart has an extent")
    hi = float(np.float32(min(room_w / du if du > 0 else np.inf, room_h / dv if dv > 0 else np.inf)))
    if pack_charts(c, width, height, hi, padding)[0] is not None:
        return hi, None
    lo, rejected = 0.0, hi
    for _ in range(16):
        mid = float(np.float32(0.5 * (lo + hi)))
        if mid > 0.0 and pack_charts(c, width, height, mid, padding)[0] is not None:
            lo = mid
        else:
            hi = rejected = mid
    if lo <= 0.0:
        raise ValueError("no density of the bisection fits the atlas")
    return lo, rejected
