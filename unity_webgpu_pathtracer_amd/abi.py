"""ctypes mirror of include/ptmi_plugin.h and include/ptmi_layouts.h.

These are the blittable structs that cross the drop-in boundary; the field order and
widths are checked against the C headers by tests/test_abi.py (sizeof via a compiled probe).
Reference for every field: see the comments in include/ptmi_plugin.h.
"""
import ctypes as C

import numpy as np

# ---------------------------------------------------------------------------------------
# numpy dtypes of the scene buffers (include/ptmi_layouts.h)
# ---------------------------------------------------------------------------------------
FLOAT4 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4")])

CWBVH_NODE = np.dtype([
    ("lo", "<f4", 3), ("ex", "u1"), ("ey", "u1"), ("ez", "u1"), ("imask", "u1"),
    ("childBaseIndex", "<u4"), ("triBaseIndex", "<u4"), ("meta", "u1", 8),
    ("qlox", "u1", 8), ("qloy", "u1", 8), ("qloz", "u1", 8),
    ("qhix", "u1", 8), ("qhiy", "u1", 8), ("qhiz", "u1", 8),
])
assert CWBVH_NODE.itemsize == 80

TRI_ATTR = np.dtype([
    ("normal0", "<f4", 3), ("pad0", "<f4"), ("normal1", "<f4", 3), ("pad1", "<f4"),
    ("normal2", "<f4", 3), ("pad2", "<f4"), ("tangent0", "<f4", 3), ("pad3", "<f4"),
    ("tangent1", "<f4", 3), ("pad4", "<f4"), ("tangent2", "<f4", 3), ("pad5", "<f4"),
    ("uv0", "<f4", 2), ("uv1", "<f4", 2), ("uv2", "<f4", 2), ("materialIndex", "<u4"), ("pad6", "<f4"),
])
assert TRI_ATTR.itemsize == 128

MATERIAL_FLOATS = 32   # BVHScene.cs kMaterialSize
LIGHT_FLOATS = 16      # PathTracer.cs LightStructSize

TLAS_NODE = np.dtype([
    ("lmin", "<f4", 3), ("left", "<u4"), ("lmax", "<f4", 3), ("right", "<u4"),
    ("rmin", "<f4", 3), ("triCount", "<u4"), ("rmax", "<f4", 3), ("firstTri", "<u4"),
])
assert TLAS_NODE.itemsize == 64

GPU_INSTANCE = np.dtype([
    ("localToWorld", "<f4", 16), ("worldToLocal", "<f4", 16),
    ("bvhOffset", "<i4"), ("triOffset", "<i4"), ("triAttributeOffset", "<i4"), ("materialIndex", "<i4"),
])
assert GPU_INSTANCE.itemsize == 144

BLAS_INSTANCE = np.dtype([
    ("localToWorld", "<f4", 16), ("worldToLocal", "<f4", 16),
    ("aabbMin", "<f4", 3), ("blasIndex", "<u4"), ("aabbMax", "<f4", 3), ("mask", "<u4"),
    ("pad", "<u4", 8),
])
assert BLAS_INSTANCE.itemsize == 192

PT_FEATURE_HAS_LIGHTS = 0x1
PT_FEATURE_HAS_TEXTURES = 0x2
PT_FEATURE_HAS_TLAS = 0x4
PT_FEATURE_HAS_ENVIRONMENT_TEXTURE = 0x8

PT_OK = 0
PT_ERR_INVALID_ARG = -1
PT_ERR_NO_DEVICE = -2
PT_ERR_HIP = -3
PT_ERR_NO_SCENE = -4
PT_ERR_UNSUPPORTED = -5


class _Sized(C.Structure):
    """PTSceneDesc / PTFrameParams start with structSize = sizeof(struct) (include/ptmi_plugin.h, "Versioning")."""
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.structSize = C.sizeof(type(self))


class PTSceneDesc(_Sized):
    _fields_ = [
        ("structSize", C.c_uint32), ("_pad3", C.c_uint32),
        ("bvhNodes", C.c_void_p), ("bvhNodesBytes", C.c_uint64),
        ("bvhTris", C.c_void_p), ("bvhTrisBytes", C.c_uint64),
        ("triAttrs", C.c_void_p), ("triAttrsBytes", C.c_uint64),
        ("materials", C.c_void_p), ("materialCount", C.c_uint32), ("_pad0", C.c_uint32),
        ("lights", C.c_void_p), ("lightCount", C.c_uint32), ("_pad1", C.c_uint32),
        ("textureData", C.c_void_p), ("textureDataUints", C.c_uint64),
        ("features", C.c_uint32), ("_pad2", C.c_uint32),
        ("tlasData", C.c_void_p), ("tlasDataFloats", C.c_uint64),
        ("tlasIndexOffset", C.c_uint32), ("instanceCount", C.c_uint32),
        ("gpuInstances", C.c_void_p),
        ("envTexture", C.c_void_p), ("envWidth", C.c_uint32), ("envHeight", C.c_uint32),
    ]


class PTFrameParams(_Sized):
    _fields_ = [
        ("structSize", C.c_uint32), ("_pad0", C.c_uint32),
        ("CamInvProj", C.c_float * 16),
        ("CamToWorld", C.c_float * 16),
        ("RngSeedRoot", C.c_uint32),
        ("MaxRayBounces", C.c_uint32),
        ("SamplesPerPass", C.c_int32),
        ("OutputWidth", C.c_uint32),
        ("OutputHeight", C.c_uint32),
        ("CurrentSample", C.c_uint32),
        ("EnvironmentMode", C.c_int32),
        ("EnvironmentIntensity", C.c_float),
        ("EnvironmentColor", C.c_float * 4),
        ("EnvironmentMapRotation", C.c_float),
        ("FocalLength", C.c_float),
        ("Aperture", C.c_float),
        ("UseFireflyFilter", C.c_int32),
        ("MaxFireflyLuminance", C.c_float),
        ("UseRussianRoulette", C.c_int32),
        ("DispatchGroupsX", C.c_uint32),
        ("DispatchGroupsY", C.c_uint32),
    ]

    def copy(self):
        other = PTFrameParams()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(PTFrameParams))
        return other


class PTStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "paths", "closestHitRays", "shadowRays", "nodeVisits", "triTests", "attrFetches",
        "materialFetches", "lightFetches", "texelFetches", "texDescriptorFetches",
        "pixelsWritten", "pixelsRead", "maxStackDepth", "stackOverflows", "tlasNodeVisits", "instanceVisits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}

    @property
    def rays(self):
        return int(self.closestHitRays + self.shadowRays)

    def algorithmic_bytes(self):
        """bytes the reference kernel reads/writes for this work."""
        return int(80 * self.nodeVisits + 48 * self.triTests + 128 * self.attrFetches
                   + 128 * self.materialFetches + 64 * self.lightFetches + 4 * self.texelFetches
                   + 16 * self.texDescriptorFetches + 16 * (self.pixelsWritten + self.pixelsRead)
                   + 64 * self.tlasNodeVisits + 144 * self.instanceVisits)


class PTRepackStats(C.Structure):
    """PTGetRepackStats: the mid-pass slot repack of the default schedule, counted on the device since the context was created"""
    _fields_ = [(n, C.c_uint64) for n in ("sequences", "candidates", "repacks", "slotsMoved")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PTPresentParams(C.Structure):
    """Presentation.shader uniforms (PathTracer.cs:255-264); defaults = the inspector defaults (PathTracer.cs:41-48)."""
    _fields_ = [("OutputWidth", C.c_uint32), ("OutputHeight", C.c_uint32), ("Mode", C.c_int32), ("sRGB", C.c_int32),
                ("Exposure", C.c_float), ("Brightness", C.c_float), ("Contrast", C.c_float), ("Saturation", C.c_float),
                ("Vignette", C.c_float)]


TONEMAP_NONE, TONEMAP_ACES, TONEMAP_FILMIC, TONEMAP_REINHARD, TONEMAP_LOTTES = range(5)      # PathTracer.cs:8-14


PT_MESH_HAS_32_BIT_INDICES, PT_MESH_HAS_NORMALS, PT_MESH_HAS_TANGENTS, PT_MESH_HAS_UVS = 0x1, 0x2, 0x4, 0x8


class PTMeshDesc(C.Structure):
    """One Dispatch of MeshProcessing.compute (BVHScene.cs:489-553)."""
    _fields_ = [("vertexBuffer", C.c_void_p), ("vertexBufferBytes", C.c_uint64),
                ("indexBuffer", C.c_void_p), ("indexBufferBytes", C.c_uint64),
                ("VertexStride", C.c_uint32), ("PositionOffset", C.c_uint32), ("NormalOffset", C.c_uint32),
                ("TangentOffset", C.c_uint32), ("UVOffset", C.c_uint32), ("MaterialIndex", C.c_uint32),
                ("TriangleCount", C.c_uint32), ("OutputTriangleStart", C.c_uint32),
                ("LocalToWorld", C.c_float * 16), ("WorldToLocal", C.c_float * 16),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class PTTextureDesc(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("hasAlpha", C.c_int32), ("_pad", C.c_uint32)]


class PTTimings(C.Structure):
    _fields_ = [("passes", C.c_uint64), ("kernelMsTotal", C.c_double),
                ("kernelMsLast", C.c_double), ("kernelLaunches", C.c_uint64)]


# ---------------------------------------------------------------------------------------
# Part 3: ray queries (PTTraceRays / PTTraceRaysHost)
# ---------------------------------------------------------------------------------------
PT_FAR_PLANE = 100000.0            # include/ptmi_layouts.h
PT_QUERY_CLOSEST = 0
PT_QUERY_ANY_HIT = 1
PT_QUERY_SURFACE = 2
PT_MISS = 0xFFFFFFFF               # PTRayHit.prim / PTRaySurface.instance "none"


class PTRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("tmax", C.c_float), ("reserved", C.c_uint32)]


class PTRayHit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim", C.c_uint32)]


class PTRaySurface(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("t", C.c_float), ("normal", C.c_float * 3), ("materialIndex", C.c_int32),
                ("uv", C.c_float * 2), ("instance", C.c_uint32), ("prim", C.c_uint32)]


assert C.sizeof(PTRay) == 32 and C.sizeof(PTRayHit) == 16 and C.sizeof(PTRaySurface) == 48


# ---------------------------------------------------------------------------------------
# Part 4: guide buffers and denoising (PTRenderGuides / PTDenoise)
# ---------------------------------------------------------------------------------------
PT_DENOISE_DEMODULATE_ALBEDO = 0x1


class PTDenoiseParams(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("iterations", C.c_int32), ("sigmaLuminance", C.c_float),
                ("sigmaNormal", C.c_float), ("sigmaDepth", C.c_float), ("flags", C.c_uint32)]


assert C.sizeof(PTDenoiseParams) == 24


def denoise_params(iterations: int = 5, sigma_luminance: float = 4.0, sigma_normal: float = 128.0, sigma_depth: float = 1.0,
                   demodulate: bool = True) -> PTDenoiseParams:
    """PTDenoiseParams with the header's suggested values (5 levels, sigmas 4 / 128 / 1, albedo demodulation on)."""
    return PTDenoiseParams(C.sizeof(PTDenoiseParams), iterations, sigma_luminance, sigma_normal, sigma_depth,
                           PT_DENOISE_DEMODULATE_ALBEDO if demodulate else 0)


# ---------------------------------------------------------------------------------------
# Part 6: per-pixel variance across passes (PTAccumulateMoments / PTMeasureNoise / PTDenoiseMoments)
# ---------------------------------------------------------------------------------------
class PTNoiseParams(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("relFloor", C.c_float), ("threshold", C.c_float), ("percentile", C.c_float)]


class PTNoiseStats(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("observations", C.c_uint32), ("samples", C.c_uint64), ("pixels", C.c_uint64),
                ("pixelsBelow", C.c_uint64), ("meanError", C.c_float), ("maxError", C.c_float), ("percentileError", C.c_float),
                ("_pad", C.c_uint32), ("histogram", C.c_uint32 * 256)]


assert C.sizeof(PTNoiseParams) == 16 and C.sizeof(PTNoiseStats) == 1072


def noise_params(rel_floor: float = 0.01, threshold: float = 0.02, percentile: float = 0.95) -> PTNoiseParams:
    """PTNoiseParams with the header's suggested values (floor 0.01, threshold 2 %, 95th percentile)."""
    return PTNoiseParams(C.sizeof(PTNoiseParams), rel_floor, threshold, percentile)


def noise_stats() -> PTNoiseStats:
    """An empty PTNoiseStats with structSize set, for PTMeasureNoise to fill."""
    st = PTNoiseStats()
    st.structSize = C.sizeof(PTNoiseStats)
    return st


# ---------------------------------------------------------------------------------------
# Part 7: adaptive sampling (PTAdaptiveBegin / PTSetActiveBlocks / PTRenderPassActive)
# ---------------------------------------------------------------------------------------
class PTAdaptiveSelect(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("threshold", C.c_float), ("maxSamples", C.c_uint32), ("addSamples", C.c_uint32),
                ("dilate", C.c_uint32)]


assert C.sizeof(PTAdaptiveSelect) == 20


def adaptive_select(threshold: float, max_samples: int, add_samples: int, dilate: bool = True) -> PTAdaptiveSelect:
    return PTAdaptiveSelect(C.sizeof(PTAdaptiveSelect), threshold, max_samples, add_samples, 1 if dilate else 0)


# ---- radiance queries (include/ptmi_plugin.h Part 8)
class PTRadianceRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("rng", C.c_uint32), ("reserved", C.c_uint32)]


class PTRadiance(C.Structure):
    _fields_ = [("rgb", C.c_float * 3), ("rng", C.c_uint32)]


assert C.sizeof(PTRadianceRay) == 32 and C.sizeof(PTRadiance) == 16


# ---- irradiance gathers (include/ptmi_plugin.h Part 13)
PT_GATHER_MAX_SAMPLES = 65536


class PTReceiver(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("seed", C.c_uint32), ("normal", C.c_float * 3), ("reserved", C.c_uint32)]


class PTIrradiance(C.Structure):
    _fields_ = [("rgb", C.c_float * 3), ("m2", C.c_float)]


assert C.sizeof(PTReceiver) == 32 and C.sizeof(PTIrradiance) == 16


# ---- SH light probes (include/ptmi_plugin.h Part 15)
PT_PROBE_DELTA_LIGHTS = 1


class PTProbe(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("seed", C.c_uint32)]


class PTProbeCoeffs(C.Structure):
    _fields_ = [("sh", (C.c_float * 3) * 9), ("m2", C.c_float)]


class PTProbeQuery(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("probe", C.c_uint32)]


assert C.sizeof(PTProbe) == 16 and C.sizeof(PTProbeCoeffs) == 112 and C.sizeof(PTProbeQuery) == 16


# ---- probe volumes (include/ptmi_plugin.h Part 16)
PT_GRID_WRAP = 1
PT_GRID_VISIBILITY = 2
PT_GRID_MAX_AXIS = 1024


class PTProbeDepthMap(C.Structure):
    _fields_ = [("moments", (C.c_float * 2) * 64)]


class PTProbeGrid(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("flags", C.c_uint32), ("spacing", C.c_float * 3), ("normalBias", C.c_float),
                ("counts", C.c_uint32 * 3), ("reserved", C.c_uint32)]


assert C.sizeof(PTProbeDepthMap) == 512 and C.sizeof(PTProbeGrid) == 48


# ---- probe placement (include/ptmi_plugin.h Part 18)
PT_PROBE_INSIDE = 1
PT_PLACE_KEEP_OFFSETS = 1
PT_PLACE_MAX_ITERATIONS = 16


class PTProbePlacement(C.Structure):
    _fields_ = [("offset", C.c_float * 3), ("state", C.c_uint32)]


class PTProbePlaceParams(C.Structure):
    _fields_ = [("spacing", C.c_float * 3), ("maxDistance", C.c_float), ("minFrontDistance", C.c_float), ("backfaceShare", C.c_float),
                ("maxOffset", C.c_float), ("iterations", C.c_uint32)]


class PTProbePlaceStats(C.Structure):
    _fields_ = [("back", C.c_uint32), ("front", C.c_uint32), ("nearestBack", C.c_uint32), ("nearestFront", C.c_uint32),
                ("farthestFront", C.c_uint32), ("tNearestBack", C.c_float), ("tNearestFront", C.c_float), ("tFarthestFront", C.c_float)]


assert C.sizeof(PTProbePlacement) == 16 and C.sizeof(PTProbePlaceParams) == 32 and C.sizeof(PTProbePlaceStats) == 32
# one PTProbePlaceStats row as a numpy record
PLACE_STATS_DTYPE = [("back", "<u4"), ("front", "<u4"), ("nearestBack", "<u4"), ("nearestFront", "<u4"), ("farthestFront", "<u4"),
                     ("tNearestBack", "<f4"), ("tNearestFront", "<f4"), ("tFarthestFront", "<f4")]


def probe_place_params(spacing, max_distance: float = None, min_front_distance: float = None, backface_share: float = 0.25,
                       max_offset: float = 0.45, iterations: int = 4) -> PTProbePlaceParams:
    """PTProbePlaceParams for a grid of `spacing` (one number or three).  max_distance: default the spacing's diagonal;
    min_front_distance: default 0.2 of the smallest spacing."""
    s = [float(x) for x in (np.broadcast_to(np.asarray(spacing, np.float64), (3,)))]
    p = PTProbePlaceParams()
    for a in range(3):
        p.spacing[a] = s[a]
    p.maxDistance = float(np.linalg.norm(s)) if max_distance is None else float(max_distance)
    p.minFrontDistance = 0.2 * min(s) if min_front_distance is None else float(min_front_distance)
    p.backfaceShare, p.maxOffset, p.iterations = float(backface_share), float(max_offset), int(iterations)
    return p


# ---- reflection probes (include/ptmi_plugin.h Part 20)
PT_REFLECTION_MIN_RES = 8
PT_REFLECTION_MAX_RES = 256


class PTReflectionTexel(C.Structure):
    _fields_ = [("rgb", C.c_float * 3), ("aux", C.c_float)]


class PTReflectionQuery(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("roughness", C.c_float), ("direction", C.c_float * 3), ("probe", C.c_uint32)]


class PTReflectionBox(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("pad0", C.c_float), ("bmax", C.c_float * 3), ("pad1", C.c_float)]


assert C.sizeof(PTReflectionTexel) == 16 and C.sizeof(PTReflectionQuery) == 32 and C.sizeof(PTReflectionBox) == 32


# ---- shading from the bakes (include/ptmi_plugin.h Part 21)
PT_SHADE_MISS = 1
PT_SHADE_DFG_RES = (16, 32, 64)


class PTShadeInputs(C.Structure):
    _fields_ = [("grid", PTProbeGrid), ("dSH", C.c_void_p), ("dDepth", C.c_void_p), ("dPlacement", C.c_void_p), ("dMaps", C.c_void_p),
                ("dProbes", C.c_void_p), ("dBoxes", C.c_void_p), ("dDFG", C.c_void_p), ("probeCount", C.c_uint32), ("res", C.c_uint32),
                ("levels", C.c_uint32), ("dfgRes", C.c_uint32)]


assert C.sizeof(PTShadeInputs) == 120


# ---- first hits shaded from baked lightmaps (include/ptmi_plugin.h Part 22)
PT_LIGHTMAP_TWO_SIDED = 1
PT_LIGHTMAP_MAX_BINDINGS = 64
PT_LIGHTMAP_NONE = 0xFFFFFFFF


class PTLightmapBinding(C.Structure):
    _fields_ = [("firstPrim", C.c_uint32), ("primCount", C.c_uint32), ("instance", C.c_uint32), ("flags", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("reserved", C.c_uint32 * 2), ("dImage", C.c_void_p), ("dUvs", C.c_void_p)]


assert C.sizeof(PTLightmapBinding) == 48


# ---- direct light at first hits (include/ptmi_plugin.h Part 24)
PT_DIRECT_CENTERED = 1
PT_DIRECT_MAX_STRATA = 4


class PTDirectParams(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("strata", C.c_uint32), ("seed", C.c_uint32), ("flags", C.c_uint32), ("minAlpha", C.c_float),
                ("reserved", C.c_uint32 * 3)]


assert C.sizeof(PTDirectParams) == 32


def direct_params(strata: int = 1, seed: int = 0, centered: bool = False, min_alpha: float = 0.0) -> PTDirectParams:
    """A PTDirectParams with structSize set"""
    p = PTDirectParams()
    p.structSize = C.sizeof(PTDirectParams)
    p.strata, p.seed, p.flags, p.minAlpha = int(strata), int(seed) & 0xFFFFFFFF, PT_DIRECT_CENTERED if centered else 0, float(min_alpha)
    return p


# ---- direct light over many lights: the light grid (include/ptmi_plugin.h Part 25)
PT_LIGHT_GRID_MAX_DIM = 256
PT_LIGHT_GRID_MAX_CELLS = 1 << 20


class PTLightGridParams(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("origin", C.c_float * 3), ("cellSize", C.c_float), ("dims", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class PTLightGridStats(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("built", C.c_uint32), ("cells", C.c_uint32), ("lightCount", C.c_uint32), ("longest", C.c_uint32),
                ("stale", C.c_uint32), ("entries", C.c_uint64), ("generation", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "structSize"}


assert C.sizeof(PTLightGridParams) == 36 and C.sizeof(PTLightGridStats) == 40


def light_grid_params(origin, cell_size: float, dims) -> PTLightGridParams:
    """A PTLightGridParams with structSize set: dims[0] x dims[1] x dims[2] cubes of cell_size from origin"""
    p = PTLightGridParams()
    p.structSize = C.sizeof(PTLightGridParams)
    p.origin[:] = [float(x) for x in origin]
    p.cellSize = float(cell_size)
    p.dims[:] = [int(d) for d in dims]
    return p


# ---- lightmap charts (include/ptmi_plugin.h Part 14)
PT_CHART_MAX_SIZE = 8192
PT_CHART_MAX_DILATE = 16


class PTChartDesc(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("bvhOffset", C.c_int32), ("triOffset", C.c_int32), ("triAttributeOffset", C.c_int32),
                ("triangleCount", C.c_int32), ("instance", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("seedBase", C.c_uint32), ("reserved", C.c_uint32 * 3)]


assert C.sizeof(PTChartDesc) == 48


def chart_desc(width: int, height: int, triangle_count: int, offsets=(0, 0, 0), instance: int = -1, seed: int = 0) -> PTChartDesc:
    """A PTChartDesc with structSize set: the BLAS by its three offsets, the atlas size, the instance (-1: identity), seedBase."""
    d = PTChartDesc()
    d.structSize = C.sizeof(PTChartDesc)
    d.bvhOffset, d.triOffset, d.triAttributeOffset = (int(o) for o in offsets)
    d.triangleCount, d.instance = int(triangle_count), int(instance)
    d.width, d.height, d.seedBase = int(width), int(height), int(seed) & 0xFFFFFFFF
    return d


# ---- lightmap UVs (include/ptmi_plugin.h Part 23)
PT_UNWRAP_NO_CHART = 0xFFFFFFFF
PT_UNWRAP_MAX_PADDING = 16
PT_UNWRAP_MAX_SWEEPS = 64


class PTUnwrapDesc(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("bvhOffset", C.c_int32), ("triOffset", C.c_int32), ("triAttributeOffset", C.c_int32),
                ("triangleCount", C.c_int32), ("reserved", C.c_uint32 * 7)]


class PTUnwrapChart(C.Structure):
    _fields_ = [("firstPrim", C.c_uint32), ("cls", C.c_uint32), ("triCount", C.c_uint32), ("reserved", C.c_uint32),
                ("umin", C.c_float), ("vmin", C.c_float), ("umax", C.c_float), ("vmax", C.c_float)]


class PTUnwrapStats(C.Structure):
    _fields_ = [("excluded", C.c_uint32), ("linkedEdges", C.c_uint32), ("singleCharts", C.c_uint32), ("sweeps", C.c_uint32)]

    def as_dict(self):
        return {"excluded": self.excluded, "linked_edges": self.linkedEdges, "single_charts": self.singleCharts, "sweeps": self.sweeps}


UNWRAP_CHART_DTYPE = [("firstPrim", "<u4"), ("cls", "<u4"), ("triCount", "<u4"), ("reserved", "<u4"), ("umin", "<f4"), ("vmin", "<f4"), ("umax", "<f4"),
                      ("vmax", "<f4")]
assert C.sizeof(PTUnwrapDesc) == 48 and C.sizeof(PTUnwrapChart) == 32 and C.sizeof(PTUnwrapStats) == 16


def unwrap_desc(triangle_count: int, offsets=(0, 0, 0)) -> PTUnwrapDesc:
    """A PTUnwrapDesc with structSize set: the BLAS by its three offsets and its triangle count."""
    d = PTUnwrapDesc()
    d.structSize = C.sizeof(PTUnwrapDesc)
    d.bvhOffset, d.triOffset, d.triAttributeOffset = (int(o) for o in offsets)
    d.triangleCount = int(triangle_count)
    return d


# ---- the lightmap denoiser (include/ptmi_plugin.h Part 17)
PT_LMFILTER_MAX_ITERATIONS = 8
PT_LMFILTER_MAX_NORMAL_POWER = 7
PT_LMFILTER_MAX_SAMPLES = 1 << 24


class PTLightmapDenoiseParams(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("samples", C.c_uint32), ("iterations", C.c_uint32), ("normalPower", C.c_uint32),
                ("sigmaLuminance", C.c_float), ("sigmaPosition", C.c_float), ("sigmaPlane", C.c_float), ("reserved", C.c_uint32 * 5)]


assert C.sizeof(PTLightmapDenoiseParams) == 48


def lightmap_denoise_params(samples: int, iterations: int = 5, sigma_luminance: float = 4.0, sigma_position: float = 4.0, sigma_plane: float = 1.0,
                            normal_power: int = 5) -> PTLightmapDenoiseParams:
    """A PTLightmapDenoiseParams with structSize set and the header's suggested values; samples: the total behind m2."""
    p = PTLightmapDenoiseParams()
    p.structSize = C.sizeof(PTLightmapDenoiseParams)
    p.samples, p.iterations, p.normalPower = int(samples), int(iterations), int(normal_power)
    p.sigmaLuminance, p.sigmaPosition, p.sigmaPlane = float(sigma_luminance), float(sigma_position), float(sigma_plane)
    return p


# ---- adaptive gathers (include/ptmi_plugin.h Part 19)
PT_ADAPTIVE_GATHER_MAX_TOTAL = 1 << 24
PT_ADAPTIVE_GATHER_MAX_ENTRIES = 1 << 31


class PTAdaptiveGather(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("firstSample", C.c_uint32), ("minSamples", C.c_uint32), ("addSamples", C.c_uint32),
                ("maxSamples", C.c_uint32), ("threshold", C.c_float), ("darkFloor", C.c_float), ("reserved", C.c_uint32 * 5)]


class PTAdaptiveGatherStats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("maxCount", C.c_uint32), ("samples", C.c_uint64), ("stoppedThreshold", C.c_uint64),
                ("stoppedMaxSamples", C.c_uint64), ("stoppedNonFinite", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


assert C.sizeof(PTAdaptiveGather) == 48 and C.sizeof(PTAdaptiveGatherStats) == 40


def adaptive_gather(threshold: float, min_samples: int = 16, add_samples: int = 16, max_samples: int = 1024, dark_floor: float = 0.0,
                    first_sample: int = 0) -> PTAdaptiveGather:
    """A PTAdaptiveGather with structSize set: the relative standard error of the mean luminance to reach, the samples of round 0,
    of every later round and at most, the luminance below which the error is measured against dark_floor, the first sample index."""
    a = PTAdaptiveGather()
    a.structSize = C.sizeof(PTAdaptiveGather)
    a.firstSample = int(first_sample) & 0xFFFFFFFF
    a.minSamples, a.addSamples, a.maxSamples = int(min_samples), int(add_samples), int(max_samples)
    a.threshold, a.darkFloor = float(threshold), float(dark_floor)
    return a


# ---------------------------------------------------------------------------------------
# Part 10: geometry rebuilds and tree quality (PTRebuildGeometry / PTMeasureGeometry / PTMeasureBVHArrays)
# ---------------------------------------------------------------------------------------
class PTGeometryQuality(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("nodeCapacity", C.c_uint32), ("nodeCount", C.c_uint32), ("triangleCount", C.c_uint32),
                ("levels", C.c_uint32), ("reserved", C.c_uint32), ("rootHalfArea", C.c_double), ("sahCost", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k in ("nodeCapacity", "nodeCount", "triangleCount", "levels", "rootHalfArea", "sahCost")}


assert C.sizeof(PTGeometryQuality) == 40


def geometry_quality() -> PTGeometryQuality:
    """An empty PTGeometryQuality with structSize set, for PTMeasureGeometry / PTMeasureBVHArrays to fill."""
    q = PTGeometryQuality()
    q.structSize = C.sizeof(PTGeometryQuality)
    return q


# ---------------------------------------------------------------------------------------
# Part 11: skinned geometry (PTSetSkin / PTSkinGeometry / PTSkinVerticesHost)
# ---------------------------------------------------------------------------------------
PT_SKIN_MAX_JOINTS = 1024
PT_SKIN_REBUILD = 0x1


class PTSkinDesc(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("jointCount", C.c_uint32), ("restVertices", C.c_void_p), ("joints", C.c_void_p),
                ("weights", C.c_void_p), ("restAttrs", C.c_void_p)]


assert C.sizeof(PTSkinDesc) == 40


def skin_desc() -> PTSkinDesc:
    """An empty PTSkinDesc with structSize set."""
    d = PTSkinDesc()
    d.structSize = C.sizeof(PTSkinDesc)
    return d


# ---------------------------------------------------------------------------------------
# Part 12: morph targets (PTSetMorph / PTMorphGeometry / PTMorphVerticesHost)
# ---------------------------------------------------------------------------------------
PT_MORPH_MAX_TARGETS = 1024
MORPH_ENTRY = np.dtype([("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("target", "<u4")])
assert MORPH_ENTRY.itemsize == 16


class PTMorphEntry(C.Structure):
    _fields_ = [("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float), ("target", C.c_uint32)]


class PTMorphDesc(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("targetCount", C.c_uint32), ("restVertices", C.c_void_p), ("restAttrs", C.c_void_p),
                ("positionOffsets", C.c_void_p), ("positionEntries", C.c_void_p), ("normalOffsets", C.c_void_p), ("normalEntries", C.c_void_p),
                ("tangentOffsets", C.c_void_p), ("tangentEntries", C.c_void_p)]


assert C.sizeof(PTMorphDesc) == 72 and C.sizeof(PTMorphEntry) == 16


def morph_desc() -> PTMorphDesc:
    """An empty PTMorphDesc with structSize set."""
    d = PTMorphDesc()
    d.structSize = C.sizeof(PTMorphDesc)
    return d


def as_void_p(arr):
    """Borrowed host pointer of a C-contiguous numpy array (None -> NULL)."""
    if arr is None:
        return None
    assert arr.flags["C_CONTIGUOUS"]
    return arr.ctypes.data_as(C.c_void_p)
