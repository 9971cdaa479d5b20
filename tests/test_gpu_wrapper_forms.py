"""The two call forms of the Python host layer (unity_webgpu_pathtracer_amd/pathtracer.py) on the MI355X: every call that takes
numpy arrays or device tensors gives the same answer in the kind it was asked in.

One table row per call.  With list lengths 1 and 3 a row is called once with numpy inputs and once with the same data as tensors
on the context's device: numpy in gives numpy out, tensors in give tensors on that device, shapes and dtypes are the docstrings',
and the two results are equal bit for bit (uint32 views: NaN payloads and signed zeros count).  With list length 0 a row does what
its ZERO column records, per form: empty results of the shapes and dtypes its `outs` name, or a plugin.PluginError with a code.
That column was recorded from the wrapper as it stood before the forms were written once, and it is kept as recorded even where
it looks like an accident -- the numpy and the tensor form of one call disagreeing, for instance."""
import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer

pytestmark = pytest.mark.gpu

F = np.float32
W = H = 16
SPP = 2
RES = abi.PT_REFLECTION_MIN_RES
LEVELS = 2
TEXELS = plugin.reflection_texel_count(RES, LEVELS)
EMPTY = "empty"
INVALID = abi.PT_ERR_INVALID_ARG


class Baked:
    """the Cornell box at 16 x 16 with its bakes -- a 2 x 2 x 2 probe volume, two boxed reflection probes, a DFG table, one bound
    lightmap -- and three first hits of camera rays with everything the shading calls take, all as numpy"""

    def __init__(self):
        import torch
        self.pt = pt = PathTracer(scenes.cornell_box(), width=W, height=H, samplesPerPass=SPP, maxRayBounces=2, schedule=1)
        self.dev = torch.device(f"cuda:{pt.device}")
        rng = np.random.default_rng(7)
        self.volume = pt.bake_probe_volume((-0.8, 0.2, -0.8), (0.8, 1.8, 0.8), (2, 2, 2), spp=SPP, depth_spp=SPP)
        pos = np.array([[0.3, 1.2, 0.2], [-0.4, 0.7, -0.1]], F)
        self.reflections = pt.capture_reflection_probes(pos, res=RES, spp=SPP, levels=LEVELS, boxes=(pos - F(0.9), pos + F(0.9)))
        self.dfg = pt.bake_dfg(16).cpu().numpy()
        pt.bind_lightmaps([pt.lightmap_binding(rng.random((8, 8, 4), dtype=F) + F(0.5), two_sided=True)])
        self.points = np.array([[0.1, 0.9, 0.2], [-0.5, 0.4, 0.3], [0.6, 1.5, -0.4]], F)
        self.normals = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]], F)
        self.pixels = np.array([5, 100, 255], np.uint32)
        self.radiance_rays = pt.camera_rays(self.pixels, seed=3)
        self.rays = np.stack([pt.camera_ray(x, y) for x, y in ((4, 7), (8, 8), (11, 5))])
        self.hits, self.surf = pt.trace_rays(self.rays, surface=True)
        assert (self.hits[:, 3].view(np.uint32) != abi.PT_MISS).all()
        self.probe_rows = self.reflections.probe_rows.cpu().numpy()
        self.box_rows = self.reflections.box_rows.cpu().numpy()
        self.terms = pt.shade_surfaces(self.rays, self.hits, self.surf, self.probe_rows, self.box_rows)[1]
        self.sh = self.volume.sh.cpu().numpy()[:2]
        self.base = rng.random((3, RES * RES, 4), dtype=F)
        self.rgba = rng.random((3, 4), dtype=F)

    def close(self):
        self.pt.close()


@pytest.fixture(scope="module")
def baked():
    b = Baked()
    yield b
    b.close()


def _adaptive(b, pos, nrm):
    out, counts, stats = b.pt.irradiance_adaptive(pos, nrm, threshold=0.5, min_samples=2, add_samples=2, max_samples=4, dark_floor=0.01)
    return out, counts, stats


# name, the call over the first n entries of the fixture's lists (numpy arrays: the tensor form gets the same arrays as tensors),
# outs(n): (shape, numpy dtype, tensor dtype) of every array of the result, ZERO: (numpy form, tensor form) at n = 0
ROWS = [
    ("trace_rays", lambda b, n: (b.pt.trace_rays, b.rays[:n]),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, INVALID)),
    ("trace_rays[surface]", lambda b, n: (lambda r: b.pt.trace_rays(r, surface=True), b.rays[:n]),
     lambda n: [((n, 4), "float32", "float32"), ((n, 12), "float32", "float32")], (EMPTY, INVALID)),
    ("radiance", lambda b, n: (lambda r: b.pt.radiance(r, spp=SPP), b.radiance_rays[:n]),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, INVALID)),
    ("irradiance", lambda b, n: (lambda p, q: b.pt.irradiance(p, q, spp=SPP), b.points[:n], b.normals[:n]),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, INVALID)),
    ("irradiance[receivers]", lambda b, n: (lambda r: b.pt.irradiance(receivers=r, spp=SPP), b.pt._receivers(b.points[:n], b.normals[:n], None)),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, INVALID)),
    ("irradiance_adaptive", lambda b, n: (lambda p, q: _adaptive(b, p, q), b.points[:n], b.normals[:n]),
     lambda n: [((n, 4), "float32", "float32"), ((n,), "uint32", "int32")], (EMPTY, INVALID)),
    ("probe_sh", lambda b, n: (lambda p: b.pt.probe_sh(p, spp=SPP), b.points[:n]),
     lambda n: [((n, 9, 3), "float32", "float32"), ((n,), "float32", "float32")], (EMPTY, INVALID)),
    ("probe_depth", lambda b, n: (lambda p: b.pt.probe_depth(p, spp=SPP), b.points[:n]),
     lambda n: [((n, 64, 2), "float32", "float32")], (EMPTY, INVALID)),
    ("capture_reflection_base", lambda b, n: (lambda p: b.pt.capture_reflection_base(p, res=RES, spp=SPP), b.points[:n]),
     lambda n: [((n, RES * RES, 4), "float32", "float32")], (EMPTY, EMPTY)),
    ("place_probes", lambda b, n: (lambda p: b.pt.place_probes(p, 0.8, spp=SPP, iterations=1), b.points[:n]),
     lambda n: [((n, 3), "float32", "float32"), ((n,), "uint32", "int32")], (EMPTY, INVALID)),
    ("camera_rays", lambda b, n: (lambda k: b.pt.camera_rays(k, seed=3), b.pixels[:n]),
     lambda n: [((n, 8), "float32", "float32")], (INVALID, INVALID)),
    ("_sample_rays[gather_rays]", lambda b, n: (lambda p, q: b.pt.gather_rays(p, q, spp=SPP), b.points[:n], b.normals[:n]),
     lambda n: [((n * SPP, 8), "float32", "float32")], (INVALID, INVALID)),
    ("_sample_rays[probe_rays]", lambda b, n: (lambda p: b.pt.probe_rays(p, spp=SPP), b.points[:n]),
     lambda n: [((n * SPP, 8), "float32", "float32")], (INVALID, INVALID)),
    ("reflection_rays", lambda b, n: (lambda p: b.pt.reflection_rays(p, res=RES, spp=SPP), b.points[:n]),
     lambda n: [((n * RES * RES * SPP, 8), "float32", "float32")], (EMPTY, EMPTY)),
    ("probe_irradiance", lambda b, n: (lambda sh, q, k: b.pt.probe_irradiance(sh, q, k), b.sh, b.normals[:n], np.array([0, 1, 5], np.uint32)[:n]),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, EMPTY)),
    ("prefilter_reflection", lambda b, n: (lambda m: b.pt.prefilter_reflection(m, RES, LEVELS), b.base[:n]),
     lambda n: [((n, TEXELS, 4), "float32", "float32")], (EMPTY, EMPTY)),
    ("shade_surfaces", lambda b, n: (b.pt.shade_surfaces, b.rays[:n], b.hits[:n], b.surf[:n], b.probe_rows, b.box_rows),
     lambda n: [((n, c), "float32", "float32") for c in (12, 12, 8, 8)], (EMPTY, EMPTY)),
    ("shade_compose", lambda b, n: (b.pt.shade_compose, b.terms[:n], b.rgba[:n], b.rgba[::-1][:n].copy(), b.dfg),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, EMPTY)),
    ("shade_baked", lambda b, n: (lambda r, h, s, d: b.pt.shade_baked(r, h, s, b.volume, b.reflections, d), b.rays[:n], b.hits[:n], b.surf[:n], b.dfg),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, EMPTY)),
    ("lightmap_lookup", lambda b, n: (b.pt.lightmap_lookup, b.rays[:n], b.hits[:n], b.surf[:n]),
     lambda n: [((n, 4), "float32", "float32"), ((n,), "uint32", "int32")], (EMPTY, EMPTY)),
    ("shade_lightmapped", lambda b, n: (lambda r, h, s, d: b.pt.shade_lightmapped(r, h, s, b.volume, b.reflections, d), b.rays[:n], b.hits[:n], b.surf[:n], b.dfg),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, EMPTY)),
    ("ProbeVolume.irradiance", lambda b, n: (lambda p, q: b.volume.irradiance(p, q), b.points[:n], b.normals[:n]),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, EMPTY)),
    ("ProbeVolume.irradiance[receivers]", lambda b, n: (lambda r: b.volume.irradiance(receivers=r), plugin.receiver_rows(b.points[:n], b.normals[:n])),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, EMPTY)),
    ("ReflectionProbes.lookup", lambda b, n: (lambda d, k, p: b.reflections.lookup(d, 0.4, k, p), b.normals[:n], np.array([1, 0, 7], np.uint32)[:n], b.points[:n]),
     lambda n: [((n, 4), "float32", "float32")], (EMPTY, EMPTY)),
]
IDS = [r[0] for r in ROWS]


def _as_tensor(b, a):
    """the numpy array as a tensor on the context's device; uint32 travels as the int32 of the same bits"""
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(b.dev)


def _call(b, row, n, tensors):
    fn, *args = row[1](b, n)
    res = fn(*[_as_tensor(b, np.ascontiguousarray(a)) for a in args] if tensors else [np.ascontiguousarray(a) for a in args])
    return list(res) if isinstance(res, tuple) else [res]


def _check_kind(b, row, n, res, tensors):
    """the arrays of a result are of the kind asked for, with the shapes and dtypes of the row's outs(n)"""
    import torch
    arrays = [r for r in res if not isinstance(r, dict)]
    outs = row[2](n)
    assert len(arrays) == len(outs), (len(arrays), len(outs))
    for a, (shape, np_dtype, t_dtype) in zip(arrays, outs):
        if tensors:
            assert isinstance(a, torch.Tensor) and a.device == b.dev, (type(a), getattr(a, "device", None))
            assert tuple(a.shape) == shape and str(a.dtype) == "torch." + t_dtype, (tuple(a.shape), a.dtype, shape, t_dtype)
        else:
            assert isinstance(a, np.ndarray), type(a)
            assert a.shape == shape and a.dtype == np.dtype(np_dtype), (a.shape, a.dtype, shape, np_dtype)
    return arrays


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    assert a.dtype.itemsize == 4, a.dtype
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_forms_agree(baked, row, n):
    got_np, got_t = _call(baked, row, n, False), _call(baked, row, n, True)
    a_np, a_t = _check_kind(baked, row, n, got_np, False), _check_kind(baked, row, n, got_t, True)
    for x, y in zip(a_np, a_t):
        assert np.array_equal(_bits(x), _bits(y)), row[0]
    assert [r for r in got_np if isinstance(r, dict)] == [r for r in got_t if isinstance(r, dict)]


def observe_zero(b, row, tensors):
    """what a row does at list length 0: EMPTY (the arrays of outs(0), checked), or the PluginError's code"""
    try:
        res = _call(b, row, 0, tensors)
    except plugin.PluginError as e:
        return e.code
    _check_kind(b, row, 0, res, tensors)
    return EMPTY


@pytest.mark.parametrize("tensors", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_zero_length(baked, row, tensors):
    assert observe_zero(baked, row, tensors) == row[3][1 if tensors else 0]
