"""Radiance queries (PTCameraRays / PTTraceRadiance / PTTraceRadianceHost, include/ptmi_plugin.h Part 8) on the MI355X.

The contract is bit-exact and the tests hold it without tolerances: the camera's rays traced as a list give the frame of
PTRenderPassTo and of the oracle; a list's results do not depend on its order, its length or on what else is in flight; n samples
in one call are n calls of one sample chained through the returned RNG state."""
import ctypes as C

import numpy as np
import pytest

from unity_webgpu_pathtracer_amd import abi, plugin, scenes
from unity_webgpu_pathtracer_amd.pathtracer import PathTracer

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 40, 24, 3                   # 960 rays = 3.75 workgroups of 256; partial 16x16 blocks both ways
N = W * H
SCENES = {"cornell_box": scenes.cornell_box, "material_zoo": scenes.material_zoo, "instanced_scene": scenes.instanced_scene}
SEED = 0x5AD1A
_oracle_frames = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tracer(name, schedule=1, spp=1):
    return PathTracer(SCENES[name](), width=W, height=H, samplesPerPass=spp, maxRayBounces=BOUNCES, schedule=schedule)


def _params(pt, seed=SEED, lens=False):
    p = pt.params(seed=seed)
    if lens:
        p.Aperture, p.FocalLength = 0.1, 3.0
    return p


def _frame(pt, p):
    """PTRenderPassTo into a caller's device frame -> (H, W, 4) numpy"""
    import torch
    out = torch.empty((H, W, 4), dtype=torch.float32, device=f"cuda:{pt.device}")
    torch.cuda.synchronize()
    pt.render_pass_to(p, out.data_ptr())
    pt.synchronize()
    return out.cpu().numpy()


def _oracle_frame(oracle, pt, name, p, lens):
    """the oracle's frame of (scene, lens): computed once, shared by the schedules (the CPU-built BVH is the same every time)"""
    key = (name, lens)
    if key not in _oracle_frames:
        _oracle_frames[key] = oracle.render(oracle.buffers_from_bvhscene(pt._bvhScene), p)[0]
    return _oracle_frames[key]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. camera rays + radiance == PTRenderPassTo == the oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
CASES = [(n, s, False) for n in SCENES for s in (1, 2, 3)] + [("material_zoo", 1, True)]


@pytest.mark.parametrize("name,schedule,lens", CASES)
def test_camera_rays_then_radiance_is_the_frame(oracle, name, schedule, lens):
    pt = _tracer(name, schedule)
    try:
        p = _params(pt, lens=lens)
        rays = pt.camera_rays(params=p)
        assert rays.shape == (N, 8) and rays.dtype == np.float32
        assert (_bits(rays[:, 7]) == 0).all()
        got = pt.radiance(rays, spp=1, params=p)
        assert got.shape == (N, 4)
        frame = _frame(pt, p)
        ref = _oracle_frame(oracle, pt, name, p, lens)
        rgb = got[:, :3].reshape(H, W, 3)
        bad_frame = int((_bits(rgb) != _bits(frame[..., :3])).any(axis=-1).sum())
        bad_oracle = int((_bits(rgb) != _bits(ref[..., :3])).any(axis=-1).sum())
        print(f"[radiance] {name} schedule {schedule} lens {lens}: {bad_frame} pixels differ from PTRenderPassTo, {bad_oracle} from the oracle")
        assert bad_frame == 0 and bad_oracle == 0
        if lens:                                        # four camera draws: the origins differ between pixels
            assert len({tuple(r) for r in _bits(rays[:, :3]).tolist()}) > 1
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. seeds
# ---------------------------------------------------------------------------------------------------------------------------
def test_camera_rays_seeds_and_pixel_lists(oracle):
    import torch
    lib = oracle.load_oracle()

    def after_two_draws(seed):
        s = C.c_uint32(seed & 0xFFFFFFFF)
        lib.oracle_random_float(C.byref(s))
        lib.oracle_random_float(C.byref(s))
        return s.value

    pt = _tracer("cornell_box")
    try:
        S = 0xC0FFEE01
        rays = pt.camera_rays(current_sample=5, seed=S)
        rng = _bits(rays[:, 6])
        for k in (0, 1, 17, W, N // 2 + 3, N - 1):
            assert int(rng[k]) == after_two_draws(k * 6 + S), k
        assert np.allclose(np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1), 1.0, atol=1e-6)
        dev = f"cuda:{pt.device}"
        idx = torch.tensor([0, N - 1, 17, 17, N], dtype=torch.int32, device=dev)      # the last one is outside the frame
        sub = pt.camera_rays(pixels=idx, current_sample=5, seed=S)
        assert sub.is_cuda and sub.shape == (5, 8)
        sub = sub.cpu().numpy()
        assert (_bits(sub[:4]) == _bits(rays[[0, N - 1, 17, 17]])).all()
        assert np.isnan(sub[4, 3:6]).all() and int(_bits(sub[4, 6:7])[0]) == 0
        # a numpy list takes the same path
        assert (_bits(pt.camera_rays(pixels=np.array([17, 0]), current_sample=5, seed=S)) == _bits(rays[[17, 0]])).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. order and padding
# ---------------------------------------------------------------------------------------------------------------------------
def test_order_and_padding():
    import torch
    pt = _tracer("material_zoo")
    try:
        p = _params(pt)
        rays = pt.camera_rays(params=p)
        full = pt.radiance(rays, params=p)
        perm = np.random.default_rng(7).permutation(N)
        assert (_bits(pt.radiance(rays[perm], params=p)) == _bits(full[perm])).all()
        for n in (1, 255, 256, 257, 960):
            assert (_bits(pt.radiance(rays[:n], params=p)) == _bits(full[:n])).all(), n
        # nothing past count is written
        dev = f"cuda:{pt.device}"
        d_rays = torch.from_numpy(rays).to(dev)
        out = torch.full((N, 4), -123.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        q = pt._radiance_params(p, spp=1)
        plugin.check(pt.lib.PTTraceRadiance(pt.ctx, C.byref(q), d_rays.data_ptr(), 257, out.data_ptr()))
        pt.synchronize()
        out = out.cpu().numpy()
        assert (_bits(out[:257]) == _bits(full[:257])).all()
        assert (out[257:] == np.float32(-123.25)).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. samples chain through the returned RNG state; few iterations -> paths finish (and restart) in the cleanup kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 2])
@pytest.mark.parametrize("name", ["material_zoo", "instanced_scene"])
def test_samples_chain(name, iterations):
    pt = _tracer(name)
    try:
        pt.set_wavefront_iterations(iterations)
        p = _params(pt)
        rays = pt.camera_rays(params=p)
        three = pt.radiance(rays, spp=3, params=p)
        cur = rays.copy()
        parts = []
        for _ in range(3):
            r = pt.radiance(cur, spp=1, params=p)
            parts.append(r[:, :3].copy())
            cur[:, 6] = r[:, 3]
        mean = ((parts[0] + parts[1]) + parts[2]) / np.float32(3)
        assert mean.dtype == np.float32
        assert (_bits(three[:, :3]) == _bits(mean)).all()
        assert (_bits(three[:, 3]) == _bits(cur[:, 6])).all()
        assert (_bits(three[:, 3]) != _bits(rays[:, 6])).any()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. calls in flight
# ---------------------------------------------------------------------------------------------------------------------------
def test_calls_in_flight():
    import torch
    pt = _tracer("instanced_scene")
    try:
        p = _params(pt)
        dev = f"cuda:{pt.device}"
        rays = pt.camera_rays(params=p)
        rng = np.random.default_rng(11)
        lists = [torch.from_numpy(np.ascontiguousarray(rays[rng.permutation(N)[:n]])).to(dev) for n in (960, 300, 700, 129)]
        torch.cuda.synchronize()
        back_to_back = [pt.radiance(t, spp=2, params=p) for t in lists]
        pt.synchronize()
        back_to_back = [t.cpu().numpy() for t in back_to_back]
        for t, got in zip(lists, back_to_back):
            alone = pt.radiance(t, spp=2, params=p)
            pt.synchronize()
            assert (_bits(alone.cpu().numpy()) == _bits(got)).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. no side effects on the frames
# ---------------------------------------------------------------------------------------------------------------------------
def test_no_side_effects_on_passes():
    pt = _tracer("material_zoo", spp=2)
    try:
        rays = pt.camera_rays(seed=3)
        frames = []
        for between in (False, True):
            pt.Reset()
            pt.OnRenderImage(SEED)
            if between:
                pt.radiance(rays[:500], spp=2)
            pt.OnRenderImage(SEED + 1)
            frames.append(pt.readback())
        assert (_bits(frames[0]) == _bits(frames[1])).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. statistics
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [1, 2, 3])
def test_statistics(schedule):
    for name in ("material_zoo", "instanced_scene"):
        pt = _tracer(name, schedule)
        try:
            pt.set_stats_level(1)
            p = _params(pt)
            rays = pt.camera_rays(params=p)
            pt.reset_stats()
            _frame(pt, p)
            frame = pt.stats().as_dict()
            pt.reset_stats()
            pt.radiance(rays, spp=1, params=p)
            pt.synchronize()
            rad = pt.stats().as_dict()
            assert rad["paths"] == N and rad["pixelsWritten"] == 0 and rad["pixelsRead"] == 0
            assert frame["pixelsWritten"] == N
            for k in frame:
                if k not in ("pixelsWritten", "pixelsRead"):
                    assert rad[k] == frame[k], (name, k, rad[k], frame[k])
            assert rad["closestHitRays"] > N and rad["nodeVisits"] > 0
            # paths = count x spp, the pixel counters do not move
            pt.radiance(rays[:300], spp=3, params=p)
            pt.synchronize()
            st = pt.stats().as_dict()
            assert st["paths"] == N + 300 * 3 and st["pixelsWritten"] == 0 and st["pixelsRead"] == 0
        finally:
            pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the torch path
# ---------------------------------------------------------------------------------------------------------------------------
def test_torch_path():
    import torch
    pt = _tracer("material_zoo")
    try:
        p = _params(pt)
        dev = f"cuda:{pt.device}"
        rays = pt.camera_rays(params=p)
        host = pt.radiance(rays, spp=2, params=p)
        d_rays = torch.from_numpy(rays).to(dev)
        got = pt.radiance(d_rays, spp=2, params=p)
        assert got.is_cuda and got.shape == (N, 4) and got.dtype == torch.float32
        assert (_bits(got.cpu().numpy()) == _bits(host)).all()
        # rays made by a torch kernel enqueued right before the query, no host synchronisation in between
        made = d_rays.flip(0).contiguous()
        got = pt.radiance(made, spp=2, params=p)
        assert (_bits(got.cpu().numpy()) == _bits(host[::-1])).all()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(plugin.PluginError) as e:
        fn()
    return e.value.code, str(e.value)


def test_errors(oracle):
    import torch
    lib = plugin.load_library()
    pt = _tracer("material_zoo")
    try:
        p = _params(pt)
        rays = pt.camera_rays(params=p)[:64]
        for schedule in (0, 4):
            pt.set_schedule(schedule)
            code, msg = _code(lambda: pt.radiance(rays, params=p))
            assert code == abi.PT_ERR_UNSUPPORTED and f"schedule {schedule}" in msg, msg
        pt.set_schedule(1)
        assert pt.radiance(rays[:0], params=p).shape == (0, 4)                        # count == 0 -> PT_OK
        bad = rays.copy()
        bad[5, 7:8].view(np.uint32)[0] = 1
        code, msg = _code(lambda: pt.radiance(bad, params=p))
        assert code == abi.PT_ERR_INVALID_ARG and "rays[5].reserved" in msg, msg
        assert _code(lambda: pt.radiance(rays, spp=4096, params=p))[0] == abi.PT_ERR_UNSUPPORTED
        # PTCameraRays without a list: more entries than pixels
        buf = torch.empty((N + 1, 8), dtype=torch.float32, device=f"cuda:{pt.device}")
        rc = lib.PTCameraRays(pt.ctx, C.byref(p), None, N + 1, buf.data_ptr())
        assert rc == abi.PT_ERR_INVALID_ARG and str(N).encode() in lib.PTGetLastError()
        # a NaN ray: no walk, the sky -- what the oracle gives a pixel that sees nothing but sky with the same params
        q = _params(pt)
        q.CamToWorld[12], q.CamToWorld[13], q.CamToWorld[14] = 1.0e4, 2.0e4, 1.0e4           # the camera far outside the scene
        sky = oracle.render(oracle.buffers_from_bvhscene(pt._bvhScene), q, window=(0, 0, 1, 1))[0][0, 0, :3]
        nan = rays[:3].copy()
        nan[0, 0], nan[1, 4], nan[2, 3:6] = np.nan, np.nan, np.nan
        got = pt.radiance(nan, params=p)
        assert (_bits(got[:, :3]) == _bits(sky)[None, :]).all(), (got, sky)
        assert (_bits(got[:, 3]) == _bits(nan[:, 6])).all()                          # the sky draws nothing
    finally:
        pt.close()
    # before PTSetScene
    ctx = C.c_void_p()
    plugin.check(lib.PTCreate(0, C.byref(ctx)))
    try:
        out = np.empty((64, 4), np.float32)
        assert lib.PTTraceRadianceHost(ctx, C.byref(p), rays.ctypes.data, 64, out.ctypes.data) == abi.PT_ERR_NO_SCENE
    finally:
        lib.PTDestroy(ctx)
