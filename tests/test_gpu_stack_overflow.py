"""The overflow rule of the two 32-entry traversal stacks (include/ptmi_plugin.h, Part 3) on the MI355X.

Inputs and expectations: tests/stack_cases.py (hand-written trees 40 levels and 48 instances deep whose answers follow from the rule
and the construction, and a chain made by BuildTLAS).  Ray queries must return those records bit for bit and count what the oracle
counts; every schedule must render the oracle's frame and counters; the guide, radiance and active-block entry points, which use
the same walks, must agree with the queries and the frames; a lane that overflows must not disturb its neighbours' slab rows.
The CPU side of the same cases is tests/test_stack_overflow.py; the small-stack build's is in tests/test_gpu_stress_variants.py."""
import numpy as np
import pytest

import stack_cases as sc
from unity_webgpu_pathtracer_amd import abi, plugin

pytestmark = pytest.mark.gpu

MISS = np.uint32(sc.MISS)
QUERY_COUNTERS = ["closestHitRays", "shadowRays", "nodeVisits", "triTests", "attrFetches", "maxStackDepth", "stackOverflows",
                  "tlasNodeVisits", "instanceVisits"]
ALL_COUNTERS = ["paths", "closestHitRays", "shadowRays", "nodeVisits", "triTests", "attrFetches", "materialFetches",
                "lightFetches", "texelFetches", "texDescriptorFetches", "pixelsWritten", "pixelsRead", "maxStackDepth",
                "stackOverflows", "tlasNodeVisits", "instanceVisits"]

QUERY_CASES = {
    "deep_cwbvh32": lambda: sc.deep_cwbvh(32),
    "deep_cwbvh33": lambda: sc.deep_cwbvh(33),
    "deep_cwbvh40": lambda: sc.deep_cwbvh(40),
    "deep_tlas48": lambda: sc.deep_tlas(48),
    "deep_blas_instances": lambda: sc.deep_blas_instances(40),
}
# name -> (case, width, height, samples per pass)
FRAME_CASES = {
    "deep_cwbvh40": (lambda: sc.deep_cwbvh(40), 48, 32, 2),
    "deep_blas_instances": (lambda: sc.deep_blas_instances(40), 48, 32, 2),
    "deep_tlas48": (lambda: sc.deep_tlas(48, floor=True), 48, 32, 2),
    "geometric_chain": (lambda: sc.Case("geometric_chain", sc.geometric_chain_scene()), 32, 24, 2),
}
SEED = 0x57AC4

_frames = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle_rays(oracle, rays, any_hit=False):
    r = np.array(rays, np.float32, copy=True)
    r[:, 7] = 1.0 if any_hit else 0.0
    return r.view(oracle.ORACLE_RAY_DTYPE).reshape(-1)


def _stats_equal(gpu, ref, fields, what):
    g, r = gpu.as_dict(), ref.as_dict()
    bad = {k: (g[k], r[k]) for k in fields if g[k] != r[k]}
    assert not bad, f"{what}: counter mismatch (gpu, oracle): {bad}"


def _query(pt, rays, **kw):
    pt.set_stats_level(1)
    pt.reset_stats()
    out = pt.trace_rays(rays, **kw)
    st = pt.stats()
    pt.set_stats_level(0)
    return out, st


def _oracle_frame(oracle, name):
    """the oracle's frame and counters of a frame case: computed once, shared by the schedules"""
    if name not in _frames:
        make, w, h, spp = FRAME_CASES[name]
        case = make()
        p = sc.scenes.frame_params(case.scene, w, h, spp=spp, seed=SEED)
        frame, st = oracle.render(case.buffers(oracle), p, shadow_any_hit=True)
        assert st.stackOverflows > 0, name                                   # the case is proven to reach the path
        _frames[name] = (case, p, frame, st)
    return _frames[name]


# ---------------------------------------------------------------------------------------------------------------------------
# ray queries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(QUERY_CASES))
def test_ray_queries_follow_the_rule(oracle, name):
    case = QUERY_CASES[name]()
    buffers = case.buffers(oracle)
    pt = case.tracer()
    try:
        for fam, f in case.families.items():
            n = len(f["rays"])
            rays = sc.pad128(f["rays"])
            row = np.arange(128) % n
            what = f"{name} {fam}"
            ref, ref_st = oracle.trace_rays(buffers, _oracle_rays(oracle, rays))
            assert (_bits(ref) == _bits(f["expected"][row])).all(), what       # the oracle gives the closed-form records (CPU test)
            hits, st = _query(pt, rays)
            same = (_bits(hits) == _bits(f["expected"][row])).all(axis=1)
            assert same.all(), (what, np.where(~same)[0][:8], hits[~same][:4], f["expected"][row][~same][:4])
            _stats_equal(st, ref_st, QUERY_COUNTERS, what)
            per_ray = 128 // n + (np.arange(n) < 128 % n)                      # copies of each ray in the padded batch
            assert st.stackOverflows == (per_ray.sum() if f["overflows"] else 0), what
            assert st.maxStackDepth == f["max_depth"], what
            # any hit: occluded exactly where the closest-hit expectation is a hit
            occ, st = _query(pt, rays, any_hit=True)
            _, ref_st = oracle.trace_rays(buffers, _oracle_rays(oracle, rays, any_hit=True))
            assert ((_bits(occ[:, 3]) != MISS) == f["hit"][row]).all(), what
            _stats_equal(st, ref_st, QUERY_COUNTERS, what + " any hit")
            # surface: the closest-hit records again, and the instance that owns the hit
            (hits2, surf), st = _query(pt, rays, surface=True)
            assert (_bits(hits2) == _bits(hits)).all(), what
            found = f["hit"][row]
            assert (_bits(surf[~found]) == 0).all(), what
            assert (_bits(surf[found, 3]) == _bits(hits[found, 0])).all() and (_bits(surf[found, 11]) == _bits(hits[found, 3])).all(), what
            if case.scene.use_tlas:
                assert (_bits(surf[found, 10]) == f["instance"][row][found]).all(), what
            assert st.stackOverflows == (per_ray.sum() if f["overflows"] else 0), what
    finally:
        pt.close()


def test_ray_queries_on_the_builder_made_chain(oracle):
    """No closed form here: the pinhole rays of every pixel against the oracle's records and counters."""
    case, p, _, _ = _oracle_frame(oracle, "geometric_chain")
    pt = case.tracer(p.OutputWidth, p.OutputHeight)
    try:
        rays = np.stack([pt.camera_ray(x, y, p) for y in range(p.OutputHeight) for x in range(p.OutputWidth)])
        buffers = case.buffers(oracle)
        for any_hit in (False, True):
            ref, ref_st = oracle.trace_rays(buffers, _oracle_rays(oracle, rays, any_hit))
            hits, st = _query(pt, rays, any_hit=any_hit)
            if any_hit:
                assert ((_bits(hits[:, 3]) != MISS) == (_bits(ref[:, 3]) != MISS)).all()
            else:
                assert (_bits(hits) == _bits(ref)).all()
            _stats_equal(st, ref_st, QUERY_COUNTERS, f"geometric chain any_hit={any_hit}")
            assert st.stackOverflows > 0
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------------
FRAME_RUNS = [(n, s, 0) for n in FRAME_CASES for s in (0, 1, 2, 3, 4)] + \
             [(n, 1, 2) for n in ("deep_blas_instances", "deep_tlas48", "geometric_chain")]      # the cleanup kernel finishes the paths


@pytest.mark.parametrize("name,schedule,iterations", FRAME_RUNS)
def test_frames_and_counters_equal_the_oracle(oracle, name, schedule, iterations):
    case, p, ref, ref_st = _oracle_frame(oracle, name)
    pt = case.tracer(p.OutputWidth, p.OutputHeight, samplesPerPass=p.SamplesPerPass, schedule=schedule)
    try:
        if iterations:
            pt.set_wavefront_iterations(iterations)
        pt.set_stats_level(1)
        pt.render_pass(p)
        gpu = pt.readback()
        bad = int((_bits(gpu) != _bits(ref)).any(axis=-1).sum())
        print(f"[stack] {name} schedule {schedule} iterations {iterations}: {bad} pixels differ, stackOverflows {pt.stats().stackOverflows}")
        assert bad == 0
        _stats_equal(pt.stats(), ref_st, ALL_COUNTERS, f"{name} schedule {schedule}")
        assert pt.stats().stackOverflows > 0
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the other entry points on the same walks
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deep_tlas48", "deep_cwbvh40"])
def test_guides_match_ray_queries(oracle, name):
    case, p, _, _ = _oracle_frame(oracle, name)
    W, H = p.OutputWidth, p.OutputHeight
    pt = case.tracer(W, H)
    try:
        rays = np.stack([pt.camera_ray(x, y, p) for y in range(H) for x in range(W)])
        hits, surf = pt.trace_rays(rays, surface=True)
        ref, _ = oracle.trace_rays(case.buffers(oracle), _oracle_rays(oracle, rays))
        assert (_bits(hits) == _bits(ref)).all()
        pt.render_guides(samples=1, params=p)
        alb, nd = pt.guides()
        h = (_bits(hits[:, 3]) != MISS).reshape(H, W)
        surf = surf.reshape(H, W, 12)
        assert h.any()
        assert (alb[~h] == np.array([1, 1, 1, 0], np.float32)).all() and (_bits(nd[~h]) == 0).all()
        assert (alb[h][:, 3] == 1).all()
        assert (_bits(nd[h][:, :3]) == _bits(surf[..., 4:7][h])).all()          # PTRaySurface.normal
        assert (_bits(nd[h][:, 3]) == _bits(surf[..., 3][h])).all()             # PTRaySurface.t
    finally:
        pt.close()


@pytest.mark.parametrize("name", ["deep_tlas48", "deep_cwbvh40"])
def test_radiance_of_the_camera_rays_is_the_frame(oracle, name):
    case, p2, _, _ = _oracle_frame(oracle, name)
    W, H = p2.OutputWidth, p2.OutputHeight
    p = sc.scenes.frame_params(case.scene, W, H, spp=1, seed=SEED)
    ref, st = oracle.render(case.buffers(oracle), p, shadow_any_hit=True)
    assert st.stackOverflows > 0
    pt = case.tracer(W, H, samplesPerPass=1, schedule=1)
    try:
        rays = pt.camera_rays(params=p)
        got = pt.radiance(rays, spp=1, params=p)
        pt.render_pass(p)
        frame = pt.readback()
        rgb = got[:, :3].reshape(H, W, 3)
        assert (_bits(frame) == _bits(ref)).all()
        assert (_bits(rgb) == _bits(frame[..., :3])).all()
    finally:
        pt.close()


@pytest.mark.parametrize("name", ["deep_tlas48", "deep_cwbvh40"])
def test_all_blocks_active_is_the_batch(oracle, name):
    case, p, _, _ = _oracle_frame(oracle, name)
    W, H, spp = p.OutputWidth, p.OutputHeight, p.SamplesPerPass
    seeds = [SEED + 10, SEED + 11]
    frames, stats = [], []
    for adaptive in (True, False):
        pt = case.tracer(W, H, samplesPerPass=spp, schedule=1)
        try:
            pt.OnRenderImage(SEED)
            pt.synchronize()
            pt.set_stats_level(1)
            pt.reset_stats()
            if adaptive:
                pt.adaptive_begin()
                pt.render_active(seeds)
            else:
                batch = []
                for j, s in enumerate(seeds):
                    pt._currentSample = spp + j * spp
                    batch.append(pt.params(s))
                plugin.check(pt.lib.PTRenderPassBatch(pt.ctx, (abi.PTFrameParams * 2)(*batch), 2))
            frames.append(pt.readback(last_output=False))
            st = pt.stats()
            stats.append((st.paths, st.closestHitRays, st.shadowRays, st.nodeVisits, st.stackOverflows, st.tlasNodeVisits))
        finally:
            pt.close()
    assert (_bits(frames[0]) == _bits(frames[1])).all(), name
    assert stats[0] == stats[1] and stats[0][4] > 0, (name, stats)


def test_direct_light_follows_the_rule_on_the_deep_tlas(oracle):
    """Direct light at the first hits of deep_tlas(48)'s rays, whose shadow rays push more than 32 TLAS entries: PTDirectLight must
    equal, bit for bit, PTDirectRays -> any-hit PTTraceRays -> PTDirectAccumulate, and PTDirectLightCulled over a one-cell grid.

    Which shadow rays can overflow follows from the construction.  A pair counts only when its light lies in front of the surface
    (N . L > 0, N turned towards the first ray).  The chain_first rays come from +x, so their hits face +x and their shadow rays
    run towards +x: the leaves below the hit lie behind such a ray and every leaf above it is nearer than the rest of the chain, so
    the stack never holds more than one entry.  The hits that face -x are the leaf_first rays': a shadow ray towards -x from the
    hit on instance j finds the rest of the chain first at every level below j and pushes leaf 0 ... j - 1: entries 32 ... j - 1
    are lost for j > 32.  So the list is the chain_first rays' first hits AND the leaf_first rays', 128 entries each, with one point
    light on either side; the light at -x stands where the quads j - 1, j - 2, ... shade the hit on quad j -- instances the
    overflowing walks lose, so the rule decides which of these entries are lit."""
    lights = np.stack([sc.scenes.pack_point_light((100.0, 24.0, 12.0), (1.0, 1.0, 1.0), 400.0, rng=1000.0),
                       sc.scenes.pack_point_light((-40.0, -28.0, 0.3), (1.0, 0.9, 0.8), 400.0, rng=1000.0)])
    case = sc.deep_tlas(48, lights=lights)
    pt = case.tracer()
    try:
        rays = np.concatenate([sc.pad128(case.families["chain_first"]["rays"]), sc.pad128(case.families["leaf_first"]["rays"])])
        hits, surf = pt.trace_rays(rays, surface=True)
        found = _bits(hits[:, 3]) != MISS
        assert found[128:].all() and found[:128].any() and not found[:128].all()     # chain first: entries 32 ... 46 are lost
        kw = dict(strata=1, centered=True)
        _, terms, recv, _ = pt.shade_surfaces(rays, hits, surf)
        pair_rays, contrib = pt.direct_rays(rays, terms, recv, **kw)
        pairs = pt.direct_pair_count(1)
        assert pairs == 2 and pair_rays.shape[0] == 2 * len(rays)
        counting = pair_rays[:, 6] > 0
        assert (counting.reshape(-1, 2) == np.stack([found & (np.arange(256) < 128), np.arange(256) >= 128], axis=1)).all()
        # the condition, on the CPU first: the oracle's any-hit walk of the pair rays overflows
        ref, ref_st = oracle.trace_rays(case.buffers(oracle), _oracle_rays(oracle, pair_rays, any_hit=True))
        assert ref_st.stackOverflows > 0
        pair_hits, st = _query(pt, pair_rays, any_hit=True)
        print(f"[stack] direct light on deep_tlas48: {int(counting.sum())} counting pairs, stackOverflows {st.stackOverflows} (oracle {ref_st.stackOverflows})")
        assert st.stackOverflows == ref_st.stackOverflows > 0
        occluded = _bits(pair_hits[:, 3]) != MISS
        assert (occluded == (_bits(ref[:, 3]) != MISS)).all()
        want = pt.direct_accumulate(terms, contrib, pair_hits, pairs)
        got = pt.direct_light(rays, hits, surf, **kw)
        assert (_bits(got) == _bits(want)).all()
        pt.build_light_grid((-64.0, -64.0, -64.0), 256.0, (1, 1, 1))
        assert (_bits(pt.direct_light(rays, hits, surf, culled=True, **kw)) == _bits(want)).all()
        # not vacuous: lit and shadowed entries on the side that overflows, light on the other side too
        lit = (want[:, 0:3] > 0).any(axis=1)
        assert lit[:128].any() and lit[128:].any() and (~lit[128:]).any() and occluded[counting].any() and not occluded[~counting].any()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# slab neighbours
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,deep,shallow", [("deep_cwbvh40", "chain_first", "terminal_first"), ("deep_tlas48", "chain_first", "leaf_first")])
def test_overflowing_lanes_leave_their_neighbours_alone(name, deep, shallow):
    """Overflowing rays on the odd lanes, shallow rays (triangle / instance 0 from the side where nothing accumulates) on the even
    ones.  The slab rows of a wave lie lane after lane: a push that strays past its row lands in the next lane's, and that lane's
    record changes.  The shallow rays' records must be those of the same rays traced alone -- and the expected ones."""
    case = QUERY_CASES[name]()
    pt = case.tracer()
    try:
        d, s = case.families[deep], case.families[shallow]
        n = len(d["rays"])
        mixed = np.zeros((128, 8), np.float32)
        mixed[1::2] = d["rays"][np.arange(64) % n]
        mixed[0::2] = s["rays"][0]
        alone = pt.trace_rays(np.ascontiguousarray(mixed[0::2]))
        for kw in ({}, {"any_hit": True}):
            got = pt.trace_rays(mixed, **kw)
            ref = pt.trace_rays(np.ascontiguousarray(mixed[0::2]), **kw)
            assert (_bits(got[0::2]) == _bits(ref)).all(), (name, kw)
        got = pt.trace_rays(mixed)
        assert (_bits(alone) == _bits(s["expected"][0])).all(axis=1).all(), name
        assert (_bits(got[0::2]) == _bits(s["expected"][0])).all(axis=1).all(), name
        assert (_bits(got[1::2]) == _bits(d["expected"][np.arange(64) % n])).all(), name
    finally:
        pt.close()


def test_schedule_1_keeps_shallow_pixels_beside_overflowing_ones(oracle):
    """The frame form of the same question, for the slabs of the wavefront schedule: in the deep_cwbvh(40) frame paths that overflow
    and paths that never leave the LDS part of the stack share waves; the megakernel (schedule 0) keeps its deep entries in a private
    array instead of a slab.  Both frames are the oracle's (test_frames_and_counters_equal_the_oracle); here they are compared
    with each other pixel by pixel, with the wave's rays reshuffled by a different number of wavefront iterations."""
    case, p, ref, _ = _oracle_frame(oracle, "deep_cwbvh40")
    frames = []
    for schedule, iterations in ((0, 0), (1, 0), (1, 3)):
        pt = case.tracer(p.OutputWidth, p.OutputHeight, samplesPerPass=p.SamplesPerPass, schedule=schedule)
        try:
            if iterations:
                pt.set_wavefront_iterations(iterations)
            pt.render_pass(p)
            frames.append(pt.readback())
        finally:
            pt.close()
    for f in frames:
        assert (_bits(f) == _bits(ref)).all()
