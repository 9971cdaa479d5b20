"""Inputs the reflection-probe tests share (tests/test_reflection.py on the host twins, tests/test_gpu_reflection.py on the kernels):
random positive maps, the lookup's query set with its edge cases, and boxes around off-centre probes."""
import math

import numpy as np

from unity_webgpu_pathtracer_amd import plugin

F = np.float32
ROUGHNESS = [0.0, 1.0, 0.5, 1.0 / 3.0, -1.0, 2.0, math.nan]
PREFILTER_SHAPES = [(8, 2), (16, 3)]            # (res, levels)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def random_base(n, res, seed):
    """(n, res * res, 4) float32 positive radiance; aux random too (the prefilter must not read it)"""
    return np.random.default_rng(seed).uniform(0.05, 4.0, (n, res * res, 4)).astype(F)


def random_maps(n, res, levels, seed):
    return np.random.default_rng(seed).uniform(0.05, 4.0, (n, plugin.reflection_texel_count(res, levels), 4)).astype(F)


def edge_directions():
    """the six axes, directions with z = 0 (the fold line), on the x = 0 and y = 0 creases, and at and around the -z pole"""
    d = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    for t in np.linspace(0.0, 2.0 * math.pi, 24, endpoint=False):
        d.append((math.cos(t), math.sin(t), 0.0))
    for t in np.linspace(0.05, math.pi - 0.05, 12):
        d += [(0.0, math.sin(t), math.cos(t)), (0.0, -math.sin(t), math.cos(t)), (math.sin(t), 0.0, math.cos(t)), (-math.sin(t), 0.0, math.cos(t))]
    for e in (1e-3, 1e-5):
        d += [(e, e, -1.0), (-e, e, -1.0), (e, -e, -1.0), (-e, -e, -1.0), (e, 0.0, -1.0), (0.0, -e, -1.0)]
    return unit(d)


def query_set(probe_count, n=4096, seed=11):
    """(n, 8) float32 PTReflectionQuery rows: random unit directions plus the edge cases, every roughness of ROUGHNESS, positions
    inside and outside the unit boxes of probe_boxes(), one probe index out of range (row 7)"""
    rng = np.random.default_rng(seed)
    edges = edge_directions()
    d = unit(rng.normal(0, 1, (n, 3)))
    d[:len(edges)] = edges
    # every edge direction at every roughness, then random pairs
    rough = rng.uniform(-0.1, 1.1, n).astype(F)
    k = len(edges)
    for i, r in enumerate(ROUGHNESS):
        d[k + i * len(edges):k + (i + 1) * len(edges)] = edges
        rough[k + i * len(edges):k + (i + 1) * len(edges)] = r
    rough[:len(ROUGHNESS)] = ROUGHNESS
    probes = rng.integers(0, probe_count, n).astype(np.uint32)
    probes[7] = probe_count
    pos = rng.uniform(-0.45, 0.45, (n, 3)).astype(F)
    pos[::5] = rng.uniform(0.6, 2.0, (len(pos[::5]), 3)).astype(F)          # outside every box
    return plugin.reflection_query_rows(d, rough, probes, pos)


def probe_boxes(probe_count, seed=12):
    """probe positions (n, 3) off the centre of the boxes (n, 8) = [-0.5, 0.5]^3 stretched a little per probe"""
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-0.3, 0.3, (probe_count, 3)).astype(F)
    lo = (-0.5 - rng.uniform(0, 0.2, (probe_count, 3))).astype(F)
    hi = (0.5 + rng.uniform(0, 0.2, (probe_count, 3))).astype(F)
    return Q, plugin.reflection_box_rows(lo, hi)
