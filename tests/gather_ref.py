"""The irradiance-gather rule (include/ptmi_plugin.h Part 13) restated in numpy float32, for tests/test_gpu_gather.py: the seed
rule, the point- and spot-light lines of EvalLight, the Lambert term and the luminance of a sample.  Written from the header's
text and util/light.hlsl's formulas, not from the device code; every operation is one float32 operation in the rule's order."""
import numpy as np

F = np.float32
PI = F(3.14159265358979323)
EPSILON = F(0.0001)
M32 = 0xFFFFFFFF


def rng_next(s: int) -> int:
    """pt_rng_next (include/ptmi_math.h): one PCG step on a uint32 state"""
    old = (s + 747796405 + 2891336453) & M32
    word = (((old >> ((old >> 28) + 4)) ^ old) * 277803737) & M32
    return ((word >> 22) ^ word) & M32


def sample_seed(seed: int, first_sample: int, j: int) -> int:
    """the RNG state sample j of an entry starts with: s = seed; pt_rng_next(&s); s += firstSample + j"""
    return (rng_next(seed & M32) + first_sample + j) & M32


def _dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def _normalize(v):
    return v * F(F(1.0) / np.sqrt(_dot(v, v), dtype=F))


def _saturate(x):
    return F(min(max(x, F(0.0)), F(1.0)))


def luminance(c):
    """luminance3 of (..., 3) float32 colours"""
    c = np.asarray(c, F)
    return (c[..., 0] * F(0.299) + c[..., 1] * F(0.587)) + c[..., 2] * F(0.114)


def direct_irradiance(light, P, N):
    """E at a receiver from ONE unoccluded point or spot light (a packed 16-float light record, scenes.pack_*_light):
    emission * falloff * max(dot(N, L), 0), the value the issue's closed form names.  Returns (3,) float32."""
    light = np.asarray(light, F)
    P, N = np.asarray(P, F), np.asarray(N, F)
    pos, emission, rng_ = light[0:3], light[4:7], light[7]
    ltype = int(light[3:4].view(np.uint32)[0])
    scatter = P + N * EPSILON
    if ltype == 2:                                   # point
        ls_normal = _normalize(scatter - pos)
        L = -ls_normal
    elif ltype == 0:                                 # spot
        L = -_normalize(scatter - pos)
    else:
        raise ValueError("closed form for point and spot lights only")
    d = pos - scatter if ltype == 0 else scatter - pos
    dist = np.sqrt(_dot(d, d), dtype=F)
    if dist > rng_:
        falloff = F(0.0)
    else:
        r = F(dist / rng_)
        falloff = _saturate(F(F(1.0) / F(F(1.0) + F(F(25.0) * r) * r)) * _saturate(F(F(1.0) - r) * F(5.0)))
    if ltype == 0:
        axis = _normalize(_normalize(light[8:11]))
        cos_theta = _dot(_normalize(-L), axis)
        outer, inner = light[12], light[13]
        if cos_theta < outer:
            falloff = F(0.0)
        elif outer < cos_theta < inner:
            falloff = F(falloff * F(F(cos_theta - outer) / F(inner - outer)))
    cos_n = max(_dot(N, L), F(0.0))
    return (emission * falloff * F(cos_n)).astype(F)
