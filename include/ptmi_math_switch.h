/*
 * ptmi_math_switch.h — ONE dispatch over the functions of include/ptmi_math.h, bit patterns in and out (test infrastructure).
 *
 * Included by oracle/pt_oracle.cpp (oracle_math, oracle_math_n: the host evaluation) and by
 * unity_webgpu_pathtracer_amd/csrc/math_probe.hip (PTMathProbe: the same switch inside a kernel), so the two sides of
 * tests/test_gpu_math.py cannot drift apart.  tests/math_cases.py names the numbers and says which inputs each one gets.
 *
 * x and y are the operands' bits: a float's for the float functions (a signalling NaN or a payload arrives unaltered), the
 * integer itself for unorm8 (14, 15) and the RNG (29, 30).  The result is a float's bits, or the integer for f2u / f2i /
 * the RNG state / the quadrant.
 */
#ifndef PT_MATH_SWITCH_H
#define PT_MATH_SWITCH_H

#include "ptmi_math.h"

#define PT_MATH_FN_COUNT 33

PT_HD uint32_t pt_math_switch(int fn, uint32_t xbits, uint32_t ybits)
{
    const float x = pt_asfloat(xbits), y = pt_asfloat(ybits);
    switch (fn) {
    case 0: return pt_asuint(pt_sin(x));
    case 1: return pt_asuint(pt_cos(x));
    case 2: return pt_asuint(pt_log(x));
    case 3: return pt_asuint(pt_log2(x));
    case 4: return pt_asuint(pt_exp2(x));
    case 5: return pt_asuint(pt_pow(x, y));
    case 6: return pt_asuint(pt_acos(x));
    case 7: return pt_asuint(pt_asin(x));
    case 8: return pt_asuint(pt_sqrt(x));
    case 9: return pt_asuint(pt_rcp(x));
    case 10: return pt_asuint(pt_atan2(x, y));                    /* x = the y-argument, y = the x-argument */
    case 11: return pt_asuint(pt_fmod(x, y));
    case 12: return pt_asuint(pt_wrap01(x));
    case 13: {                                    /* the literal loops of util/texture.hlsl:41-48 (with this project's guard) */
        float u = x;
        if (pt_abs(u) >= 16777216.0f) u = 0.0f;
        while (u > 1.0f) u -= 1.0f;
        while (u < 0.0f) u += 1.0f;
        return pt_asuint(u);
    }
    case 14: return pt_asuint(pt_unorm8(xbits));                  /* the kernels' form of a texel channel ... */
    case 15: return pt_asuint((float)(xbits & 0xFFu) / 255.0f);   /* ... and the division of util/texture.hlsl that the oracle performs */
    case 16: return pt_asuint(pt_atan(x));
    case 17: return pt_asuint(pt_rsqrt(x));
    case 18: return pt_asuint(pt_floor(x));
    case 19: return pt_asuint(pt_ceil(x));
    case 20: return pt_asuint(pt_rint(x));
    case 21: return pt_asuint(pt_trunc(x));
    case 22: return pt_asuint(pt_min(x, y));
    case 23: return pt_asuint(pt_max(x, y));
    case 24: return pt_asuint(pt_clamp(x, 0.0f, y));
    case 25: return pt_asuint(pt_saturate(x));
    case 26: return pt_asuint(pt_lerp(0.0f, x, y));
    case 27: return pt_f2u(x);
    case 28: return (uint32_t)pt_f2i(x);
    case 29: { uint32_t s = xbits; pt_rng_next(&s); return s; }                    /* state in, state out */
    case 30: { uint32_t s = xbits; return pt_asuint(pt_random_float(&s)); }        /* state in, float out */
    case 31: { int32_t q; return pt_asuint(pt_sincos_reduce(x, &q)); }             /* the reduced argument ... */
    case 32: { int32_t q; (void)pt_sincos_reduce(x, &q); return (uint32_t)q; }     /* ... and the quadrant */
    default: return 0u;
    }
}

#endif /* PT_MATH_SWITCH_H */
