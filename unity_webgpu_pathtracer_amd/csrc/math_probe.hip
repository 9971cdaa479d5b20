/*
 * math_probe.hip — evaluates the functions of include/ptmi_math.h ON THE DEVICE, one element per lane (test infrastructure:
 * libpt-math-probe.so, `make math-probe`; not part of the product library).
 *
 * tests/test_gpu_math.py compares the bits this returns with the oracle's (oracle_math_n), which runs the same switch
 * (include/ptmi_math_switch.h) on the host: the claim at the top of ptmi_math.h, function by function.
 *
 * Compiled twice, as the product's kernels are: this file with HIPFLAGS holds the entry point and the kernel of unit 0;
 * with HIPFLAGS_A and -DPT_MATH_PROBE_UNIT_A (the flags of the default schedule's unit) it holds the kernel of unit 1 only.
 */
#include <hip/hip_runtime.h>

#include "ptmi_math_switch.h"

#ifdef PT_MATH_PROBE_UNIT_A
#define PROBE_KERNEL pt_math_probe_kernel_a
#define PROBE_LAUNCH pt_math_probe_launch_a
#else
#define PROBE_KERNEL pt_math_probe_kernel
#define PROBE_LAUNCH pt_math_probe_launch
#endif

__global__ __launch_bounds__(256) void PROBE_KERNEL(int fn, const uint32_t* __restrict__ x, const uint32_t* __restrict__ y,
                                                    uint64_t n, uint32_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = pt_math_switch(fn, x[i], y[i]);
}

hipError_t PROBE_LAUNCH(int fn, const uint32_t* x, const uint32_t* y, uint64_t n, uint32_t* out)
{
    PROBE_KERNEL<<<dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, 0>>>(fn, x, y, n, out);
    return hipGetLastError();
}

#ifndef PT_MATH_PROBE_UNIT_A
hipError_t pt_math_probe_launch_a(int fn, const uint32_t* x, const uint32_t* y, uint64_t n, uint32_t* out);

/* Host arrays in and out; 0 on success, a hipError_t otherwise (unit: 0 = HIPFLAGS, 1 = HIPFLAGS_A; anything else is an error). */
extern "C" __attribute__((visibility("default")))
int PTMathProbe(int unit, int fn, const uint32_t* xbits, const uint32_t* ybits, uint64_t n, uint32_t* outbits)
{
    if ((unit != 0 && unit != 1) || fn < 0 || fn >= PT_MATH_FN_COUNT || !xbits || !ybits || !outbits || n > (1ull << 30))
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    uint32_t *dx = nullptr, *dy = nullptr, *dout = nullptr;
    hipError_t e = hipSetDevice(0);
    if (e == hipSuccess) e = hipMalloc(&dx, bytes);
    if (e == hipSuccess) e = hipMalloc(&dy, bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, bytes);
    if (e == hipSuccess) e = hipMemcpy(dx, xbits, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy, ybits, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = unit ? pt_math_probe_launch_a(fn, dx, dy, n, dout) : pt_math_probe_launch(fn, dx, dy, n, dout);
    if (e == hipSuccess) e = hipMemcpy(outbits, dout, bytes, hipMemcpyDeviceToHost);      /* synchronises with the kernel */
    (void)hipFree(dx);
    (void)hipFree(dy);
    (void)hipFree(dout);
    return (int)e;
}
#endif
