"""include/ptmi_math.h evaluated ON THE DEVICE, function by function, against the oracle's evaluation of the same switch
(include/ptmi_math_switch.h) on the host: the claim every bit-exact check of this project rests on -- both sides include one header, are
compiled without contraction and so compute the same bits -- tested directly instead of through whatever arguments the rendered
scenes happen to produce.

libpt-math-probe.so (csrc/math_probe.hip, `make math-probe`; test-only) holds one kernel, one element per lane, compiled twice: unit 0
with the flags of the product's kernels, unit 1 with those of the default schedule's unit.  The inputs are tests/math_cases.py's.

The contract: where the oracle's result is not a NaN the device's bits equal it, the sign of a zero included; where it is a NaN the
device's is a NaN (sign and payload of a NaN are not part of the contract: x86 generates 0xFFC00000, gfx950 0x7FC00000).  The two units
agree on every bit of every element."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import math_cases as mc
from math_cases import FN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "lib", "libpt-math-probe.so")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    """device(unit, fn, xbits, ybits=None) -> result bits, through PTMathProbe."""
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "unity_webgpu_pathtracer_amd", "csrc"), "math-probe"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(PROBE)
    lib.PTMathProbe.restype = C.c_int
    lib.PTMathProbe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]

    def run(unit, fn, xbits, ybits=None):
        x = np.ascontiguousarray(xbits, dtype=np.uint32)
        y = np.zeros_like(x) if ybits is None else np.ascontiguousarray(ybits, dtype=np.uint32)
        assert x.ndim == 1 and x.shape == y.shape
        out = np.full_like(x, 0xDEADBEEF)
        err = lib.PTMathProbe(unit, fn, x.ctypes.data, y.ctypes.data, x.size, out.ctypes.data)
        assert err == 0, f"PTMathProbe(unit {unit}, fn {fn}, n {x.size}) returned hipError {err}"
        return out
    return run


@pytest.mark.parametrize("name", list(FN))
def test_device_bits_equal_the_oracle(name, device, oracle):
    """Every element of the function's input sets, both units.  A failure lists function, input bits, host bits, device bits."""
    x, y = mc.cases(name)
    host = oracle.math_n(FN[name], x, y)
    dev = [device(unit, FN[name], x, y) for unit in (0, 1)]
    both = np.flatnonzero(dev[0] != dev[1])
    assert both.size == 0, f"{name}: the two units differ on {both.size} elements, first x=0x{int(x[both[0]]):08X} y=0x{int(y[both[0]]):08X}: " \
                           f"0x{int(dev[0][both[0]]):08X} / 0x{int(dev[1][both[0]]):08X}"
    mc.assert_same_bits(name, x, y, dev[0], host, "device", "host")


def test_rng_four_steps_on_the_device(device, oracle):
    """The KNOWN seeds and 2^16 random states, four steps each, the device's own state fed back in."""
    s_dev = s_host = mc.rng_states()
    for step in range(4):
        r_dev, r_host = device(0, FN["random_float"], s_dev), oracle.math_n(FN["random_float"], s_host)
        s_dev, s_host = device(0, FN["rng_next"], s_dev), oracle.math_n(FN["rng_next"], s_host)
        assert np.array_equal(s_dev, s_host) and np.array_equal(r_dev, r_host), step
        assert np.array_equal(r_dev, mc.bits(s_dev.astype(np.float32) / np.float32(4294967296.0)))


def test_accuracy_on_the_device(device):
    """tests/test_math.py::test_accuracy_on_the_domain_sets on the device's outputs (both units): the file means something on its own
    even if oracle and device were wrong together.  exp2 also over every float of [127, 128): finite and within its bound."""
    for unit in (0, 1):
        mc.check_accuracy(lambda fn, x: device(unit, fn, x))
        top = mc.exp2_top()
        got = device(unit, FN["exp2"], top)
        assert np.isfinite(mc.floats(got)).all()
        assert mc.ulp_err(got, np.exp2(mc.floats(top).astype(np.float64))).max() <= mc.ULP_BOUND["exp2"]


def test_pow_is_exp2_of_y_log2_x_on_the_device(device):
    """pow(x, y) == exp2(fl(y * log2(x))) composed from the device's own log2 and exp2 and one float32 multiplication in numpy."""
    x, y = mc.cases("pow")
    with np.errstate(all="ignore"):
        t = mc.floats(y) * mc.floats(device(0, FN["log2"], x))
    mc.assert_same_bits("pow", x, y, device(0, FN["pow"], x, y), device(0, FN["exp2"], mc.bits(t)), "pow", "exp2(y*log2 x)")
