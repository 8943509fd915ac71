"""What the tests of the solver's own logarithm share (tests/test_math_log.py on the host build, tests/test_gpu_math.py on the
device): the host build of csrc/obca_math.h and the seeded argument families.  Test infrastructure only."""
import ctypes
import functools
import os

import numpy as np

from tests import native_build

N_FAMILY = 1 << 20


@functools.lru_cache(maxsize=None)
def _lib():
    return native_build.build_shim("math_host", [os.path.join(native_build.NATIVE, "math_host.cpp")])


def host_log(x):
    """obca_log (csrc/obca_math.h) of the float64 array ``x``, host build"""
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    _lib().math_host_log(ctypes.c_longlong(x.size), x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return out


def whole_range(n=N_FAMILY, seed=1):
    """log-uniform over every positive finite double: mantissa uniform in [1, 2), exponent uniform in -1074 .. 1023 (denormals included)"""
    rng = np.random.default_rng(seed)
    x = np.ldexp(1.0 + rng.uniform(size=n), rng.integers(-1074, 1024, size=n).astype(np.int32))
    return x[x > 0.0]


def around_one(n=N_FAMILY, seed=2):
    """1 +- 2^-u, u uniform in [0, 40]: where log(x) loses its leading digits (below 1: u >= 1, so x in [1/2, 1))"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 40.0, size=n)
    below = rng.integers(0, 2, size=n).astype(bool)
    return np.where(below, 1.0 - np.exp2(-np.maximum(u, 1.0)), 1.0 + np.exp2(-u))


def barrier_products(n=N_FAMILY, seed=3):
    """products of three or four distances, each log-uniform in [1e-9, 1e2]: what row_barrier (csrc/obca_kernel.hip) takes the log of"""
    rng = np.random.default_rng(seed)
    f = 10.0 ** rng.uniform(-9.0, 2.0, size=(n, 4))
    f[rng.integers(0, 2, size=n).astype(bool), 3] = 1.0
    return f[:, 0] * f[:, 1] * f[:, 2] * f[:, 3]


FAMILIES = {"whole_range": whole_range, "around_one": around_one, "barrier_products": barrier_products}


def ulp_error(y, x):
    """|y - log(x)| in units of the last place of the double nearest log(x), with log(x) in long double (x87 extended: 64 bits)"""
    assert np.finfo(np.longdouble).nmant >= 63                      # a reference 2^11 times finer than a double
    ref = np.log(x.astype(np.longdouble))
    return np.abs(y.astype(np.longdouble) - ref) / np.spacing(np.abs(ref.astype(np.float64))).astype(np.longdouble)
