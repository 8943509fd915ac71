"""obca_log (csrc/obca_math.h), host build, against numpy's long double logarithm.  No GPU.

Bound: 1 ulp, what the device library documents for the fp64 log() that obca_log replaces in the barrier function.
Measured on 2^20 arguments per family (tests/math_case.py, fixed seeds): whole_range 0.728 ulp, around_one 0.807 ulp,
barrier_products 0.731 ulp (four more seeds each: at most 0.787 ulp); numpy's own log on the same arguments: 0.576, 0.610, 0.551."""
import numpy as np
import pytest

from tests import math_case as mc


@pytest.mark.parametrize("family", sorted(mc.FAMILIES))
def test_largest_error_is_below_one_ulp(family):
    x = mc.FAMILIES[family]()
    assert x.size > 0.99 * mc.N_FAMILY and np.all(x > 0.0) and np.all(np.isfinite(x))
    err = mc.ulp_error(mc.host_log(x), x)
    worst = int(np.argmax(err))
    print("obca_log %s: largest error %.3f ulp at x = %r (numpy's log: %.3f ulp)" % (family, float(err[worst]), float(x[worst]),
                                                                                   float(mc.ulp_error(np.log(x), x).max())))
    assert float(err[worst]) <= 1.0


def test_special_classes():
    """+0 and -0 give -inf, a negative argument NaN, +inf itself, NaN NaN; 1 gives +0 exactly"""
    with np.errstate(all="ignore"):
        y = mc.host_log(np.array([0.0, -0.0, -1.0, -np.inf, -5e-324, np.inf, np.nan, 1.0]))
    assert y[0] == -np.inf and y[1] == -np.inf
    assert np.isnan(y[2]) and np.isnan(y[3]) and np.isnan(y[4])
    assert y[5] == np.inf
    assert np.isnan(y[6])
    assert y[7] == 0.0 and not np.signbit(y[7])


def test_denormals_and_the_largest_finite_argument():
    """no special path: frexp normalises a denormal, and the largest double has exponent 1024 in frexp's convention"""
    x = np.array([5e-324, 2.5e-320, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.7976931348623157e308])
    y = mc.host_log(x)
    assert np.all(np.isfinite(y))
    assert float(mc.ulp_error(y, x).max()) <= 1.0
    assert y[0] == pytest.approx(-744.4400719213812, rel=1e-15) and y[-1] == pytest.approx(709.782712893384, rel=1e-15)
