// obca_math.h -- the solver's own elementary functions, for host and device alike.
//
// obca_log(x): natural logarithm for the barrier function (csrc/obca_kernel.hip: dlog, dpow).  The device library's log() is
// a general-purpose routine (double-double arithmetic, denormal pre-scaling); the barrier takes a log of a product of three or
// four distances and needs a faithful one, not a correctly rounded one.  Classic form:
//   x = m 2^k with m in [sqrt(1/2), sqrt(2)), f = m - 1 (exact), s = f / (2 + f), z = s^2,
//   log(1 + f) = f - f^2/2 + s (f^2/2 + R(z)),  R(z) = z (L1 + z (L2 + ... + z L7)) ~ log((1+s)/(1-s)) - 2s, |R error| < 2^-58.45,
//   log(x) = k ln2_hi - ((f^2/2 - (s (f^2/2 + R) + k ln2_lo)) - f),   ln2_hi has 21 trailing zero bits: k ln2_hi is exact.
// Every operation is an IEEE addition, multiplication, fused multiply-add (written fma(): nothing is left to contraction) or
// the one correctly rounded division, so a host build returns the device's word bit for bit.  frexp normalises denormals:
// no pre-scaling.  Largest error measured against long double on the host: tests/test_math_log.py.
// Special classes: +0 / -0 -> -inf, x < 0 -> NaN, +inf -> +inf, NaN -> NaN.
#ifndef OBCA_MATH_H
#define OBCA_MATH_H

#include <math.h>

#if defined(__HIPCC__)
#define OBCA_MATH_FN __host__ __device__ inline
#else
#define OBCA_MATH_FN inline
#endif

#if defined(__HIPCC__)
// Sine and cosine of the stage angles (device only: the host core stays on libm).  The device library's sincos() shares one
// argument reduction between the two and returns the words of its separate sin() and cos() (tests/test_gpu_math.py).
__device__ inline void obca_sincos(double x, double* s, double* c) { sincos(x, s, c); }
#endif

OBCA_MATH_FN double obca_log(double x) {
    // positive and finite (denormals included)?  One class compare where the compiler has it, two comparisons elsewhere: the
    // same predicate.  Not taken by the barrier of an interior iterate.
#if defined(__clang__)
    if (!__builtin_isfpclass(x, 0x180))                      // fcPosSubnormal | fcPosNormal
#else
    if (!(x > 0.0 && x < INFINITY))
#endif
        return x == 0.0 ? -INFINITY : (x > 0.0 ? x : NAN);   // (NaN fails both comparisons)
    int k;
    double m = frexp(x, &k);                                 // m in [1/2, 1)
    const bool low = m < 0.70710678118654752440;
    m = low ? 2.0 * m : m;                                   // m in [sqrt(1/2), sqrt(2))
    k = low ? k - 1 : k;
    const double f = m - 1.0, dk = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double R = 1.479819860511658591e-01;                                  // L7 ... L1: the minimax coefficients of R(z) / z
    R = fma(R, z, 1.531383769920937332e-01);
    R = fma(R, z, 1.818357216161805012e-01);
    R = fma(R, z, 2.222219843214978396e-01);
    R = fma(R, z, 2.857142874366239149e-01);
    R = fma(R, z, 3.999999999940941908e-01);
    R = fma(R, z, 6.666666666666735130e-01);
    const double hfsq = 0.5 * f * f;
    const double u = fma(dk, 1.90821492927058770002e-10, s * fma(R, z, hfsq));       // ln2_lo
    return fma(dk, 6.93147180369123816490e-01, -((hfsq - u) - f));                   // ln2_hi
}

#endif
