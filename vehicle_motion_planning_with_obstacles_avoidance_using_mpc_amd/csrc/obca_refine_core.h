// obca_refine_core.h -- the refinement step of the two-stage open-loop planner: a plan of N intervals resampled to
// ratio x N, yaws recomputed, step rescaled (closedLoop.update_path(allAviable=1) + a_star.create_reference_path of the
// host mirror; reference src/closed_loop.py:567-589, src/a_star.py:189-200).  One function per OUTPUT POINT, shared by
// refine_kernel of csrc/obca_refine.hip (one lane per point) and the host build (tests/native/plan_refine_host.cpp).
//
// Arithmetic, for a plan x [3,N+1], step ts and integer ratio r >= 1, N2 = r N:
//   point j < N2   i = j / r, q = j % r:  p = (double)q * ((x[i+1] - x[i]) / (double)r) + x[i]  per coordinate -- numpy's
//                  linspace(x[i], x[i+1], num=r, endpoint=False)[q] word for word, PROVIDED the multiply-add is not
//                  contracted to an FMA: the function carries `fp contract(off)` (the library is built with contraction on)
//   point N2       knot N itself
//   yaw_j          atan2(py_j+1 - py_j, px_j+1 - px_j) for j < N2, yaw_N2 = yaw_N2-1: every point recomputes its successor,
//                  so that no point depends on another lane's result
//   ts_out         ((double)N * ts) / (double)N2
// Pass-through (nothing a later launch reads may be NaN): status outside {0, 1}, a knot (x, y or yaw) that is not finite, a
// difference of neighbouring positions that is not finite (0 x inf would be NaN), ts not finite or <= 0.  Such an instance
// gets variant 0, knot 0 of the plan at every point (zeros if that knot is not finite) and ts_out = ts / r where finite,
// else 0.
#ifndef OBCA_REFINE_CORE_H
#define OBCA_REFINE_CORE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_FN __host__ __device__ inline
#else
#define RF_FN inline
#endif

namespace refine {

constexpr int MAX_N = 127;                 // the longest horizon obca_create takes (csrc/obca_capi.hip: dims_ok)
constexpr int E_INVAL = -22;               // OBCA_E_INVAL

RF_FN bool finite_(double v) { return v - v == 0.0; }          // false for NaN and +-inf, no libm call

// the checks of obca_plan_refine, made before anything is read or written (the host build makes the same ones)
RF_FN int args_check(int32_t B, int32_t N, int32_t ratio, const double* x, const double* ts, int32_t variant_ok,
                     const double* xref_out, const double* ts_out) {
    if (B < 1 || N < 1 || N > MAX_N || ratio < 1 || ratio > MAX_N || (int64_t)ratio * N > MAX_N) return E_INVAL;
    if (variant_ok != 4 && variant_ok != 6 && variant_ok != 8) return E_INVAL;
    if (!x || !ts || !xref_out || !ts_out) return E_INVAL;
    return 0;
}

// is instance (x [3,N+1], ts, status) refined (true) or passed through (false)
RF_FN bool usable(const double* x, int N, double ts, int status) {
    bool ok = (status == 0 || status == 1) && finite_(ts) && ts > 0.0;
    for (int k = 0; k <= N; ++k)
        ok = ok && finite_(x[k]) && finite_(x[N + 1 + k]) && finite_(x[2 * (N + 1) + k]);
    for (int k = 0; k < N && ok; ++k)
        ok = finite_(x[k + 1] - x[k]) && finite_(x[N + 1 + k + 1] - x[N + 1 + k]);
    return ok;
}

// position j (0 <= j <= r N) of the resampled plan; row: x (the plan's x row) or x + N + 1 (its y row)
RF_FN double coord(const double* row, int N, int r, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (j >= r * N) return row[N];
    const int i = j / r, q = j - i * r;
    const double step = (row[i + 1] - row[i]) / (double)r;
    const double prod = (double)q * step;
    return prod + row[i];
}

// output point j (0 <= j <= r N) of one instance: out = (px, py, yaw)
RF_FN void point(const double* x, int N, int r, int j, bool ok, double out[3]) {
    const int N1 = N + 1, N2 = r * N;
    if (!ok) {
        const bool k0 = finite_(x[0]) && finite_(x[N1]) && finite_(x[2 * N1]);
        out[0] = k0 ? x[0] : 0.0; out[1] = k0 ? x[N1] : 0.0; out[2] = k0 ? x[2 * N1] : 0.0;
        return;
    }
    const int j0 = j < N2 ? j : N2 - 1;                        // the last point repeats the previous yaw
    const double ax = coord(x, N, r, j0), ay = coord(x + N1, N, r, j0);
    const double bx = coord(x, N, r, j0 + 1), by = coord(x + N1, N, r, j0 + 1);
    out[0] = j < N2 ? ax : bx;
    out[1] = j < N2 ? ay : by;
    out[2] = atan2(by - ay, bx - ax);
}

RF_FN double step_out(int N, int r, double ts, bool ok) {
    if (ok) return ((double)N * ts) / (double)(r * N);
    return finite_(ts) ? ts / (double)r : 0.0;
}

}  // namespace refine

#endif
