// obca_scene_core.h -- scene pools: which obstacles of a pool of up to 64 a solve sees.  One pool per instance, K convex
// obstacles of exactly E rows each, every one optionally translating at a constant velocity; the n_sel obstacles nearest to a
// set of poses (a reference window, later the plans solved against the last selection) are gathered into obca_solve_batch's
// rows.  Plain functions shared by scene_kernel of csrc/obca_scene.hip (one wavefront per instance, one lane per pool
// obstacle) and the host build (tests/native/scene_host.cpp): the score of one obstacle, the rank of one obstacle among the
// K scores, one output row.  The distance is audit::signed_distance<4> on audit::car_corners (csrc/obca_audit_core.h),
// the samples between the knots are obca_plan_sweep's (audit::sample_pose, audit::lerp_end).
//
// Arithmetic.
//   rows at stage kk  A as given, b_kk[r] = b[r] + (kk * Ts) * (A[r,0] v_x + A[r,1] v_y): the products and sums rounded one by
//                     one (`fp contract(off)`: the library is built with contraction on), so that host and device write the
//                     same words.  Exact for a set that translates by kk Ts v (a q <= b becomes a (q - d) <= b).  Without
//                     velocities b_kk = b, no operation at all.
//   samples           x0 where given (against stage 0's rows), then interval s = 0 .. N-1 at the fractions j / n_sub,
//                     j = 0 .. n_sub (every knot once): pose by audit::sample_pose, b by audit::lerp_end between b_s and
//                     b_s+1 -- the words of obca_plan_sweep on the same rows.  variant 4: stage 0's rows at every sample
//                     (what obca_mpc4 reads).  A sample whose pose is not finite is skipped.
//   score             the smallest sampled signed distance; accumulate: min(old score, this call's smallest)
//   rank of i         the number of j with score_j < score_i, or score_j == score_i and j < i: ties go to the lower pool
//                     index.  Selected: rank < n_sel.  The slot of a selected obstacle is the number of selected obstacles of
//                     lower index, so sel is ascending in pool index.
//
// An instance is unusable -- ok 0, variant_out 0, sel = 0 .. n_sel-1, score untouched, every output row a = (1, 0),
// b = -1e6 (a half-plane 10^6 m to the left of everything: never active, never NaN) -- when a pool row, a velocity or a Ts
// it needs is not finite, when a pool row has a = (0, 0) (no half-plane), when no sample pose is finite, when a distance comes
// out as NaN (overflow), or when it is not measured (accumulate) and the selection passed in is not an ascending list of
// pool indices.
#ifndef OBCA_SCENE_CORE_H
#define OBCA_SCENE_CORE_H

#include <math.h>
#include <stdint.h>
#include "obca_audit_core.h"

#if defined(__HIPCC__)
#define SC_FN __host__ __device__ inline
#else
#define SC_FN inline
#endif

namespace scene {

constexpr int MAX_K = 64;                  // one lane per pool obstacle
constexpr int MAX_SEL = 8;                 // OBCA_MAX_OBST
constexpr int MAX_E = 4;                   // OBCA_MAX_EDGES
constexpr int MAX_N = 127;                 // the longest horizon obca_create takes
constexpr int MAX_SUB = 256;               // samples per interval: a lane measures N n_sub + 2 poses at the most
constexpr int E_INVAL = -22;               // OBCA_E_INVAL
constexpr double FILL_B = -1e6;            // rows of an unusable instance: a = (1, 0), b = FILL_B

SC_FN bool finite_(double v) { return v - v == 0.0; }          // false for NaN and +-inf, no libm call

// the checks of obca_scene_select, made before anything is read or written (the host build makes the same ones)
SC_FN int args_check(int32_t B, int32_t K, int32_t E, int32_t N, int32_t n_sel, int32_t n_sub, int32_t accumulate,
                     const double* ego, const double* pool_A, const double* pool_b, const double* pool_v, const double* Ts,
                     const double* x, const double* score, const int32_t* sel, const double* A_out, const double* b_out,
                     const int32_t* variant_out, const int32_t* ok_out) {
    if (B < 1 || K < 1 || K > MAX_K || E < 1 || E > MAX_E || N < 1 || N > MAX_N) return E_INVAL;
    if (n_sel < 1 || n_sel > MAX_SEL || n_sel > K || n_sub < 1 || n_sub > MAX_SUB) return E_INVAL;
    if (accumulate != 0 && accumulate != 1) return E_INVAL;
    if (!ego || !pool_A || !pool_b || !x || !score || !sel || !A_out || !b_out || !variant_out || !ok_out) return E_INVAL;
    if (pool_v && !Ts) return E_INVAL;
    for (int q = 0; q < 4; ++q)
        if (!finite_(ego[q])) return E_INVAL;
    if (((uintptr_t)A_out & 15) != 0) return E_INVAL;           // one 16-byte store per row of A_out
    return 0;
}

// b of row r of one obstacle (A [E,2], b [E], v [2] or NULL) at stage kk
SC_FN double row_b(const double* A, const double* b, const double* v, double Ts, int r, int kk) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!v) return b[r];
    const double t = (double)kk * Ts;
    const double p0 = A[2 * r] * v[0];
    const double p1 = A[2 * r + 1] * v[1];
    const double dot = p0 + p1;
    const double shift = t * dot;
    return b[r] + shift;
}

// are the numbers of obstacle i (its E rows, its velocity) finite and every row a half-plane; Ts is the instance's and
// checked by the caller
SC_FN bool obstacle_finite(const double* A, const double* b, const double* v, int E) {
    bool ok = !v || (finite_(v[0]) && finite_(v[1]));
    for (int r = 0; r < E; ++r)
        ok = ok && finite_(A[2 * r]) && finite_(A[2 * r + 1]) && finite_(b[r]) && (A[2 * r] != 0.0 || A[2 * r + 1] != 0.0);
    return ok;
}

// may the instance be measured in accumulate mode (the rule of obca_plan_tighten)
SC_FN bool active(int variant, int status) { return variant != 0 && (status == 0 || status == 1); }

// This call's smallest signed distance between the car and one obstacle (A [E,2], b [E], v [2] or NULL) over the samples of
// x [3,N+1] and x0 [3] or NULL; +inf when no pose is finite, NaN when a distance is.  *n_pose: the number of finite sample
// poses (the same for every obstacle of the instance).  E is a compile-time constant so that the rows live in registers.
template <int E>
SC_FN double score_rows(const double* A, const double* b, const double* v, double Ts, const double* x, int N, const double* x0,
                        int n_sub, bool stage0, const double* ego, int* n_pose) {
    const int N1 = N + 1;
    double a[2 * E], b0[E], b1[E], bj[E], C[4][2];
    for (int r = 0; r < E; ++r) { a[2 * r] = A[2 * r]; a[2 * r + 1] = A[2 * r + 1]; b0[r] = row_b(A, b, v, Ts, r, 0); }
    double best = INFINITY;
    int np = 0;
    if (x0 && finite_(x0[0]) && finite_(x0[1]) && finite_(x0[2])) {
        audit::car_corners(x0[0], x0[1], x0[2], ego, C);
        best = audit::min_nan(best, audit::signed_distance<4>(C, a, b0, E));
        ++np;
    }
    for (int s = 0; s < N; ++s) {
        const double p0[3] = {x[s], x[N1 + s], x[2 * N1 + s]}, p1[3] = {x[s + 1], x[N1 + s + 1], x[2 * N1 + s + 1]};
        if (!stage0 && v)
            for (int r = 0; r < E; ++r) b1[r] = row_b(A, b, v, Ts, r, s + 1);
        else
            for (int r = 0; r < E; ++r) b1[r] = b0[r];
        for (int j = s == 0 ? 0 : 1; j <= n_sub; ++j) {
            double p[3];
            audit::sample_pose(p0, p1, n_sub, j, p);
            if (!(finite_(p[0]) && finite_(p[1]) && finite_(p[2]))) continue;
            for (int r = 0; r < E; ++r) bj[r] = audit::lerp_end(b0[r], b1[r], n_sub, j);
            audit::car_corners(p[0], p[1], p[2], ego, C);
            best = audit::min_nan(best, audit::signed_distance<4>(C, a, bj, E));
            ++np;
        }
        for (int r = 0; r < E; ++r) b0[r] = b1[r];
    }
    *n_pose = np;
    return best;
}

// the same for a run-time row count 1 <= E <= MAX_E
template <int E = 1>
SC_FN double score_obstacle(int e, const double* A, const double* b, const double* v, double Ts, const double* x, int N,
                            const double* x0, int n_sub, bool stage0, const double* ego, int* n_pose) {
    if constexpr (E < MAX_E) {
        if (e != E) return score_obstacle<E + 1>(e, A, b, v, Ts, x, N, x0, n_sub, stage0, ego, n_pose);
    }
    return score_rows<E>(A, b, v, Ts, x, N, x0, n_sub, stage0, ego, n_pose);
}

// the running minimum; an old score that is no number is replaced
SC_FN double score_min(double old, double cur) { return cur < old || old != old ? cur : old; }

// does score sj of obstacle j rank before score si of obstacle i
SC_FN bool beats(double sj, int j, double si, int i) { return sj < si || (sj == si && j < i); }

// rank of obstacle i among score [K]
SC_FN int rank_of(const double* score, int K, int i) {
    const double si = score[i];
    int n = 0;
    for (int j = 0; j < K; ++j) n += beats(score[j], j, si, i) ? 1 : 0;
    return n;
}

// is sel [n_sel] an ascending list of pool indices
SC_FN bool sel_valid(const int32_t* sel, int n_sel, int K) {
    bool ok = true;
    for (int s = 0; s < n_sel; ++s) ok = ok && sel[s] >= 0 && sel[s] < K && (s == 0 || sel[s] > sel[s - 1]);
    return ok;
}

// output row q = slot E + r of stage kk for pool obstacle i = sel[slot] (usable), or the fill
SC_FN void out_row(const double* pool_A, const double* pool_b, const double* pool_v, double Ts, int E, int i, int r, int kk,
                   bool usable, double a[2], double* b) {
    if (!usable) { a[0] = 1.0; a[1] = 0.0; *b = FILL_B; return; }
    const double* Ai = pool_A + 2 * (int64_t)i * E;
    a[0] = Ai[2 * r]; a[1] = Ai[2 * r + 1];
    *b = row_b(Ai, pool_b + (int64_t)i * E, pool_v ? pool_v + 2 * i : nullptr, Ts, r, kk);
}

}  // namespace scene

#endif
