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

// ---- obca_scene_select_staged: the last Kt pool slots may carry rows of their own per stage (a track), where stage_ok says
// so.  Slot K - Kt + t of instance b reads stage_A / stage_b[b / stage_group, t, kk]; its pool_v plays no part in its rows
// (its pool words are still checked).  Every other slot is obca_scene_select's.

// the extra checks of obca_scene_select_staged, made with args_check before anything is read or written
SC_FN int staged_args_check(int32_t B, int32_t K, int32_t Kt, int32_t stage_group, const double* stage_A, const double* stage_b,
                            const int32_t* stage_ok) {
    if (Kt < 0 || Kt > K || stage_group < 1 || B < 1 || B % stage_group != 0) return E_INVAL;
    if (Kt > 0 && (!stage_A || !stage_b || !stage_ok)) return E_INVAL;
    return 0;
}

// the track of staged slot t of block blk: sA [N+1,E,2], sb [N+1,E]
SC_FN const double* track_A_of(const double* stage_A, int64_t blk, int Kt, int t, int N1, int E) {
    return stage_A + ((blk * Kt + t) * N1) * E * 2;
}
SC_FN const double* track_b_of(const double* stage_b, int64_t blk, int Kt, int t, int N1, int E) {
    return stage_b + ((blk * Kt + t) * N1) * E;
}

// is every word of a track finite and every row of every stage a half-plane
SC_FN bool track_finite(const double* sA, const double* sb, int N1, int E) {
    bool ok = true;
    for (int q = 0; q < N1 * E; ++q)
        ok = ok && finite_(sA[2 * q]) && finite_(sA[2 * q + 1]) && finite_(sb[q]) && (sA[2 * q] != 0.0 || sA[2 * q + 1] != 0.0);
    return ok;
}

// score_rows for a track: the samples are the same; at sample j of interval s the rows are A and b interpolated entry by
// entry between stages s and s + 1 (audit::lerp_end, obca_plan_sweep's rule for rows per stage), stage 0's at every sample
// for variant 4.  A track whose A does not change gives score_rows' words: lerp_end of two equal words is that word.
template <int E>
SC_FN double score_track(const double* sA, const double* sb, const double* x, int N, const double* x0, int n_sub, bool stage0,
                         const double* ego, int* n_pose) {
    const int N1 = N + 1;
    double a0[2 * E], a1[2 * E], aj[2 * E], b0[E], b1[E], bj[E], C[4][2];
    for (int r = 0; r < E; ++r) { a0[2 * r] = sA[2 * r]; a0[2 * r + 1] = sA[2 * r + 1]; b0[r] = sb[r]; }
    double best = INFINITY;
    int np = 0;
    if (x0 && finite_(x0[0]) && finite_(x0[1]) && finite_(x0[2])) {
        audit::car_corners(x0[0], x0[1], x0[2], ego, C);
        best = audit::min_nan(best, audit::signed_distance<4>(C, a0, b0, E));
        ++np;
    }
    for (int s = 0; s < N; ++s) {
        const double p0[3] = {x[s], x[N1 + s], x[2 * N1 + s]}, p1[3] = {x[s + 1], x[N1 + s + 1], x[2 * N1 + s + 1]};
        if (!stage0) {
            const double* nA = sA + 2 * (s + 1) * E;
            const double* nb = sb + (s + 1) * E;
            for (int r = 0; r < E; ++r) { a1[2 * r] = nA[2 * r]; a1[2 * r + 1] = nA[2 * r + 1]; b1[r] = nb[r]; }
        } else {
            for (int r = 0; r < E; ++r) { a1[2 * r] = a0[2 * r]; a1[2 * r + 1] = a0[2 * r + 1]; b1[r] = b0[r]; }
        }
        for (int j = s == 0 ? 0 : 1; j <= n_sub; ++j) {
            double p[3];
            audit::sample_pose(p0, p1, n_sub, j, p);
            if (!(finite_(p[0]) && finite_(p[1]) && finite_(p[2]))) continue;
            for (int r = 0; r < E; ++r) {
                aj[2 * r] = audit::lerp_end(a0[2 * r], a1[2 * r], n_sub, j);
                aj[2 * r + 1] = audit::lerp_end(a0[2 * r + 1], a1[2 * r + 1], n_sub, j);
                bj[r] = audit::lerp_end(b0[r], b1[r], n_sub, j);
            }
            audit::car_corners(p[0], p[1], p[2], ego, C);
            best = audit::min_nan(best, audit::signed_distance<4>(C, aj, bj, E));
            ++np;
        }
        for (int r = 0; r < E; ++r) { a0[2 * r] = a1[2 * r]; a0[2 * r + 1] = a1[2 * r + 1]; b0[r] = b1[r]; }
    }
    *n_pose = np;
    return best;
}

// the same for a run-time row count 1 <= E <= MAX_E
template <int E = 1>
SC_FN double score_track_obstacle(int e, const double* sA, const double* sb, const double* x, int N, const double* x0, int n_sub,
                                  bool stage0, const double* ego, int* n_pose) {
    if constexpr (E < MAX_E) {
        if (e != E) return score_track_obstacle<E + 1>(e, sA, sb, x, N, x0, n_sub, stage0, ego, n_pose);
    }
    return score_track<E>(sA, sb, x, N, x0, n_sub, stage0, ego, n_pose);
}

// staged slot index of pool obstacle i (0 .. Kt-1), or -1 where it has pool rows: i below K - Kt, or stage_ok 0
SC_FN int staged_slot(int i, int K, int Kt, const int32_t* ok /* [Kt] of the instance, or NULL */) {
    const int t = i - (K - Kt);
    return (ok && t >= 0 && ok[t] != 0) ? t : -1;
}

// out_row for a selected staged slot: stage kk's rows of the track as they are
SC_FN void out_row_track(const double* sA, const double* sb, int E, int r, int kk, double a[2], double* b) {
    const double* Ak = sA + 2 * (int64_t)kk * E;
    a[0] = Ak[2 * r]; a[1] = Ak[2 * r + 1];
    *b = sb[(int64_t)kk * E + r];
}

}  // namespace scene

#endif
