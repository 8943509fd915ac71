// obca_poolloop_core.h -- the closed loop over scene pools: what happens around one solve of one rollout whose world is a
// pool of up to 64 obstacles (obca_pool_loop_advance of include/obca_mpc.h).  The solve itself and the selection in front of
// it are calls that exist (obca_scene_select, obca_solve_batch); this is the harness between two of them, as serial code:
//   finish   (solved == 1, flag RUN)  record the step, read the solve, measure the applied interval against the WHOLE pool
//                                     (scene::score_obstacle on the two-knot plan [x0 p1] with Ts = ts_opt: the words
//                                     obca_scene_select measures), move the pool by ts_opt (scene::row_b at stage 1,
//                                     accumulated step by step), advance the state as rollout::finish does, set the flag
//                                     in the order COLLISION, CAP, GOAL
//   start    (solved == 0)            k = 0, u0 = 0, histories filled, flag FAILED / GOAL / RUN
//   prepare  (always, afterwards)     the reference window of rollout::prepare's H4 word for word, and the variant of the
//                                     next solve (0 for a rollout that is not RUN, whose window is its pose)
// The serial step() below is the specification; poolloop_kernel of csrc/obca_poolloop.hip (one wavefront per rollout, one
// lane per pool obstacle) calls the same pieces and must write the same words.  Contraction is off wherever a word is
// compared (PL_EXACT, as RO_EXACT / scene::row_b): the library is built with contraction on.  The one exception is the
// clearance: scene::score_obstacle is obca_scene_select's code, contracted in the library and on the device's sin / cos, so
// clear_hist is obca_scene_select's word on the device and the host build's word only where the arithmetic is exact
// (heading 0, axis-parallel rows, dyadic numbers); elsewhere the two agree as obca_scene_select's scores do, to ~1e-12 m.
//
// A failed step (status outside {0, 1}, a word of the applied knot, input or step length that is not finite, ts <= 0, a
// clearance that is no number) counts in no history but status, iters and sel: rollout::finish's rule.  Nothing written is
// ever NaN except the fill of x_closed beyond the driven knots; the window copies the words of the path it is given.
#ifndef OBCA_POOLLOOP_CORE_H
#define OBCA_POOLLOOP_CORE_H

#include <math.h>
#include <stdint.h>
#include "../../include/obca_mpc.h"
#include "obca_loop_core.h"
#include "obca_scene_core.h"

#if defined(__HIPCC__)
#define PL_FN __host__ __device__ inline
#else
#define PL_FN inline
#endif

#if defined(__clang__)
#define PL_EXACT _Pragma("clang fp contract(off)")
#else
#define PL_EXACT /* g++: built with -ffp-contract=off */
#endif

namespace poolloop {

constexpr int MAX_STEPS = 1024;
constexpr double WINDOW_FAR = 100000.0;       // rollout::prepare's H4: no point at or beyond this squared distance is taken

// obca_pool_loop_init's words
inline void init(obca_pool_loop* d) { loop::init_common(d); d->clearance = loop::NEVER_STOP; d->goal_tol2 = loop::DEFAULT_GOAL_TOL2; }

// the checks of obca_pool_loop_advance, made before anything is read or written (the host build makes the same ones)
PL_FN int args_check(const obca_pool_loop* d, int32_t solved) {
    if (!d || d->struct_size != (uint32_t)sizeof(obca_pool_loop)) return scene::E_INVAL;
    if (d->B < 1 || d->K < 1 || d->K > scene::MAX_K || d->E < 1 || d->E > scene::MAX_E || d->N < 1 || d->N > scene::MAX_N)
        return scene::E_INVAL;
    if (d->path_max < 1 || d->max_steps < 1 || d->max_steps > MAX_STEPS) return scene::E_INVAL;
    if (solved != 0 && solved != 1) return scene::E_INVAL;
    if (d->variant != 4 && d->variant != 6 && d->variant != 8) return scene::E_INVAL;
    if (d->n_sub < 0 || d->n_sub > scene::MAX_SUB || d->n_sel < 0 || d->n_sel > scene::MAX_SEL) return scene::E_INVAL;
    if (!scene::finite_(d->clearance) || !scene::finite_(d->goal_tol2) || !(d->goal_tol2 > 0.0)) return scene::E_INVAL;
    for (int q = 0; q < 4; ++q)
        if (!scene::finite_(d->ego[q])) return scene::E_INVAL;
    if (!d->pool_A || !d->goal || !d->path || !d->path_len) return scene::E_INVAL;
    if (!d->x0 || !d->u0 || !d->pool_b || !d->k || !d->flags) return scene::E_INVAL;
    if (!d->x_closed || !d->u_closed || !d->T_closed || !d->status_hist || !d->iters_hist || !d->clear_hist) return scene::E_INVAL;
    if (!d->xref_out || !d->variant_out) return scene::E_INVAL;
    if (d->n_sel >= 1 && !d->sel_hist) return scene::E_INVAL;
    if (solved == 1) {
        if (!d->status || !d->iters || !d->ts_opt || !d->xopt || !d->uopt) return scene::E_INVAL;
        if (d->n_sel >= 1 && !d->sel) return scene::E_INVAL;
    }
    return 0;
}

// squared distance of the car to one path point: the words of rollout::prepare's H4 and of rollout::at_goal
PL_FN double dist2(double px, double py, double qx, double qy) {
    PL_EXACT
    const double dx = px - qx, dy = py - qy;
    return dx * dx + dy * dy;
}

PL_FN bool at_goal(double px, double py, const double* goal, double goal_tol2) {
    return !(dist2(px, py, goal[0], goal[1]) >= goal_tol2);
}

// does candidate (dj, j) replace (di, i) when two first-strict-minima are combined: the smaller distance, ties to the
// lower index.  A search that found nothing holds (WINDOW_FAR, INT32_MAX) and never wins; NaN is never held.
PL_FN bool window_beats(double dj, int j, double di, int i) { return dj < di || (dj == di && j < i); }

// first strict minimum below WINDOW_FAR over points first, first + stride, ... < len of path [3,P]; *best_i stays INT32_MAX
// when there is none.  (first, stride) = (0, 1) is the serial loop of rollout::prepare.
PL_FN double window_search(const double* path, int P, int len, double px, double py, int first, int stride, int* best_i) {
    double best = WINDOW_FAR;
    int i0 = INT32_MAX;
    for (int i = first; i < len; i += stride) {
        const double d = dist2(px, py, path[i], path[P + i]);
        if (d < best) { best = d; i0 = i; }
    }
    *best_i = i0;
    return best;
}

// the path point column t of the window shows, the window starting at i0
PL_FN int window_point(int i0, int t, int len) { return (i0 + t < len - 1) ? i0 + t : len - 1; }

// is the solve one that cannot be applied
PL_FN bool solve_bad(int st, double p1x, double p1y, double p1t, double ux, double uy, double ts) {
    const bool fin = scene::finite_(p1x) && scene::finite_(p1y) && scene::finite_(p1t) && scene::finite_(ux) && scene::finite_(uy) &&
                     scene::finite_(ts);
    return !(st == 0 || st == 1) || !fin || !(ts > 0.0);
}

// the flag after an applied step kb (the state already advanced to p1); c is the interval's clearance
PL_FN int flag_after(const obca_pool_loop& d, int kb, double c, double p1x, double p1y, const double* goal) {
    if (d.n_sub > 0 && c < d.clearance) return OBCA_DONE_COLLISION;
    if (kb + 1 == d.max_steps) return OBCA_DONE_CAP;
    if (at_goal(p1x, p1y, goal, d.goal_tol2)) return OBCA_DONE_GOAL;
    return OBCA_RUN;
}

// the flag of a rollout at its start
PL_FN int flag_start(const obca_pool_loop& d, double px, double py, double pt, int len, const double* goal) {
    if (!(scene::finite_(px) && scene::finite_(py) && scene::finite_(pt)) || len < 1 || len > d.path_max) return OBCA_DONE_FAILED;
    return at_goal(px, py, goal, d.goal_tol2) ? OBCA_DONE_GOAL : OBCA_RUN;
}

// the path length used to form addresses: a RUN rollout has 1 <= path_len <= path_max since its start; a caller that broke
// that reads inside its own path all the same
PL_FN int safe_len(int len, int P) { return len < 1 ? 1 : (len > P ? P : len); }

// may step kb be written into histories of S steps (true for every RUN rollout since its start)
PL_FN bool step_in_range(int kb, int S) { return kb >= 0 && kb < S; }

// ---- the serial definition: one call of obca_pool_loop_advance for rollout b
inline void finish(const obca_pool_loop& d, int64_t b) {
    if (d.flags[b] != OBCA_RUN) return;
    const int S = d.max_steps, N = d.N, N1 = N + 1, K = d.K, E = d.E, kb = d.k[b];
    if (!step_in_range(kb, S)) { d.flags[b] = OBCA_DONE_FAILED; return; }      // a counter the caller broke: nothing is written
    d.status_hist[b * S + kb] = d.status[b];
    d.iters_hist[b * S + kb] = d.iters[b];
    for (int s = 0; s < d.n_sel; ++s) d.sel_hist[(b * S + kb) * d.n_sel + s] = d.sel[b * d.n_sel + s];
    const double* xo = d.xopt + b * 3 * N1;
    const double* uo = d.uopt + b * 2 * N;
    const double p1[3] = {xo[1], xo[N1 + 1], xo[2 * N1 + 1]}, u[2] = {uo[0], uo[N]}, ts = d.ts_opt[b];
    if (solve_bad(d.status[b], p1[0], p1[1], p1[2], u[0], u[1], ts)) { d.flags[b] = OBCA_DONE_FAILED; return; }
    const double* pA = d.pool_A + b * K * E * 2;
    double* pb = d.pool_b + b * K * E;
    const double* pv = d.pool_v ? d.pool_v + b * K * 2 : nullptr;
    double c = INFINITY;
    if (d.n_sub > 0) {
        const double* p0 = d.x0 + 3 * b;
        const double xx[6] = {p0[0], p1[0], p0[1], p1[1], p0[2], p1[2]};
        for (int i = 0; i < K; ++i) {
            int n_pose = 0;
            c = audit::min_nan(c, scene::score_obstacle(E, pA + 2 * i * E, pb + i * E, pv ? pv + 2 * i : nullptr, ts, xx, 1, nullptr,
                                                        d.n_sub, pv == nullptr, d.ego, &n_pose));
        }
        if (c != c) { d.flags[b] = OBCA_DONE_FAILED; return; }
        d.clear_hist[b * S + kb] = c;
    }
    if (pv)
        for (int i = 0; i < K; ++i)
            for (int r = 0; r < E; ++r) pb[i * E + r] = scene::row_b(pA + 2 * i * E, pb + i * E, pv + 2 * i, ts, r, 1);
    for (int j = 0; j < 3; ++j) {
        d.x0[3 * b + j] = p1[j];
        d.x_closed[(b * (S + 1) + kb + 1) * 3 + j] = p1[j];
    }
    for (int j = 0; j < 2; ++j) {
        d.u0[2 * b + j] = u[j];
        d.u_closed[(b * S + kb) * 2 + j] = u[j];
    }
    d.T_closed[b * S + kb] = ts;
    d.k[b] = kb + 1;
    d.flags[b] = flag_after(d, kb, c, p1[0], p1[1], d.goal + 2 * b);
}

inline void start(const obca_pool_loop& d, int64_t b) {
    const int S = d.max_steps;
    const double* p = d.x0 + 3 * b;
    d.k[b] = 0;
    d.u0[2 * b] = 0.0; d.u0[2 * b + 1] = 0.0;
    for (int j = 0; j < 3; ++j) d.x_closed[b * (S + 1) * 3 + j] = p[j];
    for (int q = 3; q < 3 * (S + 1); ++q) d.x_closed[b * (S + 1) * 3 + q] = NAN;
    for (int q = 0; q < 2 * S; ++q) d.u_closed[b * S * 2 + q] = 0.0;
    for (int q = 0; q < S; ++q) {
        d.T_closed[b * S + q] = 0.0;
        d.status_hist[b * S + q] = 0;
        d.iters_hist[b * S + q] = 0;
        d.clear_hist[b * S + q] = INFINITY;
    }
    for (int q = 0; q < S * d.n_sel; ++q) d.sel_hist[b * S * d.n_sel + q] = -1;
    d.flags[b] = flag_start(d, p[0], p[1], p[2], d.path_len[b], d.goal + 2 * b);
}

inline void prepare(const obca_pool_loop& d, int64_t b) {
    const int N1 = d.N + 1, P = d.path_max;
    const double* p = d.x0 + 3 * b;
    double* xr = d.xref_out + b * 3 * N1;
    if (d.flags[b] != OBCA_RUN) { loop::mask_rollout(d.variant_out, d.xref_out, d.x0, b, N1); return; }
    d.variant_out[b] = d.variant;
    const double* path = d.path + b * 3 * P;
    const int len = safe_len(d.path_len[b], P);
    int i0;
    window_search(path, P, len, p[0], p[1], 0, 1, &i0);
    if (i0 == INT32_MAX) i0 = 0;
    for (int t = 0; t < N1; ++t) {
        const int i = window_point(i0, t, len);
        for (int j = 0; j < 3; ++j) xr[j * N1 + t] = path[j * P + i];
    }
}

inline void step(const obca_pool_loop& d, int32_t solved, int64_t b) {
    if (solved) finish(d, b);
    else start(d, b);
    prepare(d, b);
}

}  // namespace poolloop

#endif
