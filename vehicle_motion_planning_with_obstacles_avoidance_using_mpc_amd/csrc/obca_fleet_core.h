// obca_fleet_core.h -- the fleet closed loop: V cars that share one world (obca_fleet_step of include/obca_mpc.h).  Every
// closed loop over scene pools drives B rollouts through B private pools; here rollout b = g V + a is car a of world g, and
// the last V slots of every rollout's pool (K = Ks + V slots, E = 4) are "car j of my world".  The solve, the selection and the
// advance are calls that exist (obca_scene_select, obca_solve_batch, obca_pool_loop_advance); this is the step between two of
// them that lets the cars of a world see each other, as serial code:
//   measure   (measure == 1, n_sub > 0)  for every car that applied a step in this loop step (k[b] == step + 1): the smallest
//                                        signed distance to every other car of its world over the interval x_prev -> x0,
//                                        both cars moving; the history word, the flags FAILED / COLLISION, and for a car
//                                        flagged here the masked window of poolloop::prepare
//   agents    (always, afterwards)       slot Ks + j of every rollout of the world: the rectangle of car j where it stands
//                                        now, translating with its last applied speed along its heading -- or a spare
// The serial step() below is the specification; fleet_kernel of csrc/obca_fleet.hip (one workgroup per world, one wavefront
// per car, one lane per other car) calls the same pieces and must write the same words.
//
// Arithmetic.  car_rows rounds every product and sum on its own (FL_EXACT: the library is built with contraction on), so
// that a heading of 0 and dyadic numbers give the words of gridpool::box_rows on host and device alike; at other headings
// the two differ by the sin / cos of their maths libraries.  A -0.0 in A: sin(0) = +0.0 but its negation would be -0.0, and
// sin(-0.0) is -0.0.  Neither reaches A: c and s are taken as cos + 0.0 and sin + 0.0 (which turns -0.0 into +0.0 and
// changes no other number) and the negated normals as 0.0 - c and 0.0 - s (+0.0 for a zero).  The distances never see the
// sign of a zero; only a word-for-word comparison does.  pair_clear is audit::car_corners and audit::plan_distance as the
// library builds them (contracted), as obca_plan_clearance and obca_scene_select measure.
//
// What is not there is not measured: a pair of which one pose word (before or after the step) is not finite counts +inf,
// exactly as such a car is a spare slot for the others.  A distance that is itself no number (overflow) is NaN and ends the
// car FAILED.  Nothing written is ever NaN.
#ifndef OBCA_FLEET_CORE_H
#define OBCA_FLEET_CORE_H

#include <math.h>
#include <stdint.h>
#include "../../include/obca_mpc.h"
#include "obca_audit_core.h"
#include "obca_loop_core.h"
#include "obca_gridpool_core.h"

#if defined(__HIPCC__)
#define FL_FN __host__ __device__ inline
#else
#define FL_FN inline
#endif

#if defined(__clang__)
#define FL_EXACT _Pragma("clang fp contract(off)")
#else
#define FL_EXACT /* g++: built with -ffp-contract=off */
#endif

namespace fleet {

constexpr int MAX_V = 16;                  // one wavefront per car: 1024 threads
constexpr int MAX_K = 64;                  // scene::MAX_K
constexpr int E = 4;                       // rows of a car
constexpr int MAX_N = 127;                 // scene::MAX_N
constexpr int MAX_STEPS = 1024;            // poolloop::MAX_STEPS
constexpr int MAX_SUB = 256;               // scene::MAX_SUB
constexpr int E_INVAL = -22;               // OBCA_E_INVAL

FL_FN bool finite_(double v) { return v - v == 0.0; }          // false for NaN and +-inf, no libm call
FL_FN bool pose_finite(const double* p) { return finite_(p[0]) && finite_(p[1]) && finite_(p[2]); }

// obca_fleet_init's words
inline void init(obca_fleet* d) { loop::init_common(d); d->clearance = loop::NEVER_STOP; d->far = loop::DEFAULT_FAR; }

// the checks of obca_fleet_step, made before anything is read or written (the host build makes the same ones)
FL_FN int args_check(const obca_fleet* d, int32_t measure) {
    if (!d || d->struct_size != (uint32_t)sizeof(obca_fleet)) return E_INVAL;
    if (d->G < 1 || d->V < 1 || d->V > MAX_V || d->Ks < 0 || d->Ks + d->V > MAX_K || d->N < 1 || d->N > MAX_N) return E_INVAL;
    if (d->max_steps < 1 || d->max_steps > MAX_STEPS || d->step < 0 || d->step >= d->max_steps) return E_INVAL;
    if (d->n_sub < 0 || d->n_sub > MAX_SUB) return E_INVAL;
    if (measure != 0 && measure != 1) return E_INVAL;
    if (d->see != OBCA_FLEET_SEE_ALL && d->see != OBCA_FLEET_SEE_LOWER) return E_INVAL;
    if (d->predict != OBCA_FLEET_PREDICT_VELOCITY && d->predict != OBCA_FLEET_PREDICT_STATIC) return E_INVAL;
    if (!finite_(d->clearance) || !finite_(d->margin) || !(d->margin >= 0.0) || !finite_(d->far) || !(d->far > 0.0)) return E_INVAL;
    for (int q = 0; q < 4; ++q)
        if (!finite_(d->ego[q])) return E_INVAL;
    if (!d->x_prev || !d->x0 || !d->u0 || !d->k || !d->flags || !d->pool_A || !d->pool_b || !d->pool_v) return E_INVAL;
    if (!d->agent_clear_hist || !d->xref_out || !d->variant_out) return E_INVAL;
    return 0;
}

// the four rows of the car rectangle at pose (x, y, th), grown by margin on every side: audit::car_corners' rectangle in
// gridpool::box_rows' row order (top, front, bottom, rear for a car that looks along +x)
FL_FN void car_rows(double x, double y, double th, const double* ego, double margin, double* A, double* b) {
    FL_EXACT
    const double L = ego[0] + ego[2], W = ego[1] + ego[3];
    const double hl = L / 2, hw = W / 2;
    const double off = hl - ego[2];
    const double c = cos(th) + 0.0, s = sin(th) + 0.0;
    const double ox = off * c, oy = off * s;
    const double cx = x + ox, cy = y + oy;
    const double nc = 0.0 - c, ns = 0.0 - s;
    const double nx[4] = {ns, c, s, nc}, ny[4] = {c, s, nc, ns};
    const double half[4] = {hw, hl, hw, hl};
    for (int r = 0; r < 4; ++r) {
        const double p0 = nx[r] * cx;
        const double p1 = ny[r] * cy;
        const double dot = p0 + p1;
        const double e = dot + half[r];
        A[2 * r] = nx[r];
        A[2 * r + 1] = ny[r];
        b[r] = e + margin;
    }
}

// the speed other cars assume of a car: its last applied one while it runs, 0 once it has ended (it is parked where it
// stands) or under a static prediction; never a word that is not finite
FL_FN double agent_speed(int predict, int flag, double u_speed) {
    return (predict == OBCA_FLEET_PREDICT_VELOCITY && flag == OBCA_RUN) ? loop::finite_or_zero(u_speed) : 0.0;
}

// is slot Ks + j of car a's pool a spare
FL_FN bool agent_spare(int see, int a, int j, const double* pose_j) {
    return j == a || (see == OBCA_FLEET_SEE_LOWER && j > a) || !pose_finite(pose_j);
}

// slot Ks + j of car a: rows A [4,2], b [4] and velocity v [2], from car j's pose, flag and last input
FL_FN void agent_slot(const obca_fleet& d, int a, int j, const double* pose_j, int flag_j, double u_speed_j, double* A, double* b,
                      double* v) {
    FL_EXACT
    if (agent_spare(d.see, a, j, pose_j)) {
        gridpool::spare_rows(d.far, A, b);
        v[0] = 0.0; v[1] = 0.0;
        return;
    }
    car_rows(pose_j[0], pose_j[1], pose_j[2], d.ego, d.margin, A, b);
    const double sp = agent_speed(d.predict, flag_j, u_speed_j);
    const double c = cos(pose_j[2]) + 0.0, s = sin(pose_j[2]) + 0.0;
    v[0] = sp * c;
    v[1] = sp * s;
}

// the smallest signed distance between car i (as the footprint) and car j (as rows, no margin) over the n_sub + 1 samples of
// the interval, both poses interpolated linearly (audit::sample_pose); i < j by convention, so that both cars of a pair
// read one word.  +inf when a pose word is not finite (the pair is not measured), NaN when a distance is no number.
FL_FN double pair_clear(const double* pi0, const double* pi1, const double* pj0, const double* pj1, const double* ego, int n_sub) {
    if (!(pose_finite(pi0) && pose_finite(pi1) && pose_finite(pj0) && pose_finite(pj1))) return INFINITY;
    double best = INFINITY;
    for (int s = 0; s <= n_sub; ++s) {
        double p[3], q[3], C[4][2], A[8], b[4];
        audit::sample_pose(pi0, pi1, n_sub, s, p);
        audit::sample_pose(pj0, pj1, n_sub, s, q);
        audit::car_corners(p[0], p[1], p[2], ego, C);
        car_rows(q[0], q[1], q[2], ego, 0.0, A, b);
        best = audit::min_nan(best, audit::plan_distance<4>(C, A, b, 4));
    }
    return best;
}

// did rollout b apply a step in loop step `step`
FL_FN bool stepped(const obca_fleet& d, int64_t b) { return d.k[b] == d.step + 1; }

// the pose car b is measured from: where it was before the step if it stepped, else where it stands
FL_FN const double* pose_before(const obca_fleet& d, int64_t b) { return (stepped(d, b) ? d.x_prev : d.x0) + 3 * b; }

// the pair value of cars a and j of world g (a != j), the lower index as the footprint
FL_FN double pair_of(const obca_fleet& d, int64_t g, int a, int j) {
    const int lo = a < j ? a : j, hi = a < j ? j : a;
    const int64_t bl = g * d.V + lo, bh = g * d.V + hi;
    return pair_clear(pose_before(d, bl), d.x0 + 3 * bl, pose_before(d, bh), d.x0 + 3 * bh, d.ego, d.n_sub);
}

// the flag of a car that stepped after its fold c
FL_FN int flag_after(const obca_fleet& d, int flag, double c) {
    if (c != c) return OBCA_DONE_FAILED;
    if (flag == OBCA_RUN && c < d.clearance) return OBCA_DONE_COLLISION;
    return flag;
}

// ---- the serial definition: one call of obca_fleet_step for world g
inline void measure_world(const obca_fleet& d, int64_t g) {
    const int V = d.V, S = d.max_steps, N1 = d.N + 1;
    double fold[MAX_V];
    for (int a = 0; a < V; ++a) {                                   // every fold from the poses alone, before any flag changes
        fold[a] = INFINITY;
        if (!stepped(d, g * V + a)) continue;
        for (int j = 0; j < V; ++j)
            if (j != a) fold[a] = audit::min_nan(fold[a], pair_of(d, g, a, j));
    }
    for (int a = 0; a < V; ++a) {
        const int64_t b = g * V + a;
        if (!stepped(d, b)) continue;
        if (fold[a] == fold[a]) d.agent_clear_hist[b * S + d.step] = fold[a];
        const int was = d.flags[b], now = flag_after(d, was, fold[a]);
        if (now == was) continue;
        d.flags[b] = now;
        loop::mask_rollout(d.variant_out, d.xref_out, d.x0, b, N1);
    }
}

inline void write_agents(const obca_fleet& d, int64_t g) {
    const int V = d.V, K = d.Ks + d.V;
    for (int a = 0; a < V; ++a) {
        const int64_t b = g * V + a;
        for (int j = 0; j < V; ++j) {
            const int64_t bj = g * V + j, slot = b * K + d.Ks + j;
            agent_slot(d, a, j, d.x0 + 3 * bj, d.flags[bj], d.u0[2 * bj], d.pool_A + slot * E * 2, d.pool_b + slot * E,
                       d.pool_v + slot * 2);
        }
    }
}

inline void step(const obca_fleet& d, int32_t measure, int64_t g) {
    if (measure && d.n_sub > 0) measure_world(d, g);
    write_agents(d, g);
}

}  // namespace fleet

#endif
