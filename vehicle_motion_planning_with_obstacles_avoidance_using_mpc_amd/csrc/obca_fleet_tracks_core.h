// obca_fleet_tracks_core.h -- the fleet closed loop, prediction by plans (obca_fleet_tracks of include/obca_mpc.h).
// obca_fleet_step (csrc/obca_fleet_core.h) makes another car a rectangle that translates at its last speed; here the plan that
// car has just solved becomes rows per stage -- a track -- which obca_scene_select_staged reads in place of the pool slot.
// Rollout q = g V + j is car j of world g.  The next solve starts one step later than the plan, so its stage kk is knot
// kk + 1 of the plan; stage N, for which the plan has no knot, continues the last interval's displacement at the heading of
// knot N.  One track per car per world, shared by its observers; what observer a may use of car j is a mask word.
// The serial world() below is the specification; tracks_kernel of csrc/obca_fleet_tracks.hip calls the same pieces and must
// write the same words.
//
// Arithmetic.  The rows are fleet::car_rows (every product and sum rounded on its own), the extrapolation is FL_EXACT too:
// heading 0 and dyadic numbers give the same words on host and device, other headings differ by the sin / cos of the two
// maths libraries.  obca_pool_loop_advance copied knot 1 to x0, so stage 0 of a usable plan holds the words obca_fleet_step
// writes into the pool slot of that car.  A car without a usable plan gets its rows at x0 at every stage, or the spare's
// where it has no pose; its mask words are 0, so nobody reads them as a plan.
#ifndef OBCA_FLEET_TRACKS_CORE_H
#define OBCA_FLEET_TRACKS_CORE_H

#include "obca_fleet_core.h"

namespace tracks {

constexpr int E = fleet::E;

// obca_fleet_tracks_init's words
inline void init(struct obca_fleet_tracks* d) { loop::init_common(d); d->far = loop::DEFAULT_FAR; }

// the checks of obca_fleet_tracks, made before anything is read or written (the host build makes the same ones)
FL_FN int args_check(const struct obca_fleet_tracks* d) {
    if (!d || d->struct_size != (uint32_t)sizeof(struct obca_fleet_tracks)) return fleet::E_INVAL;
    if (d->G < 1 || d->V < 1 || d->V > fleet::MAX_V || d->N < 1 || d->N > fleet::MAX_N || d->step < 0) return fleet::E_INVAL;
    if (d->see != OBCA_FLEET_SEE_ALL && d->see != OBCA_FLEET_SEE_LOWER) return fleet::E_INVAL;
    if (!fleet::finite_(d->margin) || !(d->margin >= 0.0) || !fleet::finite_(d->far) || !(d->far > 0.0)) return fleet::E_INVAL;
    for (int q = 0; q < 4; ++q)
        if (!fleet::finite_(d->ego[q])) return fleet::E_INVAL;
    if (!d->x0 || !d->flags || !d->k || !d->xopt || !d->status || !d->track_A || !d->track_b || !d->track_ok) return fleet::E_INVAL;
    return 0;
}

// everything about the plan of rollout q but its words: the car runs, applied this loop step, and the solve is feasible
FL_FN bool plan_applied(const struct obca_fleet_tracks& d, int64_t q) {
    return d.flags[q] == OBCA_RUN && d.k[q] == d.step + 1 && (d.status[q] == 0 || d.status[q] == 1);
}

// is the plan of rollout q usable
FL_FN bool plan_usable(const struct obca_fleet_tracks& d, int64_t q) {
    bool ok = plan_applied(d, q);
    const double* xo = d.xopt + q * 3 * (d.N + 1);
    for (int w = 0; w < 3 * (d.N + 1); ++w) ok = ok && fleet::finite_(xo[w]);
    return ok;
}

// the pose of stage kk of the next solve from the plan xo [3,N+1]
FL_FN void stage_pose(const double* xo, int N, int kk, double* p) {
    FL_EXACT
    const int N1 = N + 1;
    if (kk < N) { p[0] = xo[kk + 1]; p[1] = xo[N1 + kk + 1]; p[2] = xo[2 * N1 + kk + 1]; return; }
    const double dx = xo[N] - xo[N - 1];
    const double dy = xo[N1 + N] - xo[N1 + N - 1];
    p[0] = xo[N] + dx;
    p[1] = xo[N1 + N] + dy;
    p[2] = xo[2 * N1 + N];
}

// stage kk of the track of car j of world g: A [4,2], b [4]
FL_FN void track_rows(const struct obca_fleet_tracks& d, int64_t q, bool usable, int kk, double* A, double* b) {
    if (usable) {
        double p[3];
        stage_pose(d.xopt + q * 3 * (d.N + 1), d.N, kk, p);
        fleet::car_rows(p[0], p[1], p[2], d.ego, d.margin, A, b);
    } else if (fleet::pose_finite(d.x0 + 3 * q)) {
        fleet::car_rows(d.x0[3 * q], d.x0[3 * q + 1], d.x0[3 * q + 2], d.ego, d.margin, A, b);
    } else {
        gridpool::spare_rows(d.far, A, b);
    }
}

// what observer a may use of car j of its world
FL_FN int mask_word(const struct obca_fleet_tracks& d, int64_t g, int a, int j, bool usable_j) {
    return (usable_j && !fleet::agent_spare(d.see, a, j, d.x0 + 3 * (g * d.V + j))) ? 1 : 0;
}

// ---- the serial definition: one call of obca_fleet_tracks for world g
inline void world(const struct obca_fleet_tracks& d, int64_t g) {
    const int V = d.V, N1 = d.N + 1;
    bool use[fleet::MAX_V];
    for (int j = 0; j < V; ++j) {
        const int64_t q = g * V + j;
        use[j] = plan_usable(d, q);
        for (int kk = 0; kk < N1; ++kk) track_rows(d, q, use[j], kk, d.track_A + (q * N1 + kk) * E * 2, d.track_b + (q * N1 + kk) * E);
    }
    for (int a = 0; a < V; ++a)
        for (int j = 0; j < V; ++j) d.track_ok[(g * V + a) * V + j] = mask_word(d, g, a, j, use[j]);
}

}  // namespace tracks

#endif
