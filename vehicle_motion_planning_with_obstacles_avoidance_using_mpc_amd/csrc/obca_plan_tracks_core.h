// obca_plan_tracks_core.h -- open-loop plans measured against timed tracks themselves (obca_plan_tracks of include/obca_mpc.h).
// obca_pool_tracks (csrc/obca_pool_tracks_core.h) measures the one interval a closed loop has just driven; obca_scene_select_staged
// scores a plan against rows interpolated entry by entry between two stage times.  Here the N intervals of a plan are sampled as
// obca_scene_select samples them, and at every sample the obstacle is the track's own rectangle at the track's pose at the
// sample's time: across knots and turning.  Plan b reads track block b / group.  One plan, as serial code:
//   states    the state word of every track (ptracks' rule, the clock being dt[b] and t0[b]); written for every plan
//   measure   only a plan with variant[b] != 0 and status[b] 0 or 1 (NULL: every plan): for every usable track the smallest
//             distance over the samples -- x0 at knot 0's time where given, then the n_sub + 1 samples of every interval; a
//             sample whose car pose is not finite is skipped
//   outputs   track_clear[b,j] (+inf for a slot not in state 1), track_min[b] their fold, score[b,K-Kt+j] the running minimum --
//             or, for a plan that was not measured, has no finite sample pose or met a distance that is no number: NaN in
//             track_clear[b,:] and track_min[b], its score row untouched
// The serial plan() below is the specification; plan_tracks_kernel of csrc/obca_plan_tracks.hip (one wavefront per plan) calls
// the same pieces and must write the same words.
//
// Arithmetic.  Knot kk of plan b is at t0[b] + (double)kk dt[b], one product and one sum, each rounded on its own (FL_EXACT):
// the word ptracks::stage_time forms for stage kk with k = 0 and Ts = dt, so a plan's knot time and the time of the stage row
// it was solved against are one word.  The track's pose is ptracks::pose_at (FL_EXACT); the car's pose, the sample's time and
// the distance are audit::sample_pose, audit::lerp_end, audit::car_corners and audit::plan_distance<4> against
// fleet::car_rows(..., 0.0, ...) as the library builds them (contracted), as ptracks::sample_clear measures.
// A track that is not usable is never read beyond the check that says so; a length outside 1 .. L is never used as an index.
#ifndef OBCA_PLAN_TRACKS_CORE_H
#define OBCA_PLAN_TRACKS_CORE_H

#include "obca_pool_tracks_core.h"

namespace plantracks {

// obca_plan_tracks_init's words
inline void init(struct obca_plan_tracks* d) { loop::init_common(d); d->far = loop::DEFAULT_FAR; }

// the checks of obca_plan_tracks, made before anything is read or written (the host build makes the same ones)
FL_FN int args_check(const struct obca_plan_tracks* d) {
    if (!d || d->struct_size != (uint32_t)sizeof(struct obca_plan_tracks)) return fleet::E_INVAL;
    if (d->B < 1 || d->Kt < 1 || d->Kt > fleet::MAX_K || d->K < d->Kt || d->K > fleet::MAX_K || d->N < 1 || d->N > fleet::MAX_N)
        return fleet::E_INVAL;
    if (d->L < 1 || d->L > ptracks::MAX_L || d->group < 1 || d->B % d->group != 0) return fleet::E_INVAL;
    if (d->n_sub < 1 || d->n_sub > fleet::MAX_SUB) return fleet::E_INVAL;
    if (!fleet::finite_(d->far) || !(d->far > 0.0)) return fleet::E_INVAL;
    for (int q = 0; q < 4; ++q)
        if (!fleet::finite_(d->ego[q])) return fleet::E_INVAL;
    if (!d->track_x || !d->track_t || !d->track_len || !d->track_size || !d->dt || !d->x) return fleet::E_INVAL;
    if (!d->track_clear || !d->track_min || !d->track_state) return fleet::E_INVAL;
    return 0;
}

// track j of the block plan b reads
FL_FN ptracks::Track track_of(const struct obca_plan_tracks& d, int64_t b, int j) {
    const int64_t q = (b / d.group) * d.Kt + j;
    ptracks::Track T;
    T.x = d.track_x + q * d.L * 3;
    T.t = d.track_t + q * d.L;
    T.size = d.track_size + q * 4;
    T.len = d.track_len[q];
    return T;
}

// the clock of plan b: its step and its offset
FL_FN double t0_of(const struct obca_plan_tracks& d, int64_t b) { return d.t0 ? d.t0[b] : 0.0; }
FL_FN bool clock_usable(const struct obca_plan_tracks& d, int64_t b) {
    return fleet::finite_(d.dt[b]) && d.dt[b] > 0.0 && fleet::finite_(t0_of(d, b));
}

// the time of knot kk of plan b: one product, one sum (ptracks::stage_time's word for k = 0, Ts = dt)
FL_FN double knot_time(const struct obca_plan_tracks& d, int64_t b, int kk) {
    FL_EXACT
    const double steps = (double)kk;
    const double off = steps * d.dt[b];
    return t0_of(d, b) + off;
}

// the state word of track T for plan b, serially
FL_FN int track_state(const struct obca_plan_tracks& d, int64_t b, const ptracks::Track& T) {
    const bool frame = ptracks::frame_usable(T, d.L);
    bool knots = frame;
    for (int i = 0; knots && i < T.len; ++i) knots = ptracks::knot_usable(T, i);
    return ptracks::state_word(T.len, frame, knots, clock_usable(d, b));
}

// is plan b measured: obca_scene_select's accumulate rule
FL_FN bool measured(const struct obca_plan_tracks& d, int64_t b) {
    const int var = d.variant ? d.variant[b] : 6, st = d.status ? d.status[b] : 0;
    return var != 0 && (st == 0 || st == 1);
}

// the samples of a plan are numbered p = 0 .. n_samples - 1: p = s (n_sub + 1) + j is sample j of interval s, and where x0 is
// given p = N (n_sub + 1) is x0 at knot 0's time
FL_FN int n_samples(const struct obca_plan_tracks& d) { return d.N * (d.n_sub + 1) + (d.x0 ? 1 : 0); }

// the car's pose and the time of sample p of plan b; false where the pose is not finite (the sample is skipped)
FL_FN bool sample_of(const struct obca_plan_tracks& d, int64_t b, int p, double* pose, double* when) {
    const int ns1 = d.n_sub + 1, N1 = d.N + 1;
    const int s = p / ns1, j = p - s * ns1;
    if (s >= d.N) {
        pose[0] = d.x0[3 * b]; pose[1] = d.x0[3 * b + 1]; pose[2] = d.x0[3 * b + 2];
        *when = knot_time(d, b, 0);
    } else {
        const double* x = d.x + b * 3 * N1;
        const double p0[3] = {x[s], x[N1 + s], x[2 * N1 + s]}, p1[3] = {x[s + 1], x[N1 + s + 1], x[2 * N1 + s + 1]};
        audit::sample_pose(p0, p1, d.n_sub, j, pose);
        *when = audit::lerp_end(knot_time(d, b, s), knot_time(d, b, s + 1), d.n_sub, j);
    }
    return fleet::pose_finite(pose);
}

// sample p of plan b against usable track T: the car's footprint at the sample's pose, the obstacle's margin-free rows at the
// track's pose at the sample's time; +inf for a sample that is skipped
FL_FN double sample_clear(const struct obca_plan_tracks& d, int64_t b, const ptracks::Track& T, int p) {
    double pose[3], when, q[3], C[4][2], A[8], bb[4];
    if (!sample_of(d, b, p, pose, &when)) return INFINITY;
    ptracks::pose_at(T, when, q);
    audit::car_corners(pose[0], pose[1], pose[2], d.ego, C);
    fleet::car_rows(q[0], q[1], q[2], T.size, 0.0, A, bb);
    return audit::plan_distance<4>(C, A, bb, 4);
}

// the running minimum of a score word; an old score that is no number is replaced (scene::score_min)
FL_FN double score_fold(double old, double cur) { return cur < old || old != old ? cur : old; }

// ---- the serial definition: one call of obca_plan_tracks for plan b
inline void plan(const struct obca_plan_tracks& d, int64_t b) {
    const int Kt = d.Kt, np = n_samples(d);
    int state[fleet::MAX_K];
    double cur[fleet::MAX_K];
    for (int j = 0; j < Kt; ++j) d.track_state[b * Kt + j] = state[j] = track_state(d, b, track_of(d, b, j));
    bool ok = measured(d, b);
    double fold = INFINITY;
    if (ok) {
        int posed = 0;
        for (int p = 0; p < np; ++p) {
            double pose[3], when;
            posed += sample_of(d, b, p, pose, &when) ? 1 : 0;
        }
        ok = posed > 0;
    }
    if (ok)
        for (int j = 0; j < Kt; ++j) {
            cur[j] = INFINITY;
            if (state[j] != 1) continue;
            const ptracks::Track T = track_of(d, b, j);
            for (int p = 0; p < np; ++p) cur[j] = audit::min_nan(cur[j], sample_clear(d, b, T, p));
            fold = audit::min_nan(fold, cur[j]);
        }
    ok = ok && fold == fold;
    for (int j = 0; j < Kt; ++j) {
        d.track_clear[b * Kt + j] = ok ? cur[j] : NAN;
        if (ok && d.score && state[j] == 1) {
            double* sc = d.score + b * d.K + (d.K - Kt) + j;
            *sc = score_fold(*sc, cur[j]);
        }
    }
    d.track_min[b] = ok ? fold : NAN;
}

}  // namespace plantracks

#endif
