// obca_pool_tracks_core.h -- the closed loop over scene pools, obstacles on timed tracks (obca_pool_tracks of
// include/obca_mpc.h).  A pool obstacle translates at pool_v (obca_pool_loop_advance) or is another car of a fleet
// (csrc/obca_fleet_core.h); here the last Kt slots of a rollout's pool follow timed pose sequences.  Rollout b reads track
// block b / group; track j of the block is pool slot K - Kt + j.  The step between two solves, as serial code:
//   measure   (measure == 1, n_sub > 0)  for a rollout that applied a step in this loop step (k[b] == step + 1): the smallest
//                                        signed distance to every usable track over the interval x_prev -> x0, the obstacle at
//                                        the TRACK's pose at every sample's time; the history word, the flags FAILED /
//                                        COLLISION, and for a car flagged here the masked window of poolloop::prepare
//   rows      (always, afterwards)       the pool slot (rows now, chord velocity), the rows at the N + 1 stage times of the
//                                        next solve, the mask word and the state word of every tracked slot -- or a spare
// The serial rollout() below is the specification; pool_tracks_kernel of csrc/obca_pool_tracks.hip (one wavefront per rollout)
// calls the same pieces and must write the same words.
//
// Arithmetic.  The times, the interpolation and the chord velocity round every product and sum on their own (FL_EXACT), the
// rows are fleet::car_rows, which does the same: heading 0 and dyadic numbers give the same words on host and device, other
// headings differ by the sin / cos of the two maths libraries.  The measurement is audit::lerp_end, audit::sample_pose,
// audit::car_corners and audit::plan_distance as the library builds them (contracted), as obca_fleet_step measures.
// A track that is not usable is never read beyond the check that says so.  Nothing written is ever NaN: a pose that is not
// finite (the difference of two knot words overflowed) gives the spare's rows, a velocity word that is not finite gives 0, a
// distance that is no number ends the car FAILED without a history word.
#ifndef OBCA_POOL_TRACKS_CORE_H
#define OBCA_POOL_TRACKS_CORE_H

#include "obca_fleet_core.h"

namespace ptracks {

constexpr int E = fleet::E;
constexpr int MAX_L = 4096;

// obca_pool_tracks_init's words
inline void init(struct obca_pool_tracks* d) { loop::init_common(d); d->clearance = loop::NEVER_STOP; d->far = loop::DEFAULT_FAR; }

// the checks of obca_pool_tracks, made before anything is read or written (the host build makes the same ones)
FL_FN int args_check(const struct obca_pool_tracks* d, int32_t measure) {
    if (!d || d->struct_size != (uint32_t)sizeof(struct obca_pool_tracks)) return fleet::E_INVAL;
    if (d->B < 1 || d->Kt < 1 || d->K < d->Kt || d->K > fleet::MAX_K || d->N < 1 || d->N > fleet::MAX_N) return fleet::E_INVAL;
    if (d->L < 1 || d->L > MAX_L || d->group < 1 || d->B % d->group != 0) return fleet::E_INVAL;
    if (d->max_steps < 1 || d->max_steps > fleet::MAX_STEPS || d->step < 0 || d->step >= d->max_steps) return fleet::E_INVAL;
    if (d->n_sub < 0 || d->n_sub > fleet::MAX_SUB) return fleet::E_INVAL;
    if (measure != 0 && measure != 1) return fleet::E_INVAL;
    if (d->predict != OBCA_TRACK_PREDICT_TRACK && d->predict != OBCA_TRACK_PREDICT_VELOCITY && d->predict != OBCA_TRACK_PREDICT_STATIC)
        return fleet::E_INVAL;
    if (!fleet::finite_(d->clearance) || !fleet::finite_(d->margin) || !(d->margin >= 0.0) || !fleet::finite_(d->far) || !(d->far > 0.0))
        return fleet::E_INVAL;
    for (int q = 0; q < 4; ++q)
        if (!fleet::finite_(d->ego[q])) return fleet::E_INVAL;
    if (!d->track_x || !d->track_t || !d->track_len || !d->track_size || !d->Ts || !d->x_prev || !d->x0 || !d->k) return fleet::E_INVAL;
    if (!d->flags || !d->pool_A || !d->pool_b || !d->pool_v || !d->stage_A || !d->stage_b || !d->stage_ok || !d->track_state)
        return fleet::E_INVAL;
    if (!d->track_clear_hist || !d->xref_out || !d->variant_out) return fleet::E_INVAL;
    return 0;
}

// one track of a block: its knots, its length word and its rectangle
struct Track {
    const double* x;                   // [L,3]
    const double* t;                   // [L]
    const double* size;                // [4]
    int len;
};

FL_FN Track track_of(const struct obca_pool_tracks& d, int64_t b, int j) {
    const int64_t q = (b / d.group) * d.Kt + j;
    Track T;
    T.x = d.track_x + q * d.L * 3;
    T.t = d.track_t + q * d.L;
    T.size = d.track_size + q * 4;
    T.len = d.track_len[q];
    return T;
}

// the clock of rollout b: its step and its offset
FL_FN double t0_of(const struct obca_pool_tracks& d, int64_t b) { return d.t0 ? d.t0[b] : 0.0; }
FL_FN bool clock_usable(const struct obca_pool_tracks& d, int64_t b) {
    return fleet::finite_(d.Ts[b]) && d.Ts[b] > 0.0 && fleet::finite_(t0_of(d, b));
}

// the time of stage kk of the next solve of rollout b: one product, one sum
FL_FN double stage_time(const struct obca_pool_tracks& d, int64_t b, int kk) {
    FL_EXACT
    const double steps = (double)(d.k[b] + kk);
    const double dt = steps * d.Ts[b];
    return t0_of(d, b) + dt;
}

// everything about a track but its knots: the length word is in range and the rectangle is one
FL_FN bool frame_usable(const Track& T, int L) {
    FL_EXACT
    bool ok = T.len >= 1 && T.len <= L;
    for (int q = 0; q < 4; ++q) ok = ok && fleet::finite_(T.size[q]);
    const double length = T.size[0] + T.size[2], width = T.size[1] + T.size[3];
    return ok && fleet::finite_(length) && fleet::finite_(width) && length > 0.0 && width > 0.0;
}

// knot i < len of a track whose frame is usable: its words are finite and its time is below the next knot's
FL_FN bool knot_usable(const Track& T, int i) {
    bool ok = fleet::pose_finite(T.x + 3 * i) && fleet::finite_(T.t[i]);
    if (i + 1 < T.len) ok = ok && T.t[i] < T.t[i + 1];
    return ok;
}

// the state word from its three parts
FL_FN int state_word(int len, bool frame, bool knots, bool clock) { return len == 0 ? 0 : ((frame && knots && clock) ? 1 : -1); }

// the state word of track T for rollout b, serially
FL_FN int track_state(const struct obca_pool_tracks& d, int64_t b, const Track& T) {
    const bool frame = frame_usable(T, d.L);
    bool knots = frame;
    for (int i = 0; knots && i < T.len; ++i) knots = knot_usable(T, i);
    return state_word(T.len, frame, knots, clock_usable(d, b));
}

// the pose of a usable track at time t
FL_FN void pose_at(const Track& T, double t, double* p) {
    FL_EXACT
    const int last = T.len - 1;
    int i = -1;                                                       // the knot whose words are the answer, if one is
    if (last == 0 || !(t > T.t[0])) i = 0;
    else if (t >= T.t[last]) i = last;
    if (i < 0) {
        int lo = 0, hi = last;                                        // t_lo <= t < t_hi
        while (hi - lo > 1) {
            const int mid = (lo + hi) / 2;
            if (T.t[mid] <= t) lo = mid; else hi = mid;
        }
        if (t == T.t[lo]) i = lo;
        else {
            const double num = t - T.t[lo];
            const double den = T.t[hi] - T.t[lo];
            const double a = num / den;
            for (int q = 0; q < 3; ++q) {
                const double w0 = T.x[3 * lo + q];
                const double dw = T.x[3 * hi + q] - w0;
                const double step = a * dw;
                p[q] = w0 + step;
            }
            return;
        }
    }
    p[0] = T.x[3 * i]; p[1] = T.x[3 * i + 1]; p[2] = T.x[3 * i + 2];
}

// the four rows of the tracked rectangle at pose p, grown by margin -- or the spare's, for a slot that is one and for a pose
// that is not finite
FL_FN void rows_at(const struct obca_pool_tracks& d, bool usable, const Track& T, const double* p, double* A, double* b) {
    if (usable && fleet::pose_finite(p)) fleet::car_rows(p[0], p[1], p[2], T.size, d.margin, A, b);
    else gridpool::spare_rows(d.far, A, b);
}

// stage kk of tracked slot j of rollout b: A [4,2], b [4]; p receives the pose (untouched for a spare)
FL_FN void stage_rows(const struct obca_pool_tracks& d, int64_t b, bool usable, const Track& T, int kk, double* p, double* A, double* bb) {
    if (usable) pose_at(T, stage_time(d, b, kk), p);
    rows_at(d, usable, T, p, A, bb);
}

// the velocity of the pool slot: the chord from stage 0's pose p0 to stage 1's p1 over the step
FL_FN void chord_velocity(const struct obca_pool_tracks& d, int64_t b, bool usable, const double* p0, const double* p1, double* v) {
    FL_EXACT
    v[0] = 0.0; v[1] = 0.0;
    if (!usable || d.predict == OBCA_TRACK_PREDICT_STATIC || !fleet::pose_finite(p0)) return;
    const double dx = p1[0] - p0[0], dy = p1[1] - p0[1];
    v[0] = loop::finite_or_zero(dx / d.Ts[b]);
    v[1] = loop::finite_or_zero(dy / d.Ts[b]);
}

FL_FN int ok_word(const struct obca_pool_tracks& d, bool usable) { return (usable && d.predict == OBCA_TRACK_PREDICT_TRACK) ? 1 : 0; }

// did rollout b apply a step in loop step `step`, and is that measured
FL_FN bool measured(const struct obca_pool_tracks& d, int32_t measure, int64_t b) {
    return measure != 0 && d.n_sub > 0 && d.k[b] == d.step + 1;
}

// can the car of rollout b be measured: +inf for every sample otherwise (obca_fleet_step's rule for a pose that is not there)
FL_FN bool car_there(const struct obca_pool_tracks& d, int64_t b) {
    return fleet::pose_finite(d.x_prev + 3 * b) && fleet::pose_finite(d.x0 + 3 * b);
}

// sample s of the interval rollout b has just driven against usable track T: the car's footprint between x_prev and x0, the
// obstacle's margin-free rows at the track's pose at the sample's time
FL_FN double sample_clear(const struct obca_pool_tracks& d, int64_t b, const Track& T, int s) {
    const double t_prev = stage_time(d, b, -1), t_now = stage_time(d, b, 0);
    double p[3], q[3], C[4][2], A[8], bb[4];
    audit::sample_pose(d.x_prev + 3 * b, d.x0 + 3 * b, d.n_sub, s, p);
    pose_at(T, audit::lerp_end(t_prev, t_now, d.n_sub, s), q);
    audit::car_corners(p[0], p[1], p[2], d.ego, C);
    fleet::car_rows(q[0], q[1], q[2], T.size, 0.0, A, bb);
    return audit::plan_distance<4>(C, A, bb, 4);
}

// the flag of a car that stepped after its fold c (obca_fleet_step's)
FL_FN int flag_after(const struct obca_pool_tracks& d, int flag, double c) {
    if (c != c) return OBCA_DONE_FAILED;
    if (flag == OBCA_RUN && c < d.clearance) return OBCA_DONE_COLLISION;
    return flag;
}

// ---- the serial definition: one call of obca_pool_tracks for rollout b
inline void rollout(const struct obca_pool_tracks& d, int32_t measure, int64_t b) {
    const int Kt = d.Kt, N1 = d.N + 1, S = d.max_steps;
    int state[fleet::MAX_K];
    for (int j = 0; j < Kt; ++j) state[j] = track_state(d, b, track_of(d, b, j));
    if (measured(d, measure, b)) {
        double fold = INFINITY;
        if (car_there(d, b))
            for (int j = 0; j < Kt; ++j) {
                if (state[j] != 1) continue;
                const Track T = track_of(d, b, j);
                for (int s = 0; s <= d.n_sub; ++s) fold = audit::min_nan(fold, sample_clear(d, b, T, s));
            }
        if (fold == fold) d.track_clear_hist[b * S + d.step] = fold;
        const int was = d.flags[b], now = flag_after(d, was, fold);
        if (now != was) {
            d.flags[b] = now;
            loop::mask_rollout(d.variant_out, d.xref_out, d.x0, b, N1);
        }
    }
    for (int j = 0; j < Kt; ++j) {
        const Track T = track_of(d, b, j);
        const bool usable = state[j] == 1;
        const int64_t slot = b * d.K + (d.K - Kt) + j, sj = b * Kt + j;
        double p0[3] = {0.0, 0.0, 0.0}, p1[3] = {0.0, 0.0, 0.0};
        for (int kk = 0; kk < N1; ++kk) {
            double* p = kk == 0 ? p0 : p1;
            stage_rows(d, b, usable, T, kk, p, d.stage_A + (sj * N1 + kk) * E * 2, d.stage_b + (sj * N1 + kk) * E);
            if (kk == 0) rows_at(d, usable, T, p0, d.pool_A + slot * E * 2, d.pool_b + slot * E);
            if (kk == 1) chord_velocity(d, b, usable, p0, p1, d.pool_v + slot * 2);
        }
        d.stage_ok[sj] = ok_word(d, usable);
        d.track_state[sj] = state[j];
    }
}

}  // namespace ptracks

#endif
