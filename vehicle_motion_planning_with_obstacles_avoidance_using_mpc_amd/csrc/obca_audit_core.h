// obca_audit_core.h -- collision audit geometry: signed distance from the car footprint to convex obstacles, and the
// sampled / certified clearance of one closed-loop interval.  Read-only: nothing here touches solver or rollout state.
//
// Compiles for the device (obca_audit.hip) and for the host (tests/native/audit_host.cpp).  The distance restates
// tests/kkt_check.py::polytope_distance branch by branch so that the two agree value for value:
//   m = 1            half-plane: the row gap (exact signed distance)
//   m = 2            wedge (an obstacle given by three vertices): the unbounded wedge cut off at reach 1e4 (_wedge_vertices)
//   m >= 3           polygon from consecutive rows (obstacle_H_Represent emits the rows in the order of the vertex list)
//   separated        exact Euclidean distance: smallest vertex-to-edge distance of car and obstacle, both ways
//   overlapping /    separating-axis value: the largest gap over the obstacle rows and the car's edge normals (<= 0).
//   touching         For two convex polygons this is minus the penetration depth (the minimum translation separating
//                    them lies along an edge normal of one of the two).
//   degenerate rows  (neighbouring rows parallel: no vertex): the largest row gap.  The test oracle solves a small QP
//                    there instead; the row gap is a lower bound of the distance when it is positive and the oracle's own
//                    value when it is not.  Neither the solver's obstacles nor obstacle_H_Represent of a proper polygon
//                    produce such rows.
//
// Moving rectangles are built with the harness's own rect_vertices / edge_row (obca_rollout_core.h), so the audit sees
// exactly the geometry the solver is handed.
//
// Certified bound between samples.  Along a linear interpolation of the pose (x, y, theta) every point of the car moves
// by at most |dp| + r_max |dtheta| (r_max = largest distance from the pose point to a footprint corner; a rotation by
// dtheta moves a point at radius r along a chord <= r |dtheta|), and a moving box by |dc|.  Both branches of the signed
// distance are 1-Lipschitz under such displacements: the Euclidean distance trivially, the penetration depth because a set
// that moves by at most delta stays inside the delta-dilation of where it was, and separating a delta-dilated set needs
// at most delta more translation.  At the switch (distance 0) both branches are 0, so the signed distance d is 1-Lipschitz,
// and so is the minimum over the obstacles.  On a sub-interval with end values d_j, d_j+1 and displacement bound delta,
// d(u) >= max(d_j - u delta, d_j+1 - (1 - u) delta) >= (d_j + d_j+1 - delta) / 2 for every fraction u.  A box that appears
// at the end knot is absent before it: d_j+1 can then only be smaller than the end value of the obstacles present
// throughout, so the bound stays valid for them, and the new box itself is covered by min(., d_j+1).
#ifndef OBCA_AUDIT_CORE_H
#define OBCA_AUDIT_CORE_H

#include <math.h>
#include <stdint.h>
#include "obca_rollout_core.h"

#if defined(__HIPCC__)
#define AU_FN __host__ __device__ inline
#else
#define AU_FN inline
#endif

namespace audit {

constexpr double WEDGE_REACH = 1e4;        // kkt_check._wedge_vertices
constexpr double DET_EPS = 1e-12;          // parallel neighbouring rows
constexpr double VIOL_TOL = 1e-6;          // first_violation: distance below dmin - VIOL_TOL

AU_FN double dmax(double a, double b) { return a > b ? a : b; }
AU_FN double dmin_(double a, double b) { return a < b ? a : b; }

// the four corners of the car rectangle (kkt_check.car_corners): centre p + R(theta)(off, 0), L = ego0 + ego2,
// W = ego1 + ego3, off = L/2 - ego2
AU_FN void car_corners(double x, double y, double th, const double* ego, double C[4][2]) {
    const double L = ego[0] + ego[2], W = ego[1] + ego[3];
    const double off = L / 2 - ego[2];
    const double c = cos(th), s = sin(th);
    const double cx = x + c * off, cy = y + s * off;
    const double hl = L / 2, hw = W / 2;
    C[0][0] = cx + c * hl - s * hw;    C[0][1] = cy + s * hl + c * hw;
    C[1][0] = cx + c * hl + s * hw;    C[1][1] = cy + s * hl - c * hw;
    C[2][0] = cx - c * hl + s * hw;    C[2][1] = cy - s * hl - c * hw;
    C[3][0] = cx - c * hl - s * hw;    C[3][1] = cy - s * hl + c * hw;
}

// largest distance from the pose point to a footprint corner
AU_FN double car_radius(const double* ego) {
    const double L = ego[0] + ego[2], W = ego[1] + ego[3];
    const double off = L / 2 - ego[2];
    const double ax = fabs(off) + L / 2, ay = W / 2;
    return sqrt(ax * ax + ay * ay);
}

AU_FN double seg_point_dist(double px, double py, double ax, double ay, double bx, double by) {
    const double abx = bx - ax, aby = by - ay;
    double t = ((px - ax) * abx + (py - ay) * aby) / dmax(abx * abx + aby * aby, 1e-300);
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double dx = px - (ax + t * abx), dy = py - (ay + t * aby);
    return sqrt(dx * dx + dy * dy);
}

// signed distance from the car C to {q : A q <= b} given by its m rows (A [m,2], b [m]); MAXM >= max(m, 4)
template <int MAXM>
AU_FN double signed_distance(const double C[4][2], const double* A, const double* b, int m) {
    static_assert(MAXM >= 4, "the wedge has four vertices");
    double gmax = -INFINITY;
    for (int j = 0; j < m; ++j) {
        const double a0 = A[2 * j], a1 = A[2 * j + 1];
        const double nrm = sqrt(a0 * a0 + a1 * a1);
        double mn = INFINITY;
        for (int v = 0; v < 4; ++v) mn = dmin_(mn, C[v][0] * a0 + C[v][1] * a1);
        gmax = dmax(gmax, (mn - b[j]) / nrm);
    }
    if (m == 1) return gmax;
    double V[MAXM][2];
    int nv;
    if (m == 2) {
        const double a1x = A[0], a1y = A[1], a2x = A[2], a2y = A[3];
        const double det = a1x * a2y - a1y * a2x;
        if (fabs(det) < DET_EPS) return gmax;
        const double px = (b[0] * a2y - a1y * b[1]) / det, py = (a1x * b[1] - b[0] * a2x) / det;
        const double n1 = sqrt(a1x * a1x + a1y * a1y), n2 = sqrt(a2x * a2x + a2y * a2y);
        double d1x = -a1y / n1, d1y = a1x / n1;                        // along line 1, into {a2 q <= b2}
        if (a2x * d1x + a2y * d1y > 0) { d1x = -d1x; d1y = -d1y; }
        double d2x = -a2y / n2, d2y = a2x / n2;                        // along line 2, into {a1 q <= b1}
        if (a1x * d2x + a1y * d2y > 0) { d2x = -d2x; d2y = -d2y; }
        V[0][0] = px;                              V[0][1] = py;
        V[1][0] = px + WEDGE_REACH * d1x;          V[1][1] = py + WEDGE_REACH * d1y;
        V[2][0] = px + WEDGE_REACH * (d1x + d2x);  V[2][1] = py + WEDGE_REACH * (d1y + d2y);
        V[3][0] = px + WEDGE_REACH * d2x;          V[3][1] = py + WEDGE_REACH * d2y;
        nv = 4;
    } else {
        for (int j = 0; j < m; ++j) {
            const int j1 = (j + 1 == m) ? 0 : j + 1;
            const double a1x = A[2 * j], a1y = A[2 * j + 1], a2x = A[2 * j1], a2y = A[2 * j1 + 1];
            const double det = a1x * a2y - a1y * a2x;
            if (fabs(det) < DET_EPS) return gmax;
            V[j][0] = (b[j] * a2y - a1y * b[j1]) / det;
            V[j][1] = (a1x * b[j1] - b[j] * a2x) / det;
        }
        nv = m;
    }
    // separating axes of the car as well
    double best = gmax;
    for (int i = 0; i < 4; ++i) {
        const int i1 = (i + 1) & 3;
        const double ex = C[i1][0] - C[i][0], ey = C[i1][1] - C[i][1];
        const double len = dmax(sqrt(ex * ex + ey * ey), 1e-300);
        double nx = ey / len, ny = -ex / len;
        double inside = -INFINITY;
        for (int v = 0; v < 4; ++v) inside = dmax(inside, (C[v][0] - C[i][0]) * nx + (C[v][1] - C[i][1]) * ny);
        if (inside > 1e-12) { nx = -nx; ny = -ny; }
        double mv = INFINITY;
        for (int v = 0; v < nv; ++v) mv = dmin_(mv, (V[v][0] - C[i][0]) * nx + (V[v][1] - C[i][1]) * ny);
        best = dmax(best, mv);
    }
    if (best <= 0.0) return best;                                      // overlapping (or touching)
    double dm = INFINITY;
    for (int v = 0; v < 4; ++v)
        for (int i = 0; i < nv; ++i) {
            const int i1 = (i + 1 == nv) ? 0 : i + 1;
            dm = dmin_(dm, seg_point_dist(C[v][0], C[v][1], V[i][0], V[i][1], V[i1][0], V[i1][1]));
        }
    for (int v = 0; v < nv; ++v)
        for (int i = 0; i < 4; ++i) {
            const int i1 = (i + 1) & 3;
            dm = dmin_(dm, seg_point_dist(V[v][0], V[v][1], C[i][0], C[i][1], C[i1][0], C[i1][1]));
        }
    return dm;
}

// (value, stage / step, obstacle) lexicographic, a NaN value below every number: ties (among NaNs as among equal values)
// to the lowest stage, then the lowest obstacle.  A total order on distinct (stage, obstacle), so any reduction order
// gives the same winner.
AU_FN bool better(double v, int s, int o, double v2, int s2, int o2) {
    const bool n = v != v, n2 = v2 != v2;
    if (n != n2) return n;
    return (n || v == v2) ? (s < s2 || (s == s2 && o < o2)) : v < v2;
}

// one (stage, obstacle) distance of the plan audit: NaN when a corner of the car, a row or the distance itself is not
// finite.  signed_distance's dmin_ / dmax drop a NaN operand, so a non-finite input must not reach it as a number: the
// audit never turns "unknown" into "safe".
template <int MAXM>
AU_FN double plan_distance(const double C[4][2], const double* A, const double* b, int m) {
    bool ok = true;
    for (int v = 0; v < 4; ++v) ok = ok && isfinite(C[v][0]) && isfinite(C[v][1]);
    for (int j = 0; j < m; ++j) ok = ok && isfinite(A[2 * j]) && isfinite(A[2 * j + 1]) && isfinite(b[j]);
    const double d = ok ? signed_distance<MAXM>(C, A, b, m) : NAN;
    return isfinite(d) ? d : NAN;
}

// a moving rectangle (centre, heading cos / sin, length, width) as the harness hands it to the solver: clockwise vertices
// (rect_vertices), one row per edge (edge_row)
AU_FN double box_distance(const double C[4][2], double cx, double cy, double c, double s, double length, double width) {
    double V[4][2], A[8], b[4];
    rollout::rect_vertices(cx, cy, c, s, length, width, V);
    rollout::edge_row(V[0][0], V[0][1], V[1][0], V[1][1], A, b);
    rollout::edge_row(V[1][0], V[1][1], V[2][0], V[2][1], A + 2, b + 1);
    rollout::edge_row(V[2][0], V[2][1], V[3][0], V[3][1], A + 4, b + 2);
    rollout::edge_row(V[3][0], V[3][1], V[0][0], V[0][1], A + 6, b + 3);
    return signed_distance<4>(C, A, b, 4);
}

// where a moving box is at knot s + 1 given its record at knot s (cx, cy, present): the harness's update_obstacle
// (obca_rollout_core.h prepare(): appear at k == t_start, afterwards advance by Ts_opt * v along the heading), with the
// step length T = T_closed[s] the harness inherits at step s + 1.  info = the 13-double tuple of the box.
AU_FN void box_next_knot(const double* info, double cx, double cy, int s_next, double T, double out[3]) {
    RO_EXACT
    if ((double)s_next < info[9]) { out[0] = cx; out[1] = cy; out[2] = 0.0; return; }
    if ((double)s_next > info[9]) {
        out[0] = cx + T * info[5] * info[11];
        out[1] = cy + T * info[5] * info[12];
    } else {
        out[0] = cx; out[1] = cy;
    }
    out[2] = 1.0;
}

// the obstacles of one rollout: static rows (n_static obstacles of m[i] rows) and nd moving boxes
struct Scene {
    const double* ego;
    int n_static;
    const int32_t* m;                  // [n_static]
    const double *As, *bs;             // [Ms,2], [Ms]
    int nd;
    const double* dyn;                 // [nd,13] tuples (heading cos / sin at 11, 12; length 3, width 4)
};

// Sample j (0..n_sub, both knots included) of one closed-loop interval: poses p0 -> p1 interpolated linearly in
// (x, y, theta), boxes b0 -> b1 (cx, cy, present at the two knots; a box present at both ends moves linearly, one present
// only at b1 counts at the end knot only).  n_sub == 0: the single knot p0 / b0.  Every function below evaluates sample j
// from the interval's ends alone, so that a serial loop over the samples and one lane per sample compute the same words.
AU_FN void sample_pose(const double* p0, const double* p1, int n_sub, int j, double p[3]) {
    const bool first = j == 0, last = j == n_sub;
    const double t = n_sub > 0 ? (double)j / (double)n_sub : 0.0;
    for (int q = 0; q < 3; ++q) p[q] = first ? p0[q] : (last ? p1[q] : p0[q] + t * (p1[q] - p0[q]));
}

AU_FN void sample_box(const double (*b0)[3], const double (*b1)[3], int n_sub, int j, int i, double* cx, double* cy, double* on) {
    const bool first = j == 0, last = j == n_sub;
    const double t = n_sub > 0 ? (double)j / (double)n_sub : 0.0;
    if (first) { *cx = b0[i][0]; *cy = b0[i][1]; *on = b0[i][2]; }
    else if (last) { *cx = b1[i][0]; *cy = b1[i][1]; *on = b1[i][2]; }
    else { *cx = b0[i][0] + t * (b1[i][0] - b0[i][0]); *cy = b0[i][1] + t * (b1[i][1] - b0[i][1]); *on = b0[i][2]; }
}

// smallest signed distance over the scene at sample j; arg = obstacle index (static first, then n_static + j; ties to the
// lowest)
template <int MAXM>
AU_FN double sample_distance(const Scene& S, const double* p0, const double* p1, const double (*b0)[3], const double (*b1)[3],
                             int n_sub, int j, int* arg) {
    double p[3], C[4][2];
    sample_pose(p0, p1, n_sub, j, p);
    car_corners(p[0], p[1], p[2], S.ego, C);
    double best = INFINITY;
    int ai = -1, off = 0;
    for (int i = 0; i < S.n_static; ++i) {
        const double d = signed_distance<MAXM>(C, S.As + 2 * off, S.bs + off, S.m[i]);
        off += S.m[i];
        if (d < best) { best = d; ai = i; }
    }
    for (int i = 0; i < S.nd && i < OBCA_MAX_DYN; ++i) {
        double cx, cy, on;
        sample_box(b0, b1, n_sub, j, i, &cx, &cy, &on);
        if (on == 0.0) continue;
        const double* info = S.dyn + (size_t)i * rollout::DYN_W;
        const double d = box_distance(C, cx, cy, info[11], info[12], info[3], info[4]);
        if (d < best) { best = d; ai = S.n_static + i; }
    }
    *arg = ai;
    return best;
}

// the certified bound of sub-interval j-1 -> j (j >= 1) from its end distances d_prev, d: the displacement bound delta of
// the car (|dp| + rmax |dtheta|) plus the largest move of a box present at both knots, then
// min((d_prev + d - delta) / 2, d_prev, d)
AU_FN double sub_bound(const Scene& S, const double* p0, const double* p1, const double (*b0)[3], const double (*b1)[3],
                       int n_sub, int j, double rmax, double d_prev, double d) {
    double p[3], pp[3];
    sample_pose(p0, p1, n_sub, j, p);
    sample_pose(p0, p1, n_sub, j - 1, pp);
    double dc = 0.0;
    for (int i = 0; i < S.nd && i < OBCA_MAX_DYN; ++i) {
        if (!(b0[i][2] != 0.0 && b1[i][2] != 0.0)) continue;
        double cx, cy, cpx, cpy, on;
        sample_box(b0, b1, n_sub, j, i, &cx, &cy, &on);
        sample_box(b0, b1, n_sub, j - 1, i, &cpx, &cpy, &on);
        const double ux = cx - cpx, uy = cy - cpy;
        dc = dmax(dc, sqrt(ux * ux + uy * uy));
    }
    const double ux = p[0] - pp[0], uy = p[1] - pp[1];
    const double delta = sqrt(ux * ux + uy * uy) + rmax * fabs(p[2] - pp[2]) + dc;
    return dmin_((d_prev + d - delta) / 2, dmin_(d_prev, d));
}

struct IntervalResult {
    double min_val;                    // smallest sampled distance
    int min_obst, min_sub;             // where (obstacle, sample 0..n_sub)
    double lower;                      // certified lower bound over the continuous interpolated motion
    double d0, d1;                     // distance at the two knots
};

// one closed-loop interval, n_sub + 1 samples in order (sample_distance / sub_bound above)
template <int MAXM>
AU_FN IntervalResult audit_interval(const Scene& S, const double* p0, const double* p1, const double (*b0)[3],
                                    const double (*b1)[3], int n_sub) {
    const double rmax = car_radius(S.ego);
    IntervalResult R;
    double prev_d = 0.0;
    int arg;
    R.min_val = INFINITY; R.min_obst = -1; R.min_sub = 0; R.lower = INFINITY; R.d0 = R.d1 = 0.0;
    for (int j = 0; j <= n_sub; ++j) {
        const double d = sample_distance<MAXM>(S, p0, p1, b0, b1, n_sub, j, &arg);
        if (d < R.min_val) { R.min_val = d; R.min_obst = arg; R.min_sub = j; }
        if (j == 0) R.d0 = d;
        if (j == n_sub) R.d1 = d;
        if (j > 0) R.lower = dmin_(R.lower, sub_bound(S, p0, p1, b0, b1, n_sub, j, rmax, prev_d, d));
        prev_d = d;
    }
    if (n_sub == 0) R.lower = R.min_val;
    return R;
}

// ---------------------------------------------------------------------------------------------------------------------
// Swept audit of one plan interval (obca_plan_sweep): stage s -> s + 1 of an obca_solve_batch plan, whose obstacles are
// rows per stage (A0 / b0 [M,2], [M] of stage s, A1 / b1 of stage s + 1; obca_mpc4 reads stage 0's rows at every stage, so
// its caller passes stage 0's rows as both ends).  Sample j = 0..n_sub, both knots included: the pose as sample_pose
// interpolates it, obstacle i's rows entry by entry, A(t) = A0 + t (A1 - A0), b(t) = b0 + t (b1 - b0), t = j / n_sub; at
// j = 0 and j = n_sub the stage's own words.  The distance is plan_distance with its NaN rule.
//
// What the interpolated rows are.  Let K = {q : A q <= b0} and let stage s + 1 hold the rows of K + c, a translation:
// A (q - c) <= b0, that is A q <= b0 + A c, so A1 = A and db = b1 - b0 = A c.  Then b(t) = b0 + A (t c): the interpolated
// rows are exactly those of K + t c, the set moving at constant velocity -- the harness's boxes and the swept, inflated
// rectangles of obca_moving_rows_batch at any half_window / margin alike (their size does not change along the horizon).
// Certified bound.  db determines the moved set: every c' with A c' = db gives the same rows, hence the same set, so the
// displacement to charge is the smallest such c' -- the least-squares solution dc of A dc = db over the obstacle's rows
// (normal equations G dc = A^T db, G = A^T A, 2 x 2), of minimum norm where G is singular (one row, or parallel rows: a
// half-plane or a strip moves along its normal only, dc = A^T db / trace G).  Over a sub-interval the set then moves by
// |dc| / n_sub, every point of the car by at most |dp| + r_max |dtheta| of the sub-interval (header of this file), and
// the signed distance is 1-Lipschitz under both (same place), so with delta their sum and end values d_j-1, d_j
//     d(u) >= min((d_j-1 + d_j - delta) / 2, d_j-1, d_j)         for every fraction u of the sub-interval,
// sub_bound's formula, and the minimum over the obstacles is bounded by the largest |dc| among them.  The argument needs
// a translation.  Rows whose normals change (max |A1 - A0| > 1e-9 max |A0|: beyond the roundoff that edge_row leaves on
// translated vertices) or whose db no translation explains (least-squares residual |A dc - db|_2 > 1e-9 (1 + max |b|),
// b over both stages) describe a set that turns or changes shape between the knots; linear interpolation of its rows is
// then no rigid motion, no displacement bound is known, and the obstacle's move -- with it the bound of every
// sub-interval of the interval and the instance's lower_bound -- is NaN.  The sampled values are reported either way.
constexpr double SWEEP_ROW_TOL = 1e-9;     // relative change of A, and residual of the translation fit
constexpr double SWEEP_RANK_TOL = 1e-12;   // det G <= tol (trace G)^2: the rows are parallel

// min with NaN below every number (the order of better()): a NaN operand wins
AU_FN double min_nan(double a, double b) { return (a != a || b != b) ? NAN : (a < b ? a : b); }

AU_FN double lerp_end(double v0, double v1, int n_sub, int j) {
    return j == 0 ? v0 : (j == n_sub ? v1 : v0 + ((double)j / (double)n_sub) * (v1 - v0));
}

// |dc| of one obstacle (m rows at A0 / b0 and A1 / b1) over the whole interval, NaN when no translation is certified
AU_FN double plan_obstacle_move(const double* A0, const double* b0, const double* A1, const double* b1, int m) {
    if (A0 == A1 && b0 == b1) return 0.0;                            // obca_mpc4: the rows stand still
    double g00 = 0.0, g01 = 0.0, g11 = 0.0, r0 = 0.0, r1 = 0.0, amax = 0.0, dmaxA = 0.0, bmax = 0.0;
    for (int j = 0; j < m; ++j) {
        const double a0 = A0[2 * j], a1 = A0[2 * j + 1], db = b1[j] - b0[j];
        g00 += a0 * a0; g01 += a0 * a1; g11 += a1 * a1;
        r0 += a0 * db; r1 += a1 * db;
        amax = dmax(amax, dmax(fabs(a0), fabs(a1)));
        dmaxA = dmax(dmaxA, dmax(fabs(A1[2 * j] - a0), fabs(A1[2 * j + 1] - a1)));
        bmax = dmax(bmax, dmax(fabs(b0[j]), fabs(b1[j])));
    }
    const double tr = g00 + g11, det = g00 * g11 - g01 * g01;
    double cx, cy;
    if (det <= SWEEP_RANK_TOL * tr * tr) { cx = r0 / tr; cy = r1 / tr; }
    else { cx = (g11 * r0 - g01 * r1) / det; cy = (g00 * r1 - g01 * r0) / det; }
    double res = 0.0;
    for (int j = 0; j < m; ++j) {
        const double e = A0[2 * j] * cx + A0[2 * j + 1] * cy - (b1[j] - b0[j]);
        res += e * e;
    }
    const double move = sqrt(cx * cx + cy * cy);
    // written so that a NaN anywhere (a non-finite row, tr = 0) fails the test
    const bool ok = dmaxA <= SWEEP_ROW_TOL * amax && sqrt(res) <= SWEEP_ROW_TOL * (1.0 + bmax) && isfinite(move);
    return ok ? move : NAN;
}

// the obstacles of one plan: n_obs obstacles of m[i] rows starting at row off[i] of a stage
struct PlanScene {
    const double* ego;
    int n_obs;
    const int32_t *m, *off;
};

// largest plan_obstacle_move over the obstacles (NaN if any is)
AU_FN double plan_move(const PlanScene& S, const double* A0, const double* b0, const double* A1, const double* b1) {
    double mv = 0.0;
    for (int i = 0; i < S.n_obs; ++i) {
        const double mi = plan_obstacle_move(A0 + 2 * S.off[i], b0 + S.off[i], A1 + 2 * S.off[i], b1 + S.off[i], S.m[i]);
        mv = (mv != mv || mi != mi) ? NAN : dmax(mv, mi);
    }
    return mv;
}

// distance to one obstacle of K rows (A0 / b0, A1 / b1: its rows at the two stages) at sample j.  K is a compile-time
// constant so that every loop over the rows unrolls and the interpolated rows live in registers: with a run-time row
// count the device compiler keeps them in an indexed array (LDS or scratch).
template <int MAXM, int K>
AU_FN double plan_rows_distance(const double C[4][2], const double* A0, const double* b0, const double* A1, const double* b1,
                                int n_sub, int j) {
    double A[2 * K], b[K];
    for (int r = 0; r < K; ++r) {
        A[2 * r] = lerp_end(A0[2 * r], A1[2 * r], n_sub, j);
        A[2 * r + 1] = lerp_end(A0[2 * r + 1], A1[2 * r + 1], n_sub, j);
        b[r] = lerp_end(b0[r], b1[r], n_sub, j);
    }
    return plan_distance<MAXM>(C, A, b, K);
}

// the same for a run-time row count 1 <= m <= MAXM
template <int MAXM, int K = 1>
AU_FN double plan_rows_distance_m(const double C[4][2], const double* A0, const double* b0, const double* A1,
                                  const double* b1, int m, int n_sub, int j) {
    if constexpr (K < MAXM) {
        if (m != K) return plan_rows_distance_m<MAXM, K + 1>(C, A0, b0, A1, b1, m, n_sub, j);
    }
    return plan_rows_distance<MAXM, K>(C, A0, b0, A1, b1, n_sub, j);
}

// smallest distance over the obstacles at sample j, one obstacle's interpolated rows at a time; arg = its obstacle
// (lowest among equals, a NaN first).  Evaluated from the interval's ends alone, like sample_distance.
template <int MAXM>
AU_FN double plan_sample_distance(const PlanScene& S, const double* p0, const double* p1, const double* A0, const double* b0,
                                  const double* A1, const double* b1, int n_sub, int j, int* arg) {
    double p[3], C[4][2];
    sample_pose(p0, p1, n_sub, j, p);
    car_corners(p[0], p[1], p[2], S.ego, C);
    double best = INFINITY;
    int ai = 0x7fffffff;
    for (int i = 0; i < S.n_obs; ++i) {
        const int o = S.off[i];
        const double d = plan_rows_distance_m<MAXM>(C, A0 + 2 * o, b0 + o, A1 + 2 * o, b1 + o, S.m[i], n_sub, j);
        if (better(d, 0, i, best, 0, ai)) { best = d; ai = i; }
    }
    *arg = ai;
    return best;
}

// certified bound of sub-interval j-1 -> j (j >= 1): sub_bound's formula with the obstacles' move of the whole interval
// (plan_move); NaN when an end value or the move is
AU_FN double plan_sub_bound(const double* p0, const double* p1, int n_sub, int j, double rmax, double move, double d_prev,
                            double d) {
    double p[3], pp[3];
    sample_pose(p0, p1, n_sub, j, p);
    sample_pose(p0, p1, n_sub, j - 1, pp);
    const double ux = p[0] - pp[0], uy = p[1] - pp[1];
    const double delta = sqrt(ux * ux + uy * uy) + rmax * fabs(p[2] - pp[2]) + move / (double)n_sub;
    return min_nan((d_prev + d - delta) / 2, min_nan(d_prev, d));
}

struct PlanIntervalResult {
    double min_val;                    // smallest sample (NaN if any sample is)
    int min_obst;                      // its obstacle: the lowest among equal samples
    double lower;                      // certified lower bound over the continuous interpolated motion, or NaN
};

// one plan interval, n_sub >= 1: n_sub + 1 samples in order
template <int MAXM>
AU_FN PlanIntervalResult plan_interval(const PlanScene& S, const double* p0, const double* p1, const double* A0,
                                       const double* b0, const double* A1, const double* b1, int n_sub) {
    const double rmax = car_radius(S.ego);
    const double move = plan_move(S, A0, b0, A1, b1);
    PlanIntervalResult R;
    R.min_val = INFINITY; R.min_obst = 0x7fffffff; R.lower = INFINITY;
    double prev_d = 0.0;
    for (int j = 0; j <= n_sub; ++j) {
        int arg;
        const double d = plan_sample_distance<MAXM>(S, p0, p1, A0, b0, A1, b1, n_sub, j, &arg);
        if (better(d, 0, arg, R.min_val, 0, R.min_obst)) { R.min_val = d; R.min_obst = arg; }
        if (j > 0) R.lower = min_nan(R.lower, plan_sub_bound(p0, p1, n_sub, j, rmax, move, prev_d, d));
        prev_d = d;
    }
    return R;
}

// per-instance reduction of the sweep over its intervals: (value, interval, obstacle) under better(), the bound under
// min_nan, the first colliding interval.  Both are total orders / commutative, so any reduction order gives the same words.
struct PlanSweepAcc {
    double best, lower;
    int bs, bo, coll;
};

AU_FN void plan_acc_init(PlanSweepAcc& a) { a.best = INFINITY; a.lower = INFINITY; a.bs = a.bo = 0x7fffffff; a.coll = -1; }

AU_FN void plan_acc_add(PlanSweepAcc& a, int s, const PlanIntervalResult& R) {
    if (better(R.min_val, s, R.min_obst, a.best, a.bs, a.bo)) { a.best = R.min_val; a.bs = s; a.bo = R.min_obst; }
    a.lower = min_nan(a.lower, R.lower);
    if (R.min_val < 0.0 && (a.coll < 0 || s < a.coll)) a.coll = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Clearance repair (obca_plan_tighten): where a feasible plan comes closer than `target` to an obstacle between two knots,
// grow that obstacle at the two stages next to the interval, so that a re-solve against the grown rows keeps the knots
// further out.  Nothing here touches the solver: the caller re-solves with b_out in place of b (A unchanged).
//
//   d[s,i]     the n_sub + 1 samples of plan_sweep for interval s, obstacle i alone (plan_tighten_distance): their
//              smallest, or with `certified` obstacle i's own bound over the interval, plan_sub_bound with that obstacle's
//              plan_obstacle_move -- NaN where its rows turn.  Always against the caller's ORIGINAL rows.
//   need[s,i]  gain (target - d[s,i]) where d[s,i] < target, else 0 (plan_tighten_need)
//   grow[k,i]  in/out, metres: min(grow_max, grow[k,i] + max(need[k-1,i], need[k,i])) over the intervals that exist; for
//              variant 4 the largest need[.,i] at every stage, because obca_mpc4 reads stage 0's rows only.  Never decreases.
//   b_out[k,r] b[k,r] + grow[k,i] |a_r|, |a_r| = hypot(A[k,r,0], A[k,r,1]), for every row r of obstacle i (plan_tighten_stage)
//
// Why the offset rows are enough.  Let K = {q : a_r q <= b_r for all r} and K' = {q : a_r q <= b_r + g |a_r|}.  A point q
// within g of some q0 in K has a_r q = a_r q0 + a_r (q - q0) <= b_r + |a_r| g for every r: K' contains K grown by a disc of
// radius g (at a vertex it contains more, the mitred corner).  The car at a knot that keeps dmin from K' therefore keeps
// dmin + g from K.  That is a statement about knots.  Between two knots nothing is guaranteed: the shortfall measured
// there is charged to the two knots next to it (for a half-plane, a car that does not turn and gain = 1 exactly: both
// knots pushed out by e move every interpolated pose out by e), the re-solved plan may take another way, and so the caller measures again -- always
// against the original rows -- and repeats a few rounds.
//
// Passed through (grow untouched, b_out = b + grow |a| as it stood, variant_out = 0): variant 0, a status outside {0, 1}
// -- neither is measured, min_clear = NaN -- and an instance with a measurement that is not finite (min_clear = NaN, the
// NaN rule of plan_distance).
template <int MAXM>
AU_FN double plan_tighten_distance(const PlanScene& S, int i, const double* p0, const double* p1, const double* A0,
                                   const double* b0, const double* A1, const double* b1, int n_sub, int certified,
                                   double rmax) {
    const int o = S.off[i], m = S.m[i];
    const double move = certified ? plan_obstacle_move(A0 + 2 * o, b0 + o, A1 + 2 * o, b1 + o, m) : 0.0;
    double best = INFINITY, prev = 0.0;
    for (int j = 0; j <= n_sub; ++j) {
        double p[3], C[4][2];
        sample_pose(p0, p1, n_sub, j, p);
        car_corners(p[0], p[1], p[2], S.ego, C);
        const double d = plan_rows_distance_m<MAXM>(C, A0 + 2 * o, b0 + o, A1 + 2 * o, b1 + o, m, n_sub, j);
        if (!certified) best = min_nan(best, d);
        else if (j > 0) best = min_nan(best, plan_sub_bound(p0, p1, n_sub, j, rmax, move, prev, d));
        prev = d;
    }
    return best;
}

AU_FN double plan_tighten_need(double d, double target, double gain) { return d < target ? gain * (target - d) : 0.0; }

// true when the plan of an instance is one to measure and repair
AU_FN bool plan_tighten_active(int variant, int status) { return variant != 0 && (status == 0 || status == 1); }

// one (stage, obstacle): grow by inc where `update` (the instance is not passed through), then the obstacle's m rows of
// b_out from the stage's own A / b.  Returns 1 if grow rose.
AU_FN int plan_tighten_stage(const double* Ak, const double* bk, int m, double inc, double grow_max, bool update, double* grow_ki,
                             double* bout_k) {
    RO_EXACT
    double g = *grow_ki;
    int rose = 0;
    if (update) {
        const double gn = dmax(g, dmin_(grow_max, g + inc));
        rose = gn > g;
        if (rose) *grow_ki = gn;
        g = gn;
    }
    for (int r = 0; r < m; ++r) bout_k[r] = bk[r] + g * hypot(Ak[2 * r], Ak[2 * r + 1]);
    return rose;
}

}  // namespace audit

// ---------------------------------------------------------------------------------------------------------------------
// Collision stop of the closed loop (obca_rollouts_set_collision_stop): the simulator's contact check, NOT the controller's
// knowledge -- every present moving box counts, sensed or not.  After finish() has applied step k of rollout b, interval
// k (knot k -> k + 1) is measured with exactly the inputs and rules of the rollout audit (obca_audit.hip): poses from
// x_closed, the boxes at knot k from the dyn_hist record, at knot k + 1 from the harness's update law with T_closed[k],
// the static rows, n_sub + 1 samples.  The sampled minimum (stop_certified: the certified lower bound) goes to clr[b, k];
// below stop_clear the rollout ends with OBCA_DONE_COLLISION, which wins over GOAL / CAP of the same step.  The colliding
// step stays in the history: a stopped rollout's history is the unstopped one's, cut after that step.
namespace rollout {

// the interval of the step finish() has just applied to rollout b, or -1 (the stop is off, the rollout did not run this
// step -- prepare() zeroes var[.][b] of a rollout that is not running -- or its step failed and applied nothing).  Leaves
// the boxes at the two knots (cx, cy, present) in rollout b's vtx row: b0 = row[0 .. 3 nd), b1 = row[12 .. 12 + 3 nd)
// (prepare()'s scratch, free after it)
AU_FN int stop_interval(const Dev& D, int b) {
    if (D.stop_nsub <= 0 || D.var[D.sel[b]][b] == 0 || D.flags[b] == OBCA_DONE_FAILED) return -1;
    const int k = D.k[b] - 1, nd = D.n_dyn;
    if (k < 0) return -1;
    double* row = D.vtx + (size_t)b * OBCA_MAX_DYN * 8;
    const double T = D.Tc[(size_t)b * D.S + k];
    for (int i = 0; i < nd; ++i) {
        const double* rec = D.dh + (((size_t)b * D.S + k) * nd + i) * 4;
        const double* info = D.dyn + ((size_t)b * nd + i) * DYN_W;
        row[3 * i] = rec[0]; row[3 * i + 1] = rec[1]; row[3 * i + 2] = rec[2];
        audit::box_next_knot(info, rec[0], rec[1], k + 1, T, row + 3 * OBCA_MAX_DYN + 3 * i);
    }
    return k;
}

AU_FN audit::Scene stop_scene(const Dev& D, int b) {
    audit::Scene sc;
    sc.ego = D.ego;
    sc.n_static = D.n_static;
    sc.m = D.m_static;
    sc.As = D.As + (size_t)b * D.Ms * 2;
    sc.bs = D.bs + (size_t)b * D.Ms;
    sc.nd = D.n_dyn;
    sc.dyn = D.dyn + (size_t)b * D.n_dyn * DYN_W;
    return sc;
}

AU_FN void stop_apply(const Dev& D, int b, int k, double v) {
    D.clr[(size_t)b * D.S + k] = v;
    if (v < D.stop_clear) D.flags[b] = OBCA_DONE_COLLISION;
}

// serial form: one lane (host build, lock-step kernel) runs the samples in order
AU_FN void stop_check(const Dev& D, int b) {
    const int k = stop_interval(D, b);
    if (k < 0) return;
    const double* row = D.vtx + (size_t)b * OBCA_MAX_DYN * 8;
    const double* p0 = D.xc + ((size_t)b * (D.S + 1) + k) * 3;
    const audit::IntervalResult R = audit::audit_interval<OBCA_MAX_EDGES>(
        stop_scene(D, b), p0, p0 + 3, reinterpret_cast<const double (*)[3]>(row),
        reinterpret_cast<const double (*)[3]>(row + 3 * OBCA_MAX_DYN), D.stop_nsub);
    stop_apply(D, b, k, D.stop_certified ? R.lower : R.min_val);
}

#if defined(__HIPCC__)
// wavefront form (fused kernel; lock-step stop kernel): called by all 64 lanes of a one-wave workgroup with the same b.
// Lane j <= n_sub evaluates sample j and the bound of sub-interval j-1 -> j (d_j-1 from lane j-1); min-reductions across
// the lanes.  Same expressions as the serial loop and min is exact: the same words.
__device__ inline void stop_check_wave(const Dev& D, int b) {
    const int lane = threadIdx.x;
    int k = -1;
    if (lane == 0) k = stop_interval(D, b);
    __syncthreads();                                   // the vtx row written by lane 0
    k = __builtin_amdgcn_readfirstlane(k);
    if (k < 0) return;
    const int n = D.stop_nsub;
    const double* row = D.vtx + (size_t)b * OBCA_MAX_DYN * 8;
    const double (*b0)[3] = reinterpret_cast<const double (*)[3]>(row);
    const double (*b1)[3] = reinterpret_cast<const double (*)[3]>(row + 3 * OBCA_MAX_DYN);
    const double* p0 = D.xc + ((size_t)b * (D.S + 1) + k) * 3;
    const audit::Scene sc = stop_scene(D, b);
    double d = INFINITY, term = INFINITY;
    int arg;
    if (lane <= n) d = audit::sample_distance<OBCA_MAX_EDGES>(sc, p0, p0 + 3, b0, b1, n, lane, &arg);
    const double d_prev = __shfl_up(d, 1, 64);
    if (lane >= 1 && lane <= n) term = audit::sub_bound(sc, p0, p0 + 3, b0, b1, n, lane, audit::car_radius(sc.ego), d_prev, d);
    for (int w = 32; w > 0; w >>= 1) {
        d = audit::dmin_(d, __shfl_xor(d, w, 64));
        term = audit::dmin_(term, __shfl_xor(term, w, 64));
    }
    if (lane == 0) stop_apply(D, b, k, D.stop_certified ? term : d);
}
#endif

}  // namespace rollout
#endif
