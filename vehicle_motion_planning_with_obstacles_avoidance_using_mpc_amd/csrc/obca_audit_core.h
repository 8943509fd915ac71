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

// smallest signed distance over the scene at pose p with the moving boxes at box[j] = (cx, cy, on); arg = obstacle index
// (static first, then n_static + j; ties to the lowest)
template <int MAXM>
AU_FN double scene_distance(const Scene& S, const double* p, const double (*box)[3], int* arg) {
    double C[4][2];
    car_corners(p[0], p[1], p[2], S.ego, C);
    double best = INFINITY;
    int ai = -1, off = 0;
    for (int i = 0; i < S.n_static; ++i) {
        const double d = signed_distance<MAXM>(C, S.As + 2 * off, S.bs + off, S.m[i]);
        off += S.m[i];
        if (d < best) { best = d; ai = i; }
    }
    for (int j = 0; j < S.nd; ++j) {
        if (box[j][2] == 0.0) continue;
        const double* info = S.dyn + (size_t)j * rollout::DYN_W;
        const double d = box_distance(C, box[j][0], box[j][1], info[11], info[12], info[3], info[4]);
        if (d < best) { best = d; ai = S.n_static + j; }
    }
    *arg = ai;
    return best;
}

struct IntervalResult {
    double min_val;                    // smallest sampled distance
    int min_obst, min_sub;             // where (obstacle, sample 0..n_sub)
    double lower;                      // certified lower bound over the continuous interpolated motion
    double d0, d1;                     // distance at the two knots
};

// one closed-loop interval: poses p0 -> p1 interpolated linearly in (x, y, theta), boxes b0 -> b1 (a box present at
// both ends moves linearly; one present only at b1 counts at the end knot only), n_sub + 1 samples, both knots included.
// n_sub == 0: the single knot p0 / b0 (a rollout without steps).
template <int MAXM>
AU_FN IntervalResult audit_interval(const Scene& S, const double* p0, const double* p1, const double (*b0)[3],
                                    const double (*b1)[3], int n_sub) {
    constexpr int MD = OBCA_MAX_DYN;
    const double rmax = car_radius(S.ego);
    IntervalResult R;
    double prev_p[3], prev_c[MD][2], box[MD][3], p[3];
    double prev_d = 0.0;
    int arg;
    R.min_val = INFINITY; R.min_obst = -1; R.min_sub = 0; R.lower = INFINITY; R.d0 = R.d1 = 0.0;
    for (int j = 0; j <= n_sub; ++j) {
        const bool first = j == 0, last = j == n_sub;
        const double t = n_sub > 0 ? (double)j / (double)n_sub : 0.0;
        for (int q = 0; q < 3; ++q) p[q] = first ? p0[q] : (last ? p1[q] : p0[q] + t * (p1[q] - p0[q]));
        double dc = 0.0;
        for (int i = 0; i < S.nd && i < MD; ++i) {
            const bool both = b0[i][2] != 0.0 && b1[i][2] != 0.0;
            if (first) { box[i][0] = b0[i][0]; box[i][1] = b0[i][1]; box[i][2] = b0[i][2]; }
            else if (last) { box[i][0] = b1[i][0]; box[i][1] = b1[i][1]; box[i][2] = b1[i][2]; }
            else {
                box[i][0] = b0[i][0] + t * (b1[i][0] - b0[i][0]);
                box[i][1] = b0[i][1] + t * (b1[i][1] - b0[i][1]);
                box[i][2] = b0[i][2];
            }
            if (!first && both) {
                const double ux = box[i][0] - prev_c[i][0], uy = box[i][1] - prev_c[i][1];
                dc = dmax(dc, sqrt(ux * ux + uy * uy));
            }
            prev_c[i][0] = box[i][0]; prev_c[i][1] = box[i][1];
        }
        const double d = scene_distance<MAXM>(S, p, box, &arg);
        if (d < R.min_val) { R.min_val = d; R.min_obst = arg; R.min_sub = j; }
        if (first) R.d0 = d;
        if (last) R.d1 = d;
        if (!first) {
            const double ux = p[0] - prev_p[0], uy = p[1] - prev_p[1];
            const double delta = sqrt(ux * ux + uy * uy) + rmax * fabs(p[2] - prev_p[2]) + dc;
            R.lower = dmin_(R.lower, dmin_((prev_d + d - delta) / 2, dmin_(prev_d, d)));
        }
        for (int q = 0; q < 3; ++q) prev_p[q] = p[q];
        prev_d = d;
    }
    if (n_sub == 0) R.lower = R.min_val;
    return R;
}

}  // namespace audit
#endif
