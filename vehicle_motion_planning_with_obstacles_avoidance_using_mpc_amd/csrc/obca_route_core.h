// obca_route_core.h -- from an A* route to the reference of a fixed-horizon solve: the disk dilation of an occupancy grid
// (reference mapModel.dilate_map, src/model_map.py:103-107) and the resampling of a route of path_len lattice points to
// N + 1 knots equally spaced in arc length, yaws by a_star.create_reference_path's rule (src/a_star.py:189-200).  One
// function per OUTPUT CELL and per OUTPUT KNOT, shared by the kernels of csrc/obca_route.hip (one lane each) and the host
// build (tests/native/route_host.cpp).
//
// Dilation, for a grid [rows,cols] of bytes and a level 0 <= level <= MAX_LEVEL:
//   out[r,c] = 1 iff some cell (r + dy, c + dx) INSIDE the grid with dy^2 + dx^2 <= level^2 is non-zero, else 0
//   (cells outside the grid count as free; level 0 maps a non-zero byte to 1 and nothing else).
//
// Resampling, for a route (px, py) of L >= 2 points and a horizon N (all sums, products and quotients rounded one by one: the
// functions carry `fp contract(off)`, the library is built with contraction on):
//   d_i = sqrt(dx_i dx_i + dy_i dy_i), i = 0 .. L-2;  S_0 = 0, S_i+1 = S_i + d_i in index order;  S = S_L-1
//   knot k < N   s_k = ((double)k S) / (double)N;  its segment: the first i with d_i > 0 and S_i+1 >= s_k;
//                t = (s_k - S_i) / d_i;  p = p_i + t (p_i+1 - p_i) per coordinate
//   knot N       the last route point itself
//   pins         knot 0's position := start[0..1], knot N's := goal[0..1], where given
//   yaw_k        atan2(y_k+1 - y_k, x_k+1 - x_k) on these final positions for k < N, yaw_N = yaw_N-1: every knot recomputes
//                its successor, so that no knot depends on another lane's result;  then yaw_0 := start[2], yaw_N := goal[2]
// Not resampled (ok = 0; nothing a later launch reads may be NaN): L < 2 (obca_astar_batch's negative codes included),
// L > path_max, a point (x, y or yaw) among the first L that is not finite, S zero or not finite.  A pin that is not finite is
// dropped for its instance, which is then not resampled either.  Such an instance gets, with both pins (finite): start at
// knot 0 and goal at every other knot, all three components -- the start/goal-only reference; otherwise point 0 of the
// path at every knot, or zeros where that point is not finite.
#ifndef OBCA_ROUTE_CORE_H
#define OBCA_ROUTE_CORE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_FN __host__ __device__ inline
#else
#define RT_FN inline
#endif

namespace route {

constexpr int MAX_N = 127;                 // the longest horizon obca_create takes (csrc/obca_capi.hip: dims_ok)
constexpr int MAX_LEVEL = 16;              // largest dilation radius, cells: (2 x 16 + 1)^2 = 1089 reads per output cell
constexpr int MAX_CELLS = 65535;           // rows x cols, the bound of obca_astar_batch
constexpr int E_INVAL = -22;               // OBCA_E_INVAL

RT_FN bool finite_(double v) { return v - v == 0.0; }          // false for NaN and +-inf, no libm call

// the checks of obca_grid_dilate_batch, made before anything is read or written (the host build makes the same ones)
RT_FN int dilate_args_check(int32_t B, int32_t rows, int32_t cols, int32_t level, const uint8_t* grid, const uint8_t* out) {
    if (B < 1 || rows < 1 || cols < 1 || (int64_t)rows * cols > MAX_CELLS || level < 0 || level > MAX_LEVEL) return E_INVAL;
    if (!grid || !out) return E_INVAL;
    const uintptr_t total = (uintptr_t)B * rows * cols, g = (uintptr_t)grid, o = (uintptr_t)out;
    if (g < o + total && o < g + total) return E_INVAL;                    // in == out, or any other overlap
    return 0;
}

// output cell (r, c) of one grid
RT_FN uint8_t dilate_cell(const uint8_t* grid, int rows, int cols, int r, int c, int level) {
    const int r0 = r - level > 0 ? r - level : 0, r1 = r + level < rows - 1 ? r + level : rows - 1;
    const int c0 = c - level > 0 ? c - level : 0, c1 = c + level < cols - 1 ? c + level : cols - 1;
    const int l2 = level * level;
    for (int rr = r0; rr <= r1; ++rr) {
        const int dy2 = (rr - r) * (rr - r);
        for (int cc = c0; cc <= c1; ++cc)
            if (dy2 + (cc - c) * (cc - c) <= l2 && grid[rr * cols + cc] != 0) return 1;
    }
    return 0;
}

// the checks of obca_route_resample
RT_FN int args_check(int32_t B, int32_t path_max, int32_t N, const double* path, const int32_t* path_len, const double* xref,
                     const int32_t* ok) {
    if (B < 1 || path_max < 1 || N < 1 || N > MAX_N) return E_INVAL;
    if (!path || !path_len || !xref || !ok) return E_INVAL;
    return 0;
}

RT_FN bool pose_finite(const double* p) { return p && finite_(p[0]) && finite_(p[1]) && finite_(p[2]); }

RT_FN double seg_len(const double* px, const double* py, int i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dx = px[i + 1] - px[i], dy = py[i + 1] - py[i];
    const double xx = dx * dx, yy = dy * dy;
    return sqrt(xx + yy);
}

// is the route path [3,path_max] with L points resampled (true, *S_out its length) or filled (false)
RT_FN bool usable(const double* path, int path_max, int L, double* S_out) {
    *S_out = 0.0;
    if (L < 2 || L > path_max) return false;
    bool ok = true;
    for (int i = 0; i < L; ++i)
        ok = ok && finite_(path[i]) && finite_(path[path_max + i]) && finite_(path[2 * path_max + i]);
    if (!ok) return false;
    double S = 0.0;
    for (int i = 0; i + 1 < L; ++i) S = S + seg_len(path, path + path_max, i);
    *S_out = S;
    return finite_(S) && S > 0.0;
}

// position of knot k (0 <= k <= N) on the route itself, before the pins
RT_FN void on_route(const double* px, const double* py, int L, double S, int N, int k, double out[2]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    out[0] = px[L - 1]; out[1] = py[L - 1];
    if (k >= N) return;
    const double ks = (double)k * S;
    const double s = ks / (double)N;
    double Si = 0.0;
    for (int i = 0; i + 1 < L; ++i) {
        const double d = seg_len(px, py, i);
        const double Sn = Si + d;
        if (d > 0.0 && Sn >= s) {
            const double t = (s - Si) / d;
            const double tx = t * (px[i + 1] - px[i]), ty = t * (py[i + 1] - py[i]);
            out[0] = px[i] + tx; out[1] = py[i] + ty;
            return;
        }
        Si = Sn;
    }
}

// final position of knot k: the pins applied
RT_FN void knot_pos(const double* px, const double* py, int L, double S, int N, int k, const double* start, const double* goal,
                    double out[2]) {
    if (k == 0 && start) { out[0] = start[0]; out[1] = start[1]; return; }
    if (k >= N && goal) { out[0] = goal[0]; out[1] = goal[1]; return; }
    on_route(px, py, L, S, N, k, out);
}

// output knot k (0 <= k <= N) of one instance: out = (x, y, yaw).  start / goal: the instance's pins [3] or NULL;
// ok: usable() of the route AND every given pin finite
RT_FN void knot(const double* path, int path_max, int L, double S, int N, int k, const double* start, const double* goal, bool ok,
                double out[3]) {
    if (!ok) {
        if (pose_finite(start) && pose_finite(goal)) {
            const double* q = k == 0 ? start : goal;
            out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
            return;
        }
        const bool p0 = finite_(path[0]) && finite_(path[path_max]) && finite_(path[2 * path_max]);
        out[0] = p0 ? path[0] : 0.0; out[1] = p0 ? path[path_max] : 0.0; out[2] = p0 ? path[2 * path_max] : 0.0;
        return;
    }
    const double *px = path, *py = path + path_max;
    const int k0 = k < N ? k : N - 1;                          // the last knot repeats the previous yaw
    double a[2], b[2];
    knot_pos(px, py, L, S, N, k0, start, goal, a);
    knot_pos(px, py, L, S, N, k0 + 1, start, goal, b);
    out[0] = k < N ? a[0] : b[0];
    out[1] = k < N ? a[1] : b[1];
    out[2] = atan2(b[1] - a[1], b[0] - a[0]);
    if (k == 0 && start) out[2] = start[2];
    if (k >= N && goal) out[2] = goal[2];
}

// the whole decision for one instance: usable route and finite pins
RT_FN bool instance_ok(const double* path, int path_max, int L, const double* start, const double* goal, double* S_out) {
    const bool r = usable(path, path_max, L, S_out);
    return r && (!start || pose_finite(start)) && (!goal || pose_finite(goal));
}

}  // namespace route

#endif
