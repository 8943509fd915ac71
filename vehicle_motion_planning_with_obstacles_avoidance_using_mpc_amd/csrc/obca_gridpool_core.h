// obca_gridpool_core.h -- occupancy grid -> scene pool: the inverse of obca_rasterise_batch.  One grid of rows x cols bytes
// (non-zero = occupied) is covered by disjoint axis-parallel rectangles of cells, and every rectangle becomes one pool
// obstacle of E = 4 rows for obca_scene_select (pool_A [K,4,2], pool_b [K,4]).  Plain functions shared by gridpool_kernel of
// csrc/obca_gridpool.hip (one wavefront per map) and the host build (tests/native/grid_pool_host.cpp): the argument check,
// the serial cover -- which is the specification the kernel reproduces integer for integer --, the rows of one rectangle and
// the rows of a spare slot.
//
// Cover (greedy right-then-down, on a bit-packed copy `work` of the occupied cells):
//   n = 0
//   for r = 0 .. rows-1, for c = 0 .. cols-1 (row-major):
//       if (r, c) in work:
//           c1 = last column of the unbroken run of work cells (r, c), (r, c+1), ...
//           r1 = last row such that every cell of rows r .. r1, columns c .. c1 is in work
//           remove rows r..r1 x columns c..c1 from work
//           if n < K: rect[n] = (r, c, r1, c1)
//           n = n + 1
//   count = n                            (the true number, also where it exceeds K)
// A cell can leave `work` through a rectangle seeded above it: that ends a run or a downward extension early.  The
// rectangles are disjoint, their union is the occupied set, and they are listed in strictly ascending (r0, c0).  It is no
// minimum-count cover.
//
// Rows of a rectangle (r0, c0, r1, c1) at resolution `res`, grown by `pad` metres on every side:
//   xlo = c0 res - pad, xhi = c1 res + pad, ylo = r0 res - pad, yhi = r1 res + pad        (every product and difference rounded
//   on its own: `fp contract(off)`, the library is built with contraction on)
//   rows (a | b) in this order: (0, 1 | yhi), (1, 0 | xhi), (0, -1 | -ylo), (-1, 0 | -xlo)
// -- for a rectangle with area the words obstacleModel.obstacle_H_Represent gives for the clockwise polygon
// [[xlo,yhi],[xhi,yhi],[xhi,ylo],[xlo,ylo],[xlo,yhi]].  pad = 0 is the reference's convention (a cell is a lattice point; the
// box [c0,c1] x [r0,r1] rasterises back to exactly these cells); pad = res / 2 treats a cell as a square centred on its
// lattice point, so that neighbouring rectangles touch.
//
// Spare slots k >= count: rect (-1,-1,-1,-1) and the rows of the unit square [-far-1, -far]^2 in the same row order.  `far`
// is the caller's, not a constant like the -1e6 fill of obca_scene_select: a spare obstacle that is SELECTED becomes rows of
// a solve, and the structured solver (host build, 32 headline instances with a fourth obstacle added to m = [4,4,4]) stays
// feasible with the same plans to 1e-11 m for a spare at far = 100 or 1000, and is feasible on 0 of 32 at far = 1e6.  The
// Python default is far = 100.
//
// ok = 1 if count <= K, else 0: the first K rectangles are written and valid, the map is just not covered.  Nothing written
// is ever NaN.
#ifndef OBCA_GRIDPOOL_CORE_H
#define OBCA_GRIDPOOL_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GP_FN __host__ __device__ inline
#else
#define GP_FN inline
#endif

// exact arithmetic (no fused multiply-add), as RO_EXACT of obca_rollout_core.h: first statement of the functions that round
#if defined(__clang__)
#define GP_EXACT _Pragma("clang fp contract(off)")
#else
#define GP_EXACT /* g++: built with -ffp-contract=off */
#endif

namespace gridpool {

constexpr int MAX_K = 64;                  // scene::MAX_K: one lane per pool obstacle, here one lane per output slot
constexpr int E = 4;                       // rows of a rectangle
constexpr int MAX_WORDS = 4096;            // rows * ceil(cols / 64) 64-bit words: the bit-packed grid in 32 KB of LDS
constexpr int E_INVAL = -22;               // OBCA_E_INVAL

GP_FN bool finite_(double v) { return v - v == 0.0; }          // false for NaN and +-inf, no libm call

GP_FN int words_per_row(int cols) { return (cols + 63) / 64; }

// the checks of obca_grid_pool, made before anything is read or written (the host build makes the same ones); rect may be NULL
GP_FN int args_check(int32_t B, int32_t rows, int32_t cols, int32_t K, double res, double pad, double far, const uint8_t* grid,
                     const double* pool_A, const double* pool_b, const int32_t* count, const int32_t* ok) {
    if (B < 1 || K < 1 || K > MAX_K || rows < 1 || cols < 1) return E_INVAL;
    if ((int64_t)rows * (((int64_t)cols + 63) / 64) > MAX_WORDS) return E_INVAL;
    if (!finite_(res) || !finite_(pad) || !finite_(far) || !(res > 0.0) || !(pad >= 0.0) || !(far > 0.0)) return E_INVAL;
    if (!grid || !pool_A || !pool_b || !count || !ok) return E_INVAL;
    if (((uintptr_t)pool_A & 15) != 0) return E_INVAL;          // one 16-byte store per row of pool_A
    return 0;
}

// bit-packed copy of one grid: bit c % 64 of work[r W + c / 64] = (grid[r, c] != 0), the bits beyond cols zero
GP_FN void pack(const uint8_t* grid, int rows, int cols, uint64_t* work) {
    const int W = words_per_row(cols);
    for (int q = 0; q < rows * W; ++q) work[q] = 0;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c)
            if (grid[(int64_t)r * cols + c] != 0) work[r * W + (c >> 6)] |= 1ull << (c & 63);
}

GP_FN bool cell(const uint64_t* work, int W, int r, int c) { return ((work[r * W + (c >> 6)] >> (c & 63)) & 1ull) != 0; }

// the serial cover: consumes work [rows W], writes the first K rectangles (r0, c0, r1, c1) to rect [K,4], returns the count
GP_FN int cover(uint64_t* work, int rows, int cols, int K, int32_t* rect) {
    const int W = words_per_row(cols);
    int n = 0;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            if (!cell(work, W, r, c)) continue;
            int c1 = c, r1 = r;
            while (c1 + 1 < cols && cell(work, W, r, c1 + 1)) ++c1;
            while (r1 + 1 < rows) {
                bool all = true;
                for (int q = c; q <= c1 && all; ++q) all = cell(work, W, r1 + 1, q);
                if (!all) break;
                ++r1;
            }
            for (int rr = r; rr <= r1; ++rr)
                for (int q = c; q <= c1; ++q) work[rr * W + (q >> 6)] &= ~(1ull << (q & 63));
            if (n < K) { rect[4 * n] = r; rect[4 * n + 1] = c; rect[4 * n + 2] = r1; rect[4 * n + 3] = c1; }
            ++n;
        }
    return n;
}

// the four rows of the box [xlo, xhi] x [ylo, yhi]: A [4,2], b [4]
GP_FN void box_rows(double xlo, double xhi, double ylo, double yhi, double* A, double* b) {
    A[0] = 0.0; A[1] = 1.0; b[0] = yhi;
    A[2] = 1.0; A[3] = 0.0; b[1] = xhi;
    A[4] = 0.0; A[5] = -1.0; b[2] = -ylo;
    A[6] = -1.0; A[7] = 0.0; b[3] = -xlo;
}

// rows of the rectangle of cells (r0, c0, r1, c1)
GP_FN void rect_rows(int r0, int c0, int r1, int c1, double res, double pad, double* A, double* b) {
    GP_EXACT
    const double px0 = (double)c0 * res, px1 = (double)c1 * res, py0 = (double)r0 * res, py1 = (double)r1 * res;
    const double xlo = px0 - pad, xhi = px1 + pad, ylo = py0 - pad, yhi = py1 + pad;
    box_rows(xlo, xhi, ylo, yhi, A, b);
}

// rows of a spare slot: the unit square [-far-1, -far]^2
GP_FN void spare_rows(double far, double* A, double* b) {
    GP_EXACT
    const double hi = -far, lo = hi - 1.0;
    box_rows(lo, hi, lo, hi, A, b);
}

// slot k of an instance with `count` rectangles, the first min(count, K) of them in rect_in [K,4]: rows and rect words
GP_FN void slot(int k, int count, const int32_t* rect_in, double res, double pad, double far, double* A, double* b, int32_t q[4]) {
    if (k < count) {
        for (int j = 0; j < 4; ++j) q[j] = rect_in[4 * k + j];
        rect_rows(q[0], q[1], q[2], q[3], res, pad, A, b);
    } else {
        for (int j = 0; j < 4; ++j) q[j] = -1;
        spare_rows(far, A, b);
    }
}

}  // namespace gridpool

#endif
