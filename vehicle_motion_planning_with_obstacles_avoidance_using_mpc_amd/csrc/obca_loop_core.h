// obca_loop_core.h -- what the "between two solves" calls of the closed loops over scene pools share (obca_pool_loop_advance,
// obca_fleet_step, obca_fleet_tracks, obca_pool_tracks of include/obca_mpc.h): the defaults their *_init calls write, and the
// one way a rollout ends -- variant_out[b] = 0 and a reference window that is the car's pose, every word finite.  Each core
// (csrc/obca_poolloop_core.h, csrc/obca_fleet_core.h and through it the two track cores) includes this and adds its own
// init(d) on top of init_common.  The serial mask_rollout is the specification; mask_rollout_wave is what the kernels call
// and must write the same words.
#ifndef OBCA_LOOP_CORE_H
#define OBCA_LOOP_CORE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LOOP_FN __host__ __device__ inline
#else
#define LOOP_FN inline
#endif

namespace loop {

constexpr double DEFAULT_EGO[4] = {1.7, 0.75, 1.7, 0.75};     // front, left, rear, right of the reference's car
constexpr double NEVER_STOP = -1e300;                         // clearance: no finite distance is below it
constexpr double DEFAULT_FAR = 100.0;                         // where a spare slot's rectangle lies
constexpr double DEFAULT_GOAL_TOL2 = 0.1;                     // rollout::at_goal's squared distance

LOOP_FN double finite_or_zero(double v) { return v - v == 0.0 ? v : 0.0; }   // 0 for NaN and +-inf, no libm call

// what every *_init does first: all zero (= every other default), struct_size set, the default ego
template <class D>
inline void init_common(D* d) {
    memset(d, 0, sizeof(*d));
    d->struct_size = (uint32_t)sizeof(*d);
    for (int q = 0; q < 4; ++q) d->ego[q] = DEFAULT_EGO[q];
}

// ---- the serial definition: rollout b, which stands at x0 [B,3], takes no further solve
inline void mask_rollout(int32_t* variant_out, double* xref_out, const double* x0, int64_t b, int N1) {
    variant_out[b] = 0;
    for (int j = 0; j < 3; ++j)
        for (int t = 0; t < N1; ++t) xref_out[b * 3 * N1 + j * N1 + t] = finite_or_zero(x0[3 * b + j]);
}

#if defined(__HIPCC__)
// the same by one wavefront of 64, every lane holding the pose: lane 0 writes the word, the lanes stride over the window
__device__ inline void mask_rollout_wave(int32_t* variant_out, double* xref_out, int64_t b, int N1, double px, double py, double pt,
                                         int lane) {
    if (lane == 0) variant_out[b] = 0;
    const double qx = finite_or_zero(px), qy = finite_or_zero(py), qt = finite_or_zero(pt);
    double* xr = xref_out + b * 3 * N1;
    for (int t = lane; t < N1; t += 64) { xr[t] = qx; xr[N1 + t] = qy; xr[2 * N1 + t] = qt; }
}
#endif

}  // namespace loop

#endif
