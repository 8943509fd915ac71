// obca_poolloop.hip -- obca_pool_loop_advance of include/obca_mpc.h: the harness between two solves of the closed loop over
// scene pools.  The arithmetic and the serial definition are csrc/obca_poolloop_core.h.
//
// Layout (obca_scene.hip's): one wavefront per rollout, lane = pool obstacle (hence K <= 64), blocks of 256 = four rollouts.
//   measure   lane i < K runs scene::score_obstacle for its obstacle on the two-knot plan; the K values go through LDS and
//             every lane folds them in index order with audit::min_nan (broadcast reads, no atomics): the serial loop's word,
//             the same in every lane, so the flag decisions are wave-uniform
//   move      lane i < K rewrites its own E words of pool_b (after the fold: a failed step moves nothing)
//   window    lanes stride over the path_len points, each keeps its first strict minimum below 1e5; a butterfly of
//             cross-lane moves combines (distance, index) with ties to the lower index -- a total order, so every lane ends
//             with the serial loop's i0 (0 when no lane found a point)
//   stores    lanes t <= N write the window's columns, lanes below 3 the pose words, lane 0 the scalars; at a start the
//             wavefront strides over the histories
// Wavefronts beyond B run through the barrier and touch no memory; lanes beyond K form no address.  Every value a lane
// stores is picked with selects from scalars: no local array is indexed with a lane number (that is a stack frame).
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_poolloop_core.h"

namespace {

constexpr int BLOCK = 256, WAVE = 64, PER_BLOCK = BLOCK / WAVE;

__device__ inline double pick3(int j, double a, double b, double c) { return j == 0 ? a : (j == 1 ? b : c); }

__global__ void __launch_bounds__(BLOCK) poolloop_kernel(obca_pool_loop D, int32_t solved) {
    __shared__ double s_cur[PER_BLOCK][WAVE];
    const int w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t b = (int64_t)blockIdx.x * PER_BLOCK + w;
    const bool live = b < D.B;                                       // wave-uniform
    const bool mine = live && lane < D.K;
    const int K = D.K, E = D.E, N = D.N, N1 = N + 1, S = D.max_steps, n_sel = D.n_sel, P = D.path_max;

    int flag = live ? (solved ? D.flags[b] : OBCA_RUN) : OBCA_DONE_FAILED;
    double px = 0.0, py = 0.0, pt = 0.0;                             // the pose the window is made for
    if (live) { px = D.x0[3 * b]; py = D.x0[3 * b + 1]; pt = D.x0[3 * b + 2]; }

    // ---- finish, first half: record, read the solve, measure
    bool fin = live && solved && flag == OBCA_RUN;                   // wave-uniform
    const int kb = fin ? D.k[b] : 0;
    if (fin && !poolloop::step_in_range(kb, S)) {                    // a counter the caller broke: nothing is written
        fin = false;
        flag = OBCA_DONE_FAILED;
        if (lane == 0) D.flags[b] = flag;
    }
    double p1x = 0.0, p1y = 0.0, p1t = 0.0, ux = 0.0, uy = 0.0, ts = 0.0;
    bool applied = false;
    if (fin) {
        if (lane == 0) {
            D.status_hist[b * S + kb] = D.status[b];
            D.iters_hist[b * S + kb] = D.iters[b];
        }
        if (lane < n_sel) D.sel_hist[(b * S + kb) * n_sel + lane] = D.sel[b * n_sel + lane];
        const double* xo = D.xopt + b * 3 * N1;
        const double* uo = D.uopt + b * 2 * N;
        p1x = xo[1]; p1y = xo[N1 + 1]; p1t = xo[2 * N1 + 1];
        ux = uo[0]; uy = uo[N];
        ts = D.ts_opt[b];
        applied = !poolloop::solve_bad(D.status[b], p1x, p1y, p1t, ux, uy, ts);
    }
    const double* pA = mine ? D.pool_A + (b * K + lane) * E * 2 : nullptr;
    double* pb = mine ? D.pool_b + (b * K + lane) * E : nullptr;
    const double* pv = mine && D.pool_v ? D.pool_v + (b * K + lane) * 2 : nullptr;
    const bool measure = applied && D.n_sub > 0;
    double cur = INFINITY;
    if (measure && mine) {
        const double xx[6] = {px, p1x, py, p1y, pt, p1t};
        int n_pose = 0;
        cur = scene::score_obstacle(E, pA, pb, pv, ts, xx, 1, nullptr, D.n_sub, D.pool_v == nullptr, D.ego, &n_pose);
    }
    s_cur[w][lane] = cur;
    __syncthreads();

    // ---- finish, second half: fold, move the pool, advance, flag
    if (fin) {
        double c = INFINITY;
        if (measure)
            for (int j = 0; j < K; ++j) c = audit::min_nan(c, s_cur[w][j]);
        if (c != c) applied = false;
        if (!applied) {
            flag = OBCA_DONE_FAILED;
            if (lane == 0) D.flags[b] = flag;
        } else {
            if (pv) {
                double nb[scene::MAX_E];
#pragma unroll
                for (int r = 0; r < scene::MAX_E; ++r) nb[r] = r < E ? scene::row_b(pA, pb, pv, ts, r, 1) : 0.0;
#pragma unroll
                for (int r = 0; r < scene::MAX_E; ++r)
                    if (r < E) pb[r] = nb[r];
            }
            flag = poolloop::flag_after(D, kb, c, p1x, p1y, D.goal + 2 * b);
            if (lane < 3) {
                const double v = pick3(lane, p1x, p1y, p1t);
                D.x0[3 * b + lane] = v;
                D.x_closed[(b * (S + 1) + kb + 1) * 3 + lane] = v;
            }
            if (lane < 2) {
                const double v = lane == 0 ? ux : uy;
                D.u0[2 * b + lane] = v;
                D.u_closed[(b * S + kb) * 2 + lane] = v;
            }
            if (lane == 0) {
                if (measure) D.clear_hist[b * S + kb] = c;
                D.T_closed[b * S + kb] = ts;
                D.k[b] = kb + 1;
                D.flags[b] = flag;
            }
            px = p1x; py = p1y; pt = p1t;
        }
    }
    if (!live) return;

    // ---- start
    if (!solved) {
        const int len = D.path_len[b];
        flag = poolloop::flag_start(D, px, py, pt, len, D.goal + 2 * b);
        double* xc = D.x_closed + b * (S + 1) * 3;
        for (int q = lane; q < 3 * (S + 1); q += WAVE) xc[q] = q < 3 ? pick3(q, px, py, pt) : NAN;
        for (int q = lane; q < 2 * S; q += WAVE) D.u_closed[b * S * 2 + q] = 0.0;
        for (int q = lane; q < S; q += WAVE) {
            D.T_closed[b * S + q] = 0.0;
            D.status_hist[b * S + q] = 0;
            D.iters_hist[b * S + q] = 0;
            D.clear_hist[b * S + q] = INFINITY;
        }
        for (int q = lane; q < S * n_sel; q += WAVE) D.sel_hist[b * S * n_sel + q] = -1;
        if (lane < 2) D.u0[2 * b + lane] = 0.0;
        if (lane == 0) { D.k[b] = 0; D.flags[b] = flag; }
    }

    // ---- prepare
    if (flag != OBCA_RUN) {                                          // wave-uniform
        loop::mask_rollout_wave(D.variant_out, D.xref_out, b, N1, px, py, pt, lane);
        return;
    }
    double* xr = D.xref_out + b * 3 * N1;
    if (lane == 0) D.variant_out[b] = D.variant;
    const double* path = D.path + b * 3 * P;
    const int len = poolloop::safe_len(D.path_len[b], P);
    int bi;
    double bd = poolloop::window_search(path, P, len, px, py, lane, WAVE, &bi);
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const double od = __shfl_xor(bd, m, WAVE);
        const int oi = __shfl_xor(bi, m, WAVE);
        if (poolloop::window_beats(od, oi, bd, bi)) { bd = od; bi = oi; }
    }
    const int i0 = bi == INT32_MAX ? 0 : bi;
    for (int t = lane; t < N1; t += WAVE) {
        const int i = poolloop::window_point(i0, t, len);
        xr[t] = path[i]; xr[N1 + t] = path[P + i]; xr[2 * N1 + t] = path[2 * P + i];
    }
}

}  // namespace

extern "C" void obca_pool_loop_init(obca_pool_loop* d) {
    if (d) poolloop::init(d);
}

extern "C" int obca_pool_loop_advance(const obca_pool_loop* d, int32_t solved, int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (poolloop::args_check(d, solved) != 0 || device < 0) return OBCA_E_INVAL;
    const int64_t blocks = ((int64_t)d->B + PER_BLOCK - 1) / PER_BLOCK;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(poolloop_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, *d, solved);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
