// CPU exercise of the swept, inflated rows of moving boxes (rollout::moving_box_rows and sweep_h / sweep_r in
// csrc/obca_rollout_core.h) -- tests only.  The closed loop of rollout_stop_host.cpp with the option, the harness part
// of one step with it, and the host twin of obca_moving_rows_batch (csrc/obca_rows.hip); built into its own library so
// that the other shims stay as they are.
#include "rollout_stop_host.cpp"

// rollout_stop_host_run with swept rows (sweep_h = sweep_r = 0: off -- the same words as rollout_stop_host_run)
extern "C" int rollout_swept_host_run(const obca_rollout_dims* d, const double* start, const double* goal, const double* path,
                                      const int* path_len, const double* As, const double* bs, const double* dyn, double Ts0,
                                      double sense_dis, const HostParams* hp, int n_steps, int stop_nsub, double stop_clear,
                                      int certified, int exact, double sweep_h, double sweep_r, double* x_closed,
                                      double* u_closed, double* T_closed, double* x_openloop, int* variant_hist, int* iters_hist,
                                      int* status_hist, double* dyn_hist, int* steps, int* flags, double* clearance) {
    using namespace rollout;
    if ((sweep_h != 0.0 || sweep_r != 0.0) && !exact) return -22;         // as obca_rollouts_reset
    HostRollouts H(d, goal, path, path_len, As, bs, sense_dis, hp->ego, stop_nsub, stop_clear, certified, exact);
    Dev& D = H.D;
    D.sweep_h = sweep_h; D.sweep_r = sweep_r;
    const size_t B = D.B, S = D.S, nd = D.n_dyn, Nm1 = D.Nm + 1;
    for (int b = 0; b < D.B; ++b) reset(D, b, start, dyn, Ts0);
    for (int step = 0; step < n_steps; ++step) {
        for (int b = 0; b < D.B; ++b) prepare(D, b);
        for (int g = 0; g <= D.n_dyn; ++g) {
            int m[OBCA_MAX_OBST];
            for (int i = 0; i < d->n_static; ++i) m[i] = d->m_static[i];
            for (int i = 0; i < g; ++i) m[d->n_static + i] = 4;
            HostParams h6 = *hp;
            if (g > 0) h6.single_start = 1;
            int rc = lpi_host_solve_batch_warm(g == 0 ? D.N : D.Nf, d->n_static + g, m, D.var[g], D.B, D.x0, D.u0, g == 0 ? D.xref : D.xref_fix,
                                               D.A[g], D.b[g], D.Ts, D.term, &h6, D.xopt[g], D.uopt[g], D.ts[g], D.status[g], D.iters[g],
                                               nullptr, nullptr, nullptr, 0.0);
            if (rc) return rc;
            if (g == 0) continue;
            for (int b = 0; b < D.B; ++b) make_retry(D, g, b);
            rc = lpi_host_solve_batch_warm(D.Nf, d->n_static + g, m, D.var8[g], D.B, D.x0, D.u0, D.xref_fix, D.A[g], D.b[g], D.Ts, D.term,
                                           hp, D.xopt[g], D.uopt[g], D.ts[g], D.status8[g], D.iters8[g], nullptr, nullptr, nullptr, 0.0);
            if (rc) return rc;
        }
        for (int b = 0; b < D.B; ++b) { finish(D, b); stop_check(D, b); }
    }
    memcpy(x_closed, D.xc, sizeof(double) * B * (S + 1) * 3);
    memcpy(u_closed, D.uc, sizeof(double) * B * S * 2);
    memcpy(T_closed, D.Tc, sizeof(double) * B * S);
    memcpy(x_openloop, D.xol, sizeof(double) * B * S * 3 * Nm1);
    memcpy(variant_hist, D.vh, sizeof(int) * B * S);
    memcpy(iters_hist, D.ih, sizeof(int) * B * S);
    memcpy(status_hist, D.sh, sizeof(int) * B * S);
    if (nd) memcpy(dyn_hist, D.dh, sizeof(double) * B * S * nd * 4);
    memcpy(clearance, D.clr, sizeof(double) * B * S);
    for (int b = 0; b < D.B; ++b) { steps[b] = D.k[b]; flags[b] = D.flags[b]; }
    return 0;
}

// rollout_stop_host_rows with exact sensing and swept rows; the moving tuples as prepare() left them (centres advanced to
// step k) go to dyn_now [n_dyn,13]
extern "C" int rollout_swept_host_harness(const obca_rollout_dims* d, const double* start, const double* goal, const double* path,
                                          const int* path_len, const double* As, const double* bs, const double* dyn,
                                          double sense_dis, const double* ego, int k, double Ts_opt, const double* x0, int g,
                                          double sweep_h, double sweep_r, int* variant, double* A, double* b, double* dyn_now) {
    using namespace rollout;
    obca_rollout_dims d1 = *d;
    d1.batch = 1;
    HostRollouts H(&d1, goal, path, path_len, As, bs, sense_dis, ego, 0, 0.0, 0, 1);
    Dev& D = H.D;
    D.sweep_h = sweep_h; D.sweep_r = sweep_r;
    if (g < 0 || g > D.n_dyn) return -22;
    reset(D, 0, start, dyn, Ts_opt);
    D.k[0] = k; D.Ts_opt[0] = Ts_opt; D.flags[0] = OBCA_RUN;
    for (int j = 0; j < 3; ++j) D.x0[j] = x0[j];
    prepare(D, 0);
    const size_t Mg = D.Ms + 4 * g, Ng1 = (g == 0 ? D.N : D.Nf) + 1;
    *variant = D.var[g][0];
    memcpy(A, D.A[g], sizeof(double) * Ng1 * Mg * 2);
    memcpy(b, D.b[g], sizeof(double) * Ng1 * Mg);
    memcpy(dyn_now, D.dyn, sizeof(double) * D.n_dyn * DYN_W);
    return 0;
}

// host twin of obca_moving_rows_batch (include/obca_mpc.h): the same core function per (instance, stage, box)
extern "C" int rollout_swept_host_rows_batch(int B, int N, int Ms, int n_box, const double* static_A, const double* static_b,
                                             const double* boxes, const double* Ts, double half_window, double margin,
                                             double* A, double* b) {
    const size_t N1 = N + 1, M = Ms + 4 * n_box;
    for (size_t i = 0; i < (size_t)B; ++i)
        for (size_t kk = 0; kk < N1; ++kk) {
            double* Ak = A + (i * N1 + kk) * M * 2;
            double* bk = b + (i * N1 + kk) * M;
            for (int q = 0; q < 2 * Ms; ++q) Ak[q] = static_A[i * Ms * 2 + q];
            for (int q = 0; q < Ms; ++q) bk[q] = static_b[i * Ms + q];
            for (int j = 0; j < n_box; ++j)
                rollout::moving_box_rows(boxes + (i * n_box + j) * rollout::DYN_W, Ts[i], (int)kk, half_window, margin,
                                         Ak + 2 * (Ms + 4 * j), bk + Ms + 4 * j);
        }
    return 0;
}
