// Stand-alone sanitizer run of the pool-loop core (csrc/obca_poolloop_core.h through pool_loop_host.cpp) -- no test, run by
// hand:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/native/pool_loop_sanitize_main.cpp -o pool_loop_sanitize && ./pool_loop_sanitize
// Every buffer is a heap allocation of exactly the size the call may touch, so that a read or write one element outside it is
// reported.  Two shapes: the smallest (B = K = E = N = path_len = S = 1, no velocities, n_sel = 0) and B = 5, K = 64, E = 4,
// N = 127, path_max = path_len = 130, S = 3, n_sel = 8, a moving pool, driven to the cap by a scripted solver that answers
// with the window (one rollout starts with a bad path_len, one gets a failing status at step 1).  Prints
// "pool loop sanitize ok" and returns 0 when the outputs are also what they must be.
#include <cmath>
#include <cstdio>
#include <vector>
#include "pool_loop_host.cpp"

static int run(int B, int K, int E, int N, int P, int S, int n_sel, bool moving, int n_sub) {
    const int N1 = N + 1;
    std::vector<double> pA((size_t)B * K * E * 2), pv(moving ? (size_t)B * K * 2 : 0), goal((size_t)B * 2), path((size_t)B * 3 * P);
    std::vector<int> plen(B), status(B), iters(B), sel((size_t)B * n_sel), k(B), flags(B), sh((size_t)B * S), ih((size_t)B * S),
        selh((size_t)B * S * n_sel), vo(B);
    std::vector<double> ts(B), xopt((size_t)B * 3 * N1), uopt((size_t)B * 2 * N), x0((size_t)B * 3), u0((size_t)B * 2), pb((size_t)B * K * E),
        xc((size_t)B * (S + 1) * 3), uc((size_t)B * S * 2), Tc((size_t)B * S), ch((size_t)B * S), xr((size_t)B * 3 * N1);
    const double nx[4] = {1, 0, -1, 0}, ny[4] = {0, 1, 0, -1};
    unsigned long long s = 4321;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < K; ++i) {
            const double cx = 200 * rnd(), cy = 6 + 20 * rnd(), h = 0.3 + rnd();
            for (int r = 0; r < E; ++r) {
                pA[(((size_t)b * K + i) * E + r) * 2] = nx[r];
                pA[(((size_t)b * K + i) * E + r) * 2 + 1] = ny[r];
                pb[((size_t)b * K + i) * E + r] = nx[r] * cx + ny[r] * cy + h;
            }
            if (moving) { pv[((size_t)b * K + i) * 2] = rnd() - 0.5; pv[((size_t)b * K + i) * 2 + 1] = rnd() - 0.5; }
        }
        for (int i = 0; i < P; ++i) {
            path[(size_t)b * 3 * P + i] = 1.5 * i;
            path[(size_t)b * 3 * P + P + i] = 0.01 * i;
            path[(size_t)b * 3 * P + 2 * P + i] = 0.0;
        }
        plen[b] = P;
        goal[2 * b] = 1.5 * (P - 1); goal[2 * b + 1] = 0.01 * (P - 1);
        x0[3 * b] = -1.0; x0[3 * b + 1] = 0.0; x0[3 * b + 2] = 0.0;
    }
    if (B > 1) plen[B - 1] = P + 1;                                           // a bad path_len: FAILED at the start
    obca_pool_loop d;
    pool_loop_init_host(&d);
    d.B = B; d.K = K; d.E = E; d.N = N; d.n_sel = n_sel; d.path_max = P; d.max_steps = S; d.variant = moving ? 8 : 4; d.n_sub = n_sub;
    d.pool_A = pA.data(); d.pool_v = moving ? pv.data() : nullptr; d.goal = goal.data(); d.path = path.data(); d.path_len = plen.data();
    d.status = status.data(); d.iters = iters.data(); d.ts_opt = ts.data(); d.xopt = xopt.data(); d.uopt = uopt.data();
    d.sel = n_sel ? sel.data() : nullptr;
    d.x0 = x0.data(); d.u0 = u0.data(); d.pool_b = pb.data(); d.k = k.data(); d.flags = flags.data();
    d.x_closed = xc.data(); d.u_closed = uc.data(); d.T_closed = Tc.data(); d.status_hist = sh.data(); d.iters_hist = ih.data();
    d.clear_hist = ch.data(); d.sel_hist = n_sel ? selh.data() : nullptr; d.xref_out = xr.data(); d.variant_out = vo.data();
    if (pool_loop_advance_host(&d, 0) != 0) return 1;
    for (int b = 0; b < B; ++b) {
        const bool bad = B > 1 && b == B - 1;
        if (flags[b] != (bad ? OBCA_DONE_FAILED : OBCA_RUN) || k[b] != 0) return 2;
    }
    for (int step = 0; step < S; ++step) {
        for (int b = 0; b < B; ++b) {                                         // the scripted solver: the window is the plan
            for (int q = 0; q < 3 * N1; ++q) xopt[(size_t)b * 3 * N1 + q] = xr[(size_t)b * 3 * N1 + q];
            for (int q = 0; q < 2 * N; ++q) uopt[(size_t)b * 2 * N + q] = 0.25;
            ts[b] = 0.5; iters[b] = 7 + step;
            status[b] = (B > 2 && b == 1 && step == 1) ? 2 : 0;
            for (int q = 0; q < n_sel; ++q) sel[(size_t)b * n_sel + q] = q;
        }
        if (pool_loop_advance_host(&d, 1) != 0) return 3;
    }
    for (int b = 0; b < B; ++b) {
        const bool bad = B > 1 && b == B - 1, fails = B > 2 && b == 1 && S > 1;
        if (P == 1) { if (flags[b] != OBCA_DONE_CAP || k[b] != 1 || x0[3 * b] != 0.0) return 4; continue; }
        if (bad) { if (flags[b] != OBCA_DONE_FAILED || k[b] != 0 || vo[b] != 0) return 5; continue; }
        if (fails) { if (flags[b] != OBCA_DONE_FAILED || k[b] != 1 || sh[(size_t)b * S + 1] != 2) return 6; continue; }
        if (flags[b] != OBCA_DONE_CAP || k[b] != S || x0[3 * b] != 1.5 * S) return 7;
        for (int q = 0; q < S; ++q)
            if (!(ch[(size_t)b * S + q] > 0.0) || std::isinf(ch[(size_t)b * S + q])) return 8;
    }
    for (double v : xr) if (std::isnan(v)) return 9;
    for (double v : pb) if (std::isnan(v)) return 9;
    return 0;
}

int main() {
    int rc = run(1, 1, 1, 1, 1, 1, 0, false, 1);
    if (rc != 0) { std::printf("small shape: %d\n", rc); return 1; }
    rc = run(5, 64, 4, 127, 130, 3, 8, true, 4);
    if (rc != 0) { std::printf("large shape: %d\n", rc); return 2; }
    // a refused call touches nothing: a wrong struct_size with every pointer NULL
    obca_pool_loop d;
    pool_loop_init_host(&d);
    d.struct_size -= 8;
    if (pool_loop_advance_host(&d, 0) != scene::E_INVAL) return 3;
    std::printf("pool loop sanitize ok\n");
    return 0;
}
