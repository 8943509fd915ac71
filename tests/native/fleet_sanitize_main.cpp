// Stand-alone sanitizer run of the fleet core (csrc/obca_fleet_core.h through fleet_host.cpp) -- no test, run by hand:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/native/fleet_sanitize_main.cpp -o fleet_sanitize && ./fleet_sanitize
// Every buffer is a heap allocation of exactly the size the call may touch, so that a read or write one element outside it is
// reported.  The edge shapes (G, V, Ks): (1, 1, 0) the smallest, (1, 1, 63) and (1, 16, 48) the full pool of 64 slots,
// (3, 16, 0) the largest world, (2, 3, 2) with N = 127, S = 1024 and step = 1023 (the last history word), n_sub 0, 1 and 256;
// both see and predict modes; one car without a pose, one ended, one that did not step.  Prints "fleet sanitize ok" and
// returns 0 when the outputs are also what they must be.
#include <cmath>
#include <cstdio>
#include <vector>
#include "fleet_host.cpp"

static int run(int G, int V, int Ks, int N, int S, int step, int n_sub, int see, int predict) {
    const int B = G * V, K = Ks + V, N1 = N + 1;
    std::vector<double> xp((size_t)B * 3), x0((size_t)B * 3), u0((size_t)B * 2), pA((size_t)B * K * 8, 7.0), pb((size_t)B * K * 4, 7.0),
        pv((size_t)B * K * 2, 7.0), hist((size_t)B * S, -1.0), xr((size_t)B * 3 * N1, 2.0);
    std::vector<int> k(B, step + 1), flags(B, OBCA_RUN), vo(B, 8);
    for (int g = 0; g < G; ++g)
        for (int a = 0; a < V; ++a) {
            const int b = g * V + a;
            const double th = 0.4 * a - 1.0;
            x0[3 * b] = 3.0 * a; x0[3 * b + 1] = 5.0 + 0.1 * g; x0[3 * b + 2] = th;          // 3 m apart: neighbours overlap
            xp[3 * b] = x0[3 * b] - 0.5 * std::cos(th); xp[3 * b + 1] = x0[3 * b + 1] - 0.5 * std::sin(th); xp[3 * b + 2] = th - 0.05;
            u0[2 * b] = 0.5 + 0.1 * a; u0[2 * b + 1] = 0.1;
        }
    if (V > 2) { x0[3 * 1 + 1] = NAN; flags[2] = OBCA_DONE_GOAL; k[0] = step; }
    obca_fleet d;
    fleet_init_host(&d);
    d.G = G; d.V = V; d.Ks = Ks; d.N = N; d.max_steps = S; d.step = step; d.n_sub = n_sub; d.see = see; d.predict = predict;
    d.clearance = 0.0; d.margin = 0.25;
    d.x_prev = xp.data(); d.x0 = x0.data(); d.u0 = u0.data(); d.k = k.data(); d.flags = flags.data();
    d.pool_A = pA.data(); d.pool_b = pb.data(); d.pool_v = pv.data(); d.agent_clear_hist = hist.data(); d.xref_out = xr.data();
    d.variant_out = vo.data();
    if (fleet_step_host(&d, 0) != 0) return 1;
    for (double v : hist) if (v != -1.0) return 2;                            // a start measures nothing
    if (fleet_step_host(&d, 1) != 0) return 3;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < K; ++i) {
            const double* A = &pA[((size_t)b * K + i) * 8];
            if (i < Ks) { if (A[0] != 7.0 || pb[((size_t)b * K + i) * 4] != 7.0 || pv[((size_t)b * K + i) * 2] != 7.0) return 4; continue; }
            for (int r = 0; r < 4; ++r)
                if (!(std::fabs(std::hypot(A[2 * r], A[2 * r + 1]) - 1.0) < 1e-15) || !std::isfinite(pb[((size_t)b * K + i) * 4 + r])) return 5;
            if (!std::isfinite(pv[((size_t)b * K + i) * 2]) || !std::isfinite(pv[((size_t)b * K + i) * 2 + 1])) return 6;
            if (i - Ks == b % V && pb[((size_t)b * K + i) * 4] != -d.far) return 7;           // a car is no obstacle of itself
        }
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < S; ++q) {
            const double h = hist[(size_t)b * S + q];
            const bool moved = k[b] == step + 1;
            if (std::isnan(h)) return 8;
            if ((q != step || !moved || n_sub == 0) && h != -1.0) return 9;
            if (q == step && moved && n_sub > 0 && h == -1.0) return 10;
        }
    if (V > 3 && n_sub > 0 && flags[3] != OBCA_DONE_COLLISION) return 11;      // cars 3 and 4 overlap
    if (V > 2 && flags[2] != OBCA_DONE_GOAL) return 12;
    for (double v : xr) if (std::isnan(v)) return 13;
    return 0;
}

int main() {
    const int shapes[][9] = {{1, 1, 0, 1, 1, 0, 1, 0, 0},   {1, 1, 63, 5, 4, 3, 1, 1, 1},      {1, 16, 48, 5, 4, 0, 4, 0, 0},
                             {3, 16, 0, 5, 4, 2, 1, 1, 0},  {2, 3, 2, 127, 1024, 1023, 256, 0, 1}, {2, 5, 1, 5, 4, 1, 0, 1, 1}};
    for (const auto& s : shapes) {
        const int rc = run(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8]);
        if (rc != 0) { std::printf("shape G %d V %d Ks %d: %d\n", s[0], s[1], s[2], rc); return 1; }
    }
    // a refused call touches nothing: a wrong struct_size with every pointer NULL
    obca_fleet d;
    fleet_init_host(&d);
    d.struct_size -= 8;
    if (fleet_step_host(&d, 0) != fleet::E_INVAL) return 3;
    std::printf("fleet sanitize ok\n");
    return 0;
}
