// Stand-alone sanitizer run of the two host cores of the fleet's prediction by plans (csrc/obca_fleet_tracks_core.h through
// fleet_tracks_host.cpp, the staged functions of csrc/obca_scene_core.h through staged_select_host.cpp) -- no test, run by hand:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/native/fleet_tracks_sanitize_main.cpp -o fleet_tracks_sanitize && ./fleet_tracks_sanitize
// Every buffer is a heap allocation of exactly the size the call may touch, so that a read or write one element outside it is
// reported.  Tracks, (G, V, N): (1, 1, 1) the smallest, (2, 16, 127) the largest world at the longest horizon, (3, 3, 5); both
// see modes; one car ended, one that did not step, one without a pose, one plan with a word that is no number.  Staged select,
// fed with those tracks (stage_group = V, Kt = V) and on its own edges: K = Kt = 64, Kt = 0 with NULL stage pointers, E = 1,
// N = 127 with n_sub = 256, both accumulate modes.  Prints "fleet tracks sanitize ok" and returns 0 when the outputs are also
// what they must be.
#include <cmath>
#include <cstdio>
#include <vector>
#include "fleet_tracks_host.cpp"
#include "staged_select_host.cpp"

static const double EGO[4] = {1.7, 0.75, 1.7, 0.75};

// the tracks of a fleet, then one staged select per car against them: Ks static slots and the V agent slots
static int run_fleet(int G, int V, int N, int see, int Ks) {
    const int B = G * V, N1 = N + 1, K = Ks + V, step = 2, n_sel = K < 3 ? K : 3;
    std::vector<double> x0((size_t)B * 3), xo((size_t)B * 3 * N1), tA((size_t)B * N1 * 8, -7.0), tb((size_t)B * N1 * 4, -7.0);
    std::vector<int> flags(B, OBCA_RUN), k(B, step + 1), status(B, 0), tok((size_t)B * V, -7);
    for (int q = 0; q < B; ++q) {
        const double th = 0.3 * (q % V) - 1.0;
        for (int t = 0; t < N1; ++t) {
            xo[(size_t)q * 3 * N1 + t] = 4.0 * (q % V) + 0.3 * t * std::cos(th);
            xo[(size_t)q * 3 * N1 + N1 + t] = 5.0 + 0.1 * (q / V) + 0.3 * t * std::sin(th);
            xo[(size_t)q * 3 * N1 + 2 * N1 + t] = th + 0.01 * t;
        }
        for (int c = 0; c < 3; ++c) x0[3 * q + c] = xo[(size_t)q * 3 * N1 + c * N1 + 1];
    }
    if (V > 2) { flags[1] = OBCA_DONE_GOAL; k[2] = step; x0[3 * (B - 1) + 1] = NAN; status[B - 2] = 2; xo[(size_t)3 * N1 - 1] = INFINITY; }
    struct obca_fleet_tracks d;
    fleet_tracks_init_host(&d);
    d.G = G; d.V = V; d.N = N; d.step = step; d.see = see; d.margin = 0.25;
    d.x0 = x0.data(); d.flags = flags.data(); d.k = k.data(); d.xopt = xo.data(); d.status = status.data();
    d.track_A = tA.data(); d.track_b = tb.data(); d.track_ok = tok.data();
    if (fleet_tracks_host(&d) != 0) return 1;
    for (double v : tA) if (!std::isfinite(v) || v == -7.0) return 2;
    for (double v : tb) if (!std::isfinite(v) || v == -7.0) return 3;
    for (int a = 0; a < B; ++a)
        for (int j = 0; j < V; ++j) {
            const int w = tok[(size_t)a * V + j];
            if (w != 0 && w != 1) return 4;
            if (j == a % V && w != 0) return 5;                                     // a car is no obstacle of itself
            if (see == OBCA_FLEET_SEE_LOWER && j > a % V && w != 0) return 6;
        }
    if (V > 2 && (tok[(size_t)2 * V + 1] != 0 || tok[(size_t)1 * V + 0] != 0 || tok[(size_t)1 * V + 2] != 0)) return 7;   // ended, NaN plan, did not step

    // the pools: static slots far below the cars, the agent slots the tracks' stage 0 (what obca_fleet_step writes)
    std::vector<double> pA((size_t)B * K * 8), pb((size_t)B * K * 4), pv((size_t)B * K * 2, 0.1), Ts(B, 1.5), x((size_t)B * 3 * N1),
        score((size_t)B * K, -1.0), Ao((size_t)B * N1 * n_sel * 8, -7.0), bo((size_t)B * N1 * n_sel * 4, -7.0), mc(B, -7.0);
    std::vector<int> sel((size_t)B * n_sel, -7), vo(B, -7), ok(B, -7), var(B, 8);
    const double box[8] = {0, 1, 1, 0, 0, -1, -1, 0};
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < K; ++i)
            for (int r = 0; r < 4; ++r) {
                const size_t o = ((size_t)b * K + i) * 4 + r;
                if (i < Ks) { pA[2 * o] = box[2 * r]; pA[2 * o + 1] = box[2 * r + 1]; pb[o] = (r == 0 ? -20.0 - i : r == 2 ? 22.0 + i : 3.0 + i); }
                else {
                    const size_t t = (((size_t)(b / V) * V + (i - Ks)) * N1) * 4 + r;
                    pA[2 * o] = tA[2 * t]; pA[2 * o + 1] = tA[2 * t + 1]; pb[o] = tb[t];
                }
            }
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < N1; ++t) { x[(size_t)b * 3 * N1 + t] = 0.5 * t; x[(size_t)b * 3 * N1 + N1 + t] = 2.0; x[(size_t)b * 3 * N1 + 2 * N1 + t] = 0.0; }
    for (int acc = 0; acc < 2; ++acc) {
        if (scene_select_staged_host(EGO, B, K, 4, N, n_sel, 2, acc, pA.data(), pb.data(), pv.data(), Ts.data(), x.data(), x0.data(),
                                     var.data(), status.data(), V, V, tA.data(), tb.data(), tok.data(), score.data(), sel.data(),
                                     Ao.data(), bo.data(), vo.data(), ok.data(), mc.data()) != 0) return 8;
        for (int b = 0; b < B; ++b) {
            if (ok[b] != 1) return 9;                                               // an x0 without a pose is skipped, the window counts
            for (int s = 0; s < n_sel; ++s)
                if (sel[(size_t)b * n_sel + s] < 0 || sel[(size_t)b * n_sel + s] >= K) return 10;
        }
        for (double v : Ao) if (!std::isfinite(v) || v == -7.0) return 11;
        for (double v : bo) if (!std::isfinite(v) || v == -7.0) return 12;
    }
    return 0;
}

// the staged select on its own edges: tracks that turn, every slot staged or none
static int run_select(int B, int K, int Kt, int E, int N, int n_sub, int group) {
    const int N1 = N + 1, n_sel = K < 8 ? K : 8, blocks = B / group;
    std::vector<double> pA((size_t)B * K * E * 2), pb((size_t)B * K * E), x((size_t)B * 3 * N1), sA((size_t)blocks * Kt * N1 * E * 2),
        sb((size_t)blocks * Kt * N1 * E), score((size_t)B * K, -1.0), Ao((size_t)B * N1 * n_sel * E * 2, -7.0),
        bo((size_t)B * N1 * n_sel * E, -7.0), mc(B, -7.0);
    std::vector<int> sok((size_t)B * Kt, 1), sel((size_t)B * n_sel, -7), vo(B, -7), ok(B, -7);
    for (size_t q = 0; q < pb.size(); ++q) {
        const double phi = 0.7 * (double)(q % 9);
        pA[2 * q] = std::cos(phi); pA[2 * q + 1] = std::sin(phi); pb[q] = -3.0 - 0.37 * (double)(q % 17);
    }
    for (size_t q = 0; q < sb.size(); ++q) {
        const double phi = 0.01 * (double)(q / E % N1) + 1.57 * (double)(q % E);
        sA[2 * q] = std::cos(phi); sA[2 * q + 1] = std::sin(phi); sb[q] = -2.0 - 0.11 * (double)(q % 23);
    }
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < N1; ++t) { x[(size_t)b * 3 * N1 + t] = 0.1 * t; x[(size_t)b * 3 * N1 + N1 + t] = 0.3 * b; x[(size_t)b * 3 * N1 + 2 * N1 + t] = 0.02 * t; }
    for (int acc = 0; acc < 2; ++acc) {
        if (scene_select_staged_host(EGO, B, K, E, N, n_sel, n_sub, acc, pA.data(), pb.data(), nullptr, nullptr, x.data(), nullptr, nullptr,
                                     nullptr, Kt, group, Kt ? sA.data() : nullptr, Kt ? sb.data() : nullptr, Kt ? sok.data() : nullptr,
                                     score.data(), sel.data(), Ao.data(), bo.data(), vo.data(), ok.data(), mc.data()) != 0) return 1;
        for (int b = 0; b < B; ++b) if (ok[b] != 1 || !std::isfinite(mc[b])) return 2;
        for (double v : Ao) if (!std::isfinite(v) || v == -7.0) return 3;
        for (double v : bo) if (!std::isfinite(v) || v == -7.0) return 4;
        for (double v : score) if (!std::isfinite(v) || v == -1.0) return 5;
    }
    return 0;
}

int main() {
    const int fleets[][5] = {{1, 1, 1, 0, 0}, {2, 16, 127, 1, 48}, {3, 3, 5, 0, 2}, {3, 3, 5, 1, 0}, {1, 16, 1, 0, 0}};
    for (const auto& s : fleets) {
        const int rc = run_fleet(s[0], s[1], s[2], s[3], s[4]);
        if (rc != 0) { std::printf("fleet G %d V %d N %d see %d Ks %d: %d\n", s[0], s[1], s[2], s[3], s[4], rc); return 1; }
    }
    const int selects[][7] = {{1, 64, 64, 4, 5, 1, 1}, {4, 64, 16, 4, 5, 16, 2}, {5, 4, 0, 4, 5, 2, 1}, {2, 1, 1, 1, 1, 1, 2}, {1, 3, 2, 3, 127, 256, 1}};
    for (const auto& s : selects) {
        const int rc = run_select(s[0], s[1], s[2], s[3], s[4], s[5], s[6]);
        if (rc != 0) { std::printf("select B %d K %d Kt %d E %d N %d: %d\n", s[0], s[1], s[2], s[3], s[4], rc); return 1; }
    }
    // refused calls touch nothing: a wrong struct_size with every pointer NULL, a Kt beyond K
    struct obca_fleet_tracks d;
    fleet_tracks_init_host(&d);
    d.struct_size -= 8;
    if (fleet_tracks_host(&d) != fleet::E_INVAL) return 3;
    if (scene::staged_args_check(4, 4, 5, 1, nullptr, nullptr, nullptr) != scene::E_INVAL) return 4;
    std::printf("fleet tracks sanitize ok\n");
    return 0;
}
