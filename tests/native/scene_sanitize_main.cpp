// Stand-alone sanitizer run of the scene-pool core (csrc/obca_scene_core.h through scene_host.cpp) -- no test, run by hand:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/native/scene_sanitize_main.cpp -o scene_sanitize && ./scene_sanitize
// Every buffer is a heap allocation of exactly the size the call may touch, so that a read or write one element outside
// it is reported: K = 64, the largest N (127), E = 4, n_sel = 8, moving pool, both modes, one unusable instance and one
// that is not measured.  Prints "scene sanitize ok" and returns 0 when the outputs are also what they must be.
#include <cmath>
#include <cstdio>
#include <vector>
#include "scene_host.cpp"

int main() {
    const int B = 3, K = 64, E = 4, N = 127, n_sel = 8, n_sub = 3, N1 = N + 1;
    const double ego[4] = {1.7, 0.75, 1.7, 0.75};
    std::vector<double> pA((size_t)B * K * E * 2), pb((size_t)B * K * E), pv((size_t)B * K * 2), Ts(B), x((size_t)B * 3 * N1), x0((size_t)B * 3);
    std::vector<double> score((size_t)B * K), Ao((size_t)B * N1 * n_sel * E * 2), bo((size_t)B * N1 * n_sel * E), mc(B);
    std::vector<int> sel((size_t)B * n_sel), vo(B), ok(B), variant(B), status(B);
    unsigned long long s = 12345;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
    const double nx[4] = {1, 0, -1, 0}, ny[4] = {0, 1, 0, -1};
    for (int i = 0; i < B; ++i) {
        Ts[i] = 0.1 + rnd();
        variant[i] = i == 0 ? 4 : 6;
        status[i] = i == 2 ? 2 : 0;
        for (int k = 0; k < K; ++k) {
            const double cx = 140 * rnd(), cy = -10 + 20 * rnd(), h = 0.3 + rnd();
            for (int r = 0; r < E; ++r) {
                pA[(((size_t)i * K + k) * E + r) * 2] = nx[r];
                pA[(((size_t)i * K + k) * E + r) * 2 + 1] = ny[r];
                pb[((size_t)i * K + k) * E + r] = nx[r] * cx + ny[r] * cy + h;
            }
            pv[((size_t)i * K + k) * 2] = rnd() - 0.5;
            pv[((size_t)i * K + k) * 2 + 1] = rnd() - 0.5;
        }
        for (int k = 0; k < N1; ++k) {
            x[(size_t)i * 3 * N1 + k] = k;
            x[(size_t)i * 3 * N1 + N1 + k] = std::sin(0.05 * k);
            x[(size_t)i * 3 * N1 + 2 * N1 + k] = 0.05 * std::cos(0.05 * k);
        }
        x0[i * 3] = -0.5; x0[i * 3 + 1] = 0.2; x0[i * 3 + 2] = 0.0;
    }
    pb[((size_t)1 * K + 63) * E + 3] = NAN;                                   // instance 1 is unusable
    int rc = scene_select_host(ego, B, K, E, N, n_sel, n_sub, 0, pA.data(), pb.data(), pv.data(), Ts.data(), x.data(), x0.data(),
                               variant.data(), nullptr, score.data(), sel.data(), Ao.data(), bo.data(), vo.data(), ok.data(), mc.data());
    if (rc != 0 || ok[0] != 1 || ok[1] != 0 || ok[2] != 1 || vo[0] != 4 || vo[1] != 0 || vo[2] != 6) return 1;
    for (int k = 0; k < N1; ++k) x[(size_t)0 * 3 * N1 + N1 + k] += 0.7;      // a plan off the reference
    rc = scene_select_host(ego, B, K, E, N, n_sel, n_sub, 1, pA.data(), pb.data(), pv.data(), Ts.data(), x.data(), nullptr,
                           variant.data(), status.data(), score.data(), sel.data(), Ao.data(), bo.data(), vo.data(), ok.data(), mc.data());
    if (rc != 0 || ok[0] != 1 || ok[1] != 0 || ok[2] != 1 || vo[1] != 0 || vo[2] != 0 || !std::isnan(mc[2]) || std::isnan(mc[0])) return 2;
    for (double v : Ao) if (std::isnan(v)) return 3;
    for (double v : bo) if (std::isnan(v)) return 3;
    for (int q = 0; q < B * n_sel; ++q) if (sel[q] < 0 || sel[q] >= K) return 4;
    // the smallest shape as well: one obstacle of one row, one interval
    double a1[2] = {0.0, 1.0}, b1[1] = {-3.0}, x1[6] = {0, 1, 0, 0, 0, 0}, sc1[1], Ao1[4], bo1[2], mc1[1];
    int se1[1], vo1[1], ok1[1];
    rc = scene_select_host(ego, 1, 1, 1, 1, 1, 1, 0, a1, b1, nullptr, nullptr, x1, nullptr, nullptr, nullptr, sc1, se1, Ao1, bo1, vo1, ok1, mc1);
    if (rc != 0 || ok1[0] != 1 || se1[0] != 0 || std::fabs(sc1[0] - 2.25) > 1e-12) return 5;
    std::printf("scene sanitize ok\n");
    return 0;
}
