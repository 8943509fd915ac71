// Stand-alone sanitizer run of the host core of the obstacles on timed tracks (csrc/obca_pool_tracks_core.h through
// pool_tracks_host.cpp) -- no test, run by hand:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/native/pool_tracks_sanitize_main.cpp -o pool_tracks_sanitize && ./pool_tracks_sanitize
// Every buffer is a heap allocation of exactly the size the call may touch, so that a read or write one element outside it is
// reported.  Shapes (B, K, Kt, N, L, group, n_sub): (1, 1, 1, 1, 1, 1, 0) the smallest; (6, 18, 16, 127, 7, 3, 16) the longest
// horizon; (2, 64, 64, 5, 4, 2, 256) every slot tracked at the most samples; (3, 3, 2, 5, 4096, 1, 1) the longest track, full.
// Every shape with measure 0 and 1, all three predictions, t0 given and NULL, and among the tracks a length of 0, lengths
// outside 1 .. L (whose knots must not be read: they lie beyond the block's end for the last track), a knot that is no number,
// times that do not increase, a size that is no rectangle; among the rollouts one that did not step, one ended, one without a
// pose, one whose Ts is no number.  Prints "pool tracks sanitize ok" and returns 0 when the outputs are also what they must be.
#include <cmath>
#include <cstdio>
#include <vector>
#include "pool_tracks_host.cpp"

static int run(int B, int K, int Kt, int N, int L, int group, int n_sub, int predict, int measure, bool with_t0) {
    const int Bt = B / group, N1 = N + 1, S = 3, step = 1;
    std::vector<double> tx((size_t)Bt * Kt * L * 3), tt((size_t)Bt * Kt * L), ts((size_t)Bt * Kt * 4), t0(B), Ts(B), xp((size_t)B * 3),
        x0((size_t)B * 3), pA((size_t)B * K * 8, -7.0), pb((size_t)B * K * 4, -7.0), pv((size_t)B * K * 2, -7.0),
        sA((size_t)B * Kt * N1 * 8, -7.0), sb((size_t)B * Kt * N1 * 4, -7.0), hist((size_t)B * S, -7.0), xr((size_t)B * 3 * N1, -7.0);
    std::vector<int> len((size_t)Bt * Kt), k(B, step + 1), flags(B, OBCA_RUN), sok((size_t)B * Kt, -7), st((size_t)B * Kt, -7), vo(B, 8);
    for (int q = 0; q < Bt * Kt; ++q) {
        const double th0 = 0.37 * (q % 17) - 3.0;
        for (int i = 0; i < L; ++i) {
            const size_t o = (size_t)q * L + i;
            tt[o] = -1.0 + 0.5 * i + 0.125 * (i % 3);
            tx[3 * o] = 3.0 + 2.0 * (q % 11) + 0.01 * i * std::cos(th0);
            tx[3 * o + 1] = 4.0 + 0.01 * i * std::sin(th0);
            tx[3 * o + 2] = th0 + 0.001 * i;
        }
        ts[4 * q] = 1.7; ts[4 * q + 1] = 0.75; ts[4 * q + 2] = 1.7; ts[4 * q + 3] = 0.75;
        len[q] = 1 + q % L;
    }
    len[(size_t)Bt * Kt - 1] = L;                                                  // the last track, full: its last knot is the buffer's end
    if (Kt > 1) {
        len[0] = 0;
        len[1] = L + 1;
        if (L > 1) { tx[(size_t)(Bt * Kt - 1) * L * 3 + 3 * (L - 1) + 2] = NAN; }  // ... and no number
    }
    if (Bt * Kt > 5) { len[2] = -3; len[3] = 2147483647; ts[4 * 4 + 1] = -0.75; if (L > 2) { len[5] = 3; tt[(size_t)5 * L + 2] = tt[(size_t)5 * L + 1]; } }
    for (int b = 0; b < B; ++b) {
        t0[b] = 0.25 * b - 0.5; Ts[b] = 0.5 + 0.25 * (b % 3);
        for (int c = 0; c < 3; ++c) { xp[3 * b + c] = 2.0 + b + 0.1 * c; x0[3 * b + c] = 2.3 + b + 0.1 * c; }
    }
    if (B > 1) k[1] = step;
    if (B > 2) { flags[2] = OBCA_DONE_GOAL; x0[3 * 0 + 1] = NAN; }
    if (B > 3) Ts[3] = NAN;
    struct obca_pool_tracks d;
    pool_tracks_init_host(&d);
    d.B = B; d.K = K; d.Kt = Kt; d.N = N; d.L = L; d.group = group; d.max_steps = S; d.step = step; d.n_sub = n_sub; d.predict = predict;
    d.margin = 0.25; d.clearance = 0.1;
    d.track_x = tx.data(); d.track_t = tt.data(); d.track_len = len.data(); d.track_size = ts.data(); d.t0 = with_t0 ? t0.data() : nullptr;
    d.Ts = Ts.data(); d.x_prev = xp.data(); d.x0 = x0.data(); d.k = k.data(); d.flags = flags.data(); d.pool_A = pA.data(); d.pool_b = pb.data();
    d.pool_v = pv.data(); d.stage_A = sA.data(); d.stage_b = sb.data(); d.stage_ok = sok.data(); d.track_state = st.data();
    d.track_clear_hist = hist.data(); d.xref_out = xr.data(); d.variant_out = vo.data();
    if (pool_tracks_host(&d, measure) != 0) return 1;
    for (double v : sA) if (!std::isfinite(v) || v == -7.0) return 2;
    for (double v : sb) if (!std::isfinite(v) || v == -7.0) return 3;
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < K; ++s) {
            const bool tracked = s >= K - Kt;
            for (int r = 0; r < 4; ++r) {
                const double v = pb[((size_t)b * K + s) * 4 + r];
                if (tracked ? (!std::isfinite(v) || v == -7.0) : v != -7.0) return 4;   // the static slots are never touched
            }
            for (int r = 0; r < 2; ++r) {
                const double v = pv[((size_t)b * K + s) * 2 + r];
                if (tracked ? (!std::isfinite(v) || v == -7.0) : v != -7.0) return 5;
                if (tracked && predict == OBCA_TRACK_PREDICT_STATIC && v != 0.0) return 6;
            }
        }
    for (size_t q = 0; q < st.size(); ++q) {
        if (st[q] < -1 || st[q] > 1) return 7;
        if (sok[q] != ((st[q] == 1 && predict == OBCA_TRACK_PREDICT_TRACK) ? 1 : 0)) return 8;
    }
    if (Kt > 1 && (st[0] != 0 || st[1] != -1)) return 9;
    if (Bt * Kt > 5 && (st[2] != -1 || st[3] != -1 || st[4] != -1 || (L > 2 && st[5] != -1))) return 10;
    if (B > 3)
        for (int j = 0; j < Kt; ++j) if (st[(size_t)3 * Kt + j] == 1) return 11;                  // no clock, no usable track
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s) {
            const double v = hist[(size_t)b * S + s];
            const bool want = measure && n_sub > 0 && s == step && k[b] == step + 1;
            if (v != v) return 12;
            if (!want && v != -7.0) return 13;
        }
    for (double v : xr) if (v != v) return 14;
    return 0;
}

int main() {
    const int shapes[][7] = {{1, 1, 1, 1, 1, 1, 0}, {6, 18, 16, 127, 7, 3, 16}, {2, 64, 64, 5, 4, 2, 256}, {3, 3, 2, 5, 4096, 1, 1},
                             {5, 4, 3, 5, 2, 1, 1}};
    for (const auto& s : shapes)
        for (int predict = 0; predict < 3; ++predict)
            for (int measure = 0; measure < 2; ++measure)
                for (int with_t0 = 0; with_t0 < 2; ++with_t0) {
                    const int rc = run(s[0], s[1], s[2], s[3], s[4], s[5], s[6], predict, measure, with_t0 != 0);
                    if (rc != 0) {
                        std::printf("B %d K %d Kt %d N %d L %d group %d n_sub %d predict %d measure %d t0 %d: %d\n", s[0], s[1], s[2], s[3],
                                    s[4], s[5], s[6], predict, measure, with_t0, rc);
                        return 1;
                    }
                }
    // refused calls touch nothing: a wrong struct_size with every pointer NULL, a Kt beyond K, a group that does not divide B
    struct obca_pool_tracks d;
    pool_tracks_init_host(&d);
    d.struct_size -= 8;
    if (pool_tracks_host(&d, 0) != fleet::E_INVAL) return 3;
    pool_tracks_init_host(&d);
    d.B = 4; d.K = 2; d.Kt = 3; d.N = 5; d.L = 4; d.group = 1; d.max_steps = 2;
    if (pool_tracks_host(&d, 0) != fleet::E_INVAL) return 4;
    d.Kt = 2; d.group = 3;
    if (pool_tracks_host(&d, 0) != fleet::E_INVAL) return 5;
    std::printf("pool tracks sanitize ok\n");
    return 0;
}
