// Stand-alone sanitizer run of the host core of the plans measured against timed tracks (csrc/obca_plan_tracks_core.h through
// plan_tracks_host.cpp) -- no test, run by hand:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/native/plan_tracks_sanitize_main.cpp -o plan_tracks_sanitize && ./plan_tracks_sanitize
// Every buffer is a heap allocation of exactly the size the call may touch, so that a read or write one element outside it is
// reported.  Shapes (B, K, Kt, N, L, group, n_sub): (1, 1, 1, 1, 1, 1, 1) the smallest; (6, 18, 16, 127, 7, 3, 3) the longest
// horizon; (2, 64, 64, 5, 4, 2, 256) every slot tracked at the most samples; (3, 3, 2, 5, 4096, 1, 1) the longest track, full;
// (5, 4, 3, 5, 2, 1, 16) a ragged batch.  Every shape with score NULL and given, with t0 / x0 / variant / status given and NULL,
// and among the tracks a length of 0, lengths outside 1 .. L (whose knots must not be read: they lie beyond the block's end for
// the last track but one), a knot that is no number at the buffer's end, times that do not increase, a size that is no
// rectangle; among the plans a masked one, an infeasible one, one without a pose, one whose dt is no number.  Prints
// "plan tracks sanitize ok" and returns 0 when the outputs are also what they must be.
#include <cmath>
#include <cstdio>
#include <vector>
#include "plan_tracks_host.cpp"

static int run(int B, int K, int Kt, int N, int L, int group, int n_sub, bool with_score, bool with_opt) {
    const int Bt = B / group, N1 = N + 1;
    std::vector<double> tx((size_t)Bt * Kt * L * 3), tt((size_t)Bt * Kt * L), ts((size_t)Bt * Kt * 4), t0(B), dt(B), x((size_t)B * 3 * N1),
        x0((size_t)B * 3), score((size_t)B * K, 5.0), clear((size_t)B * Kt, -7.0), mn(B, -7.0);
    std::vector<int> len((size_t)Bt * Kt), variant(B, 8), status(B, 0), st((size_t)B * Kt, -7);
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
    const int last = Bt * Kt - 1;
    len[last] = L;                                                                 // the last track, full: its last knot is the buffer's end
    if (Kt > 1) {
        len[0] = 0;
        len[1] = L + 1;
        len[last - 1] = 2147483647;                                                // knots far beyond the buffer's end -- if they were read
        if (L > 1) tx[(size_t)last * L * 3 + 3 * (L - 1) + 2] = NAN;               // ... and no number
    }
    if (Bt * Kt > 6) { len[2] = -3; ts[4 * 4 + 1] = -0.75; if (L > 2) { len[5] = 3; tt[(size_t)5 * L + 2] = tt[(size_t)5 * L + 1]; } }
    for (int b = 0; b < B; ++b) {
        t0[b] = 0.25 * b - 0.5; dt[b] = 0.5 + 0.25 * (b % 3);
        for (int k = 0; k < N1; ++k) { x[(size_t)b * 3 * N1 + k] = 2.0 + b + 0.2 * k; x[(size_t)b * 3 * N1 + N1 + k] = 3.0 + 0.01 * k; x[(size_t)b * 3 * N1 + 2 * N1 + k] = 0.002 * k; }
        x0[3 * b] = 1.9 + b; x0[3 * b + 1] = 3.0; x0[3 * b + 2] = 0.0;
    }
    if (B > 1) variant[1] = 0;
    if (B > 2) { status[2] = 2; for (int k = 0; k < 3 * N1; ++k) x[k] = NAN; x0[1] = NAN; }
    if (B > 3) dt[3] = NAN;
    struct obca_plan_tracks d;
    plan_tracks_init_host(&d);
    d.B = B; d.K = K; d.Kt = Kt; d.N = N; d.L = L; d.group = group; d.n_sub = n_sub;
    d.track_x = tx.data(); d.track_t = tt.data(); d.track_len = len.data(); d.track_size = ts.data(); d.dt = dt.data(); d.x = x.data();
    if (with_opt) { d.t0 = t0.data(); d.x0 = x0.data(); d.variant = variant.data(); d.status = status.data(); }
    d.score = with_score ? score.data() : nullptr;
    d.track_clear = clear.data(); d.track_min = mn.data(); d.track_state = st.data();
    if (plan_tracks_host(&d) != 0) return 1;
    for (size_t q = 0; q < st.size(); ++q)
        if (st[q] < -1 || st[q] > 1) return 2;
    if (Kt > 1 && (st[0] != 0 || st[1] != -1 || st[(size_t)(B - 1) * Kt + Kt - 2] != -1)) return 3;
    if (Kt > 1 && L > 1 && st[(size_t)(B - 1) * Kt + Kt - 1] != -1) return 4;
    if (Bt * Kt > 6 && (st[2] != -1 || st[4] != -1 || (L > 2 && st[5] != -1))) return 5;
    if (B > 3)
        for (int j = 0; j < Kt; ++j) if (st[(size_t)3 * Kt + j] == 1) return 6;                   // no clock, no usable track
    for (int b = 0; b < B; ++b) {
        const bool masked = with_opt && ((B > 1 && b == 1) || (B > 2 && b == 2));
        const bool no_pose = B > 2 && b == 0;                                      // every pose NaN (x0 too, where it is given)
        const bool nan_row = masked || no_pose;
        if ((mn[b] != mn[b]) != nan_row) return 7;
        for (int j = 0; j < Kt; ++j) {
            const double c = clear[(size_t)b * Kt + j];
            if ((c != c) != nan_row || c == -7.0) return 8;
            if (!nan_row && st[(size_t)b * Kt + j] != 1 && c != INFINITY) return 9;
            if (!nan_row && st[(size_t)b * Kt + j] == 1 && !std::isfinite(c)) return 10;
            const double s = score[(size_t)b * K + (K - Kt) + j];
            if (!with_score || nan_row || st[(size_t)b * Kt + j] != 1) { if (s != 5.0) return 11; }
            else if (s != (c < 5.0 ? c : 5.0)) return 12;
        }
        for (int s = 0; s < K - Kt; ++s) if (score[(size_t)b * K + s] != 5.0) return 13;           // the static slots are never touched
    }
    return 0;
}

int main() {
    const int shapes[][7] = {{1, 1, 1, 1, 1, 1, 1}, {6, 18, 16, 127, 7, 3, 3}, {2, 64, 64, 5, 4, 2, 256}, {3, 3, 2, 5, 4096, 1, 1},
                             {5, 4, 3, 5, 2, 1, 16}};
    for (const auto& s : shapes)
        for (int with_score = 0; with_score < 2; ++with_score)
            for (int with_opt = 0; with_opt < 2; ++with_opt) {
                const int rc = run(s[0], s[1], s[2], s[3], s[4], s[5], s[6], with_score != 0, with_opt != 0);
                if (rc != 0) {
                    std::printf("B %d K %d Kt %d N %d L %d group %d n_sub %d score %d optional %d: %d\n", s[0], s[1], s[2], s[3], s[4], s[5],
                                s[6], with_score, with_opt, rc);
                    return 1;
                }
            }
    // refused calls touch nothing: a wrong struct_size with every pointer NULL, a Kt beyond K, a group that does not divide B
    struct obca_plan_tracks d;
    plan_tracks_init_host(&d);
    d.struct_size -= 8;
    if (plan_tracks_host(&d) != fleet::E_INVAL) return 3;
    plan_tracks_init_host(&d);
    d.B = 4; d.K = 2; d.Kt = 3; d.N = 5; d.L = 4; d.group = 1; d.n_sub = 1;
    if (plan_tracks_host(&d) != fleet::E_INVAL) return 4;
    d.Kt = 2; d.group = 3;
    if (plan_tracks_host(&d) != fleet::E_INVAL) return 5;
    std::printf("plan tracks sanitize ok\n");
    return 0;
}
