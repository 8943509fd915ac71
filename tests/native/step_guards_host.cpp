// CPU exercise of the structured core (csrc/obca_lpi_core.h) that also reports WHICH guard of the fraction-to-the-boundary rule
// set the step length of an iteration -- tests only (tests/test_gpu_guard_selects.py asserts on the host that its instances make
// every one of the eight guards bind, so that the select form of the kernels' row loop is exercised where it matters).
// Guard k: 0 / 1 lower / upper slack, 2 / 3 the elastic variables p / n (primal step a_max); 4 .. 7 their multipliers (a_z).
// A guard BINDS an iteration when the step length is below 1 and equals the smallest value that guard offered in it.
#include <math.h>

struct StepGuards { double best[8]; int bound[8]; };
static thread_local StepGuards* step_guards_now = nullptr;

static inline void step_guard(int k, double v) {
    StepGuards* g = step_guards_now;
    if (g) g->best[k] = fmin(g->best[k], v);
}
static inline void step_lengths(double a_max, double a_z) {
    StepGuards* g = step_guards_now;
    if (!g) return;
    for (int k = 0; k < 8; ++k) {
        const double a = k < 4 ? a_max : a_z;
        if (a < 1.0 && g->best[k] == a) ++g->bound[k];
        g->best[k] = INFINITY;
    }
}
#define OBCA_LPI_STEP_GUARD(k, v) step_guard(k, v)
#define OBCA_LPI_STEP_LENGTHS(a_max, a_z) step_lengths(a_max, a_z)
#include "lpi_host.cpp"

// bound [B, 8]: the number of iterations of instance i (all passes of its ladder) that guard k bound; the outputs are those of
// lpi_host_solve_batch
extern "C" int step_guards_solve_batch(int N, int n_obs, const int* m, const int* variant, int B,
                                       const double* x0, const double* u0, const double* xref, const double* A,
                                       const double* b, const double* Ts, const double* term, const HostParams* p,
                                       double* xopt, double* uopt, double* ts_opt, int* status, int* iters, double* info, int* bound) {
    for (int i = 0; i < B; ++i) {
        StepGuards g;
        for (int k = 0; k < 8; ++k) { g.best[k] = INFINITY; g.bound[k] = 0; }
        const int M = [&] { int s = 0; for (int j = 0; j < n_obs; ++j) s += m[j]; return s; }();
        const size_t N1 = (size_t)N + 1;
        step_guards_now = &g;
        const int rc = lpi_host_solve_batch(N, n_obs, m, variant + i, 1, x0 + 3 * i, u0 + 2 * i, xref + 3 * N1 * i, A + 2 * N1 * M * i,
                                            b + N1 * M * i, Ts + i, term + 3 * i, p, xopt + 3 * N1 * i, uopt + 2 * N * i, ts_opt + i,
                                            status + i, iters + i, info + 4 * i);
        step_guards_now = nullptr;
        if (rc) return rc;
        for (int k = 0; k < 8; ++k) bound[8 * i + k] = g.bound[k];
    }
    return 0;
}
