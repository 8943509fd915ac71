// CPU exerciser for tests/test_mu_entry.py -- tests only.  Two sides of one comparison: the entry of x a mu row reads as the host
// core finds it at run time (csrc/obca_lpi_core.h: make_layout, then row_value and row_jdx themselves on vectors whose entry t
// holds t, so that the value returned IS the entry read), and the constant the per-variant bodies of the one-wavefront
// compile-time-shape kernels index S.dx / S.xt with (csrc/obca_device.h: obca_mu_entry), evaluated here by the host compiler.
#include <vector>
#include "../../vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd/csrc/obca_lpi_core.h"

// out[0]: the entry row_value reads for row r, out[1]: the entry row_jdx reads; returns the number of variables, -1: r is no mu row
extern "C" int mu_entry_host_runtime(int N, int nO, int M, int variant, int r, int* out) {
    lpi::Lay L;
    lpi::make_layout(L, N, nO, M, variant);
    if (r < L.r_mu || r >= L.R) return -1;
    std::vector<double> idx(L.n), twice(L.n);
    for (int t = 0; t < L.n; ++t) { idx[t] = t; twice[t] = 2.0 * t; }
    lpi::Sh S{};
    lpi::Inst in{};
    in.Ts = 1.0;
    const lpi::SP xv{idx.data(), 1}, dv{twice.data(), 1}, none{nullptr, 1};
    out[0] = (int)lpi::row_value(L, S, in, xv, none, none, none, r);        // (a mu row reads neither the geometry nor S)
    S.x = xv; S.dx = dv;
    out[1] = (int)(lpi::row_jdx(L, S, in, r) / 2.0);                        // the step's entry, not the iterate's
    return L.n;
}
extern "C" int mu_entry_host_constant(int N, int nO, int M, int variant, int nt, int j, int lane) { return obca_mu_entry(N, nO, M, variant, nt, j, lane); }
extern "C" int mu_entry_host_own_mu_slot(int N, int nO, int M, int variant, int nt) { return obca_own_mu_slot(N, nO, M, variant, nt); }
extern "C" int mu_entry_host_mu_slot(int N, int nO, int M, int nt) { return obca_mu_slot(N, nO, M, nt); }

// the headline shape as the compiler folds it: row 128 of obca_mpc4 is the second mu row of stage 0 (stage stride 23, lambda at 5 .. 10,
// mu at 11 .. 22), the last row 198 the last mu entry of stage 5 (which has no input: 5 * 23 + 3 + 6 + 11 = 135, n = 137 with Topt)
static_assert(obca_mu_entry(5, 3, 6, 4, 64, 2, 0) == 12 && obca_mu_entry(5, 3, 6, 4, 64, 3, 6) == 135, "mu entries of the headline shape");
static_assert(obca_mu_entry(5, 3, 6, 8, 64, 2, 0) == 17 && obca_mu_entry(5, 3, 6, 8, 64, 3, 1) == 135, "mu entries under obca_mpc8");
