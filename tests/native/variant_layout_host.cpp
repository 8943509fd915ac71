// CPU restatement of the row layout for tests/test_variant_layout.py -- tests only.  Two sides of one comparison: the layout the
// host core builds at run time (csrc/obca_lpi_core.h: make_layout, the same sums as csrc/obca_kernel.hip: obca_ipm_body), and the
// constant layout and slot statements the one-wavefront compile-time-shape kernels' per-variant bodies are built from
// (csrc/obca_device.h: obca_row_layout, obca_slot_kinds, obca_own_mu_slot, obca_mixed_kinds), evaluated here by the host compiler.
#include "../../vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd/csrc/obca_lpi_core.h"

// out[15]: r_init, r_dyn, r_term, r_xb, r_ub, r_acc, r_T, r_tx, r_norm, r_dist, r_lam, r_mu, R, n, free_T
extern "C" void variant_layout_host_runtime(int N, int nO, int M, int variant, int* out) {
    lpi::Lay L;
    lpi::make_layout(L, N, nO, M, variant);
    const int f[15] = {L.r_init, L.r_dyn, L.r_term, L.r_xb, L.r_ub, L.r_acc, L.r_T, L.r_tx, L.r_norm, L.r_dist, L.r_lam, L.r_mu, L.R, L.n, L.free_T};
    for (int i = 0; i < 15; ++i) out[i] = f[i];
}
extern "C" void variant_layout_host_constant(int N, int nO, int M, int variant, int* out) {
    const ObcaRowLayout l = obca_row_layout(N, nO, M, variant);
    const int f[15] = {l.r_init, l.r_dyn, l.r_term, l.r_xb, l.r_ub, l.r_acc, l.r_T, l.r_tx, l.r_norm, l.r_dist, l.r_lam, l.r_mu, l.R, l.n, l.free_T};
    for (int i = 0; i < 15; ++i) out[i] = f[i];
}
extern "C" int variant_layout_host_slot_kinds(int N, int nO, int M, int variant, int nt, int j) { return obca_slot_kinds(N, nO, M, variant, nt, j); }
extern "C" int variant_layout_host_own_mu_slot(int N, int nO, int M, int variant, int nt) { return obca_own_mu_slot(N, nO, M, variant, nt); }
extern "C" int variant_layout_host_mixed_kinds(int N, int nO, int M, int variant, int nt) { return obca_mixed_kinds(N, nO, M, variant, nt); }

// the headline shape and the smallest one, as the compiler folds them
static_assert(obca_row_layout(5, 3, 6, 4).r_mu == 127 && obca_row_layout(5, 3, 6, 4).R == 199 && obca_row_layout(5, 3, 6, 6).R == 196 &&
              obca_row_layout(5, 3, 6, 8).R == 194 && obca_row_layout(5, 2, 2, 4).R == 139, "row counts of the listed shapes");
static_assert(obca_slot_kinds(5, 3, 6, 4, 64, 2) == OBCA_KIND_BIT_MU && obca_slot_kinds(5, 3, 6, 4, 64, 3) == OBCA_KIND_BIT_MU &&
              obca_slot_kinds(5, 3, 6, 4, 64, 4) == 0, "mu rounds of the headline shape");
