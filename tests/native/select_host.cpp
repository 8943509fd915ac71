// CPU exercise of the solver's kernel selection (csrc/obca_select.h) -- tests only.  The header is pure arithmetic; this file
// only flattens its structs into arrays of 64-bit integers for ctypes.
#include "../../vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd/csrc/obca_select.h"

namespace sel = obca_select;

extern "C" const char* select_kernel_name(int k) {
    static const char* const names[sel::K_COUNT] = {"wave r4", "wave r5", "wave r6", "wave shape", "mw r3", "mw r5", "mw shape", "gm", "gm1", "lane"};
    return k >= 0 && k < sel::K_COUNT ? names[k] : "?";
}

extern "C" int select_wave_row_slots(int rows) { return sel::wave_row_slots(rows); }
extern "C" int select_mw_row_slots(int rows) { return sel::mw_row_slots(rows); }

// out[13]: R_max, inst_off, lds_bytes, soc_lds, lds_bytes_mw, soc_lds_mw, lds_bytes_gm, gm_doubles, inst_off_gm, wave_ok, mw_ok, gm_ok, n_max
extern "C" void select_caps(int N, int nO, int M, long long* out) {
    const sel::Caps c = sel::caps(N, nO, M);
    const long long v[13] = {c.R_max, c.inst_off, c.lds_bytes, c.soc_lds, c.lds_bytes_mw, c.soc_lds_mw, c.lds_bytes_gm, c.gm_doubles,
                             c.inst_off_gm, c.wave_ok, c.mw_ok, c.gm_ok, c.n_max};
    for (int i = 0; i < 13; ++i) out[i] = v[i];
}

// n cases of in[11]: N, nO, M, mode, specialise, has_wave_shape, has_mw_shape, two_sided, lds_pad, gm_ws_failed, refused
// -> out[10]: rc, kernel, threads, lds, inst_off, soc_lds, two_sided, needs_ws, specialised, mode_available(mode)
extern "C" void select_plans(int n, const long long* in, long long* out) {
    for (int i = 0; i < n; ++i, in += 11, out += 10) {
        const sel::Caps c = sel::caps((int)in[0], (int)in[1], (int)in[2]);
        const sel::Knobs k{(int)in[3], in[4] != 0, in[5] != 0, in[6] != 0, (int)in[7], in[8], in[9] != 0};
        const sel::Plan p = sel::plan(c, k, (unsigned)in[10]);
        const long long v[10] = {p.rc, p.kernel, p.threads, p.lds, p.inst_off, p.soc_lds, p.two_sided, p.needs_ws, p.specialised,
                                 sel::mode_available(c, (unsigned)in[10], (int)in[3])};
        for (int j = 0; j < 10; ++j) out[j] = v[j];
    }
}

// the selection is usable at compile time (as obca_shape_sizes is)
static_assert(sel::caps(5, 3, 6).R_max == 199 && sel::caps(5, 3, 6).gm_doubles == 6478, "caps");
static_assert(sel::plan(sel::caps(5, 3, 6), sel::Knobs{0, false, false, false, -1, 0, false}, 0).kernel == sel::K_WAVE_R4, "plan");
