// obca_select.h -- which solver kernel a handle launches, and with what: the ONE place on the host that knows the row-slot
// limits, the LDS budget and the auto-mode rule.  Pure functions of numbers (no HIP; tests/native/select_host.cpp runs them on
// the CPU); csrc/obca_capi.hip and csrc/obca_rollout.hip map the answer to a function pointer and launch it.
#ifndef OBCA_SELECT_H
#define OBCA_SELECT_H

#include "obca_device.h"

namespace obca_select {

/* Row slots per thread: the one-wavefront kernels (_r4 / _r5 / _r6, also the fused closed loop's) hold up to 64 x 4 / 5 / 6 rows
   in registers, the four-wavefront LDS kernels 256 x 3 (_mw_r3) or 256 x 4 plus a fifth slot in LDS (_mw_r5: Rows<-5>);
   0 = beyond the family.  The kernels' own copy of these numbers: ShapeIs in csrc/obca_kernel.hip. */
constexpr int wave_row_slots(int rows) { return rows <= 256 ? 4 : rows <= 320 ? 5 : rows <= 384 ? 6 : 0; }
constexpr int mw_row_slots(int rows) { return rows <= 768 ? 3 : rows <= 1280 ? -5 : 0; }

/* One value per kernel family obca_solve_batch can launch */
enum Kernel { K_WAVE_R4, K_WAVE_R5, K_WAVE_R6, K_WAVE_SHAPE, K_MW_R3, K_MW_R5, K_MW_SHAPE, K_GM, K_GM1, K_LANE, K_COUNT };
constexpr Kernel wave_kernel(int rows) { return wave_row_slots(rows) == 4 ? K_WAVE_R4 : wave_row_slots(rows) == 5 ? K_WAVE_R5 : K_WAVE_R6; }
constexpr Kernel mw_kernel(int rows) { return mw_row_slots(rows) == 3 ? K_MW_R3 : K_MW_R5; }

/* Carve-up of the HBM-workspace kernels (GM branch of obca_ipm_body's carve-up; the LDS-resident one: obca_shape_sizes): what
   stays in LDS (the O(N) blocks of the stage-serial sweep), where the instance block starts there, and the doubles of HBM
   workspace one workgroup takes (the row state and every O(rows) array) */
struct GmSizes { long long lds_doubles; int inst_off; long long ws_doubles; };
constexpr GmSizes gm_sizes(int N, int nO, int M) {
    const int N1 = N + 1, np = N1 * nO, MW = OBCA_MAX_EDGES + 6;
    const int n_max = obca_shape_sizes(N, nO, M).n_max, R_max = obca_shape_sizes(N, nO, M).R_max;
    long long t = 0, g = 0;                                                                                  // LDS, workspace
    g += obca_even(n_max) + obca_even(n_max > 120 ? n_max : 120); t += obca_even(5 * N1 + 1); g += obca_even(n_max);
    g += 5 * obca_even(R_max);
    t += obca_even(3 * N1 + 3);
    t += 4 * obca_even(N1); g += 2 * obca_even(2 * np);
    g += 3 * obca_even(2 * np);
    g += obca_even(N1 * M * 2) + obca_even(N1 * M); t += obca_even(3 * N1);
    t += obca_even(36 * N1) + obca_even(8 * N1);
    {
        const long long nx = obca_even(n_max), nr = obca_even(R_max), ny = (long long)MW * 4 * np;
        g += obca_even(ny > nx + nr ? ny : nx + nr);
    }
    t += obca_even(36 * N1); g += obca_even(12 * np);
    t += obca_even(6 * N1) + obca_even(12 * N1) + obca_even(2 * N1) + obca_even(9 * (N1 + 1));
    t += obca_even(120);                                                                                     // FG / Mall / mall
    t += obca_even(32) + obca_even(8);
    t += 2 * obca_even(3 * N1 + 3) + obca_even(2 * N1 + 2);         // mirrors of the soft rows' E^-1, ghat; inputs + time scale
    g += 15 * obca_even((long long)((R_max + 255) / 256) * 256);    // row state (OBCA_ROW_FIELDS)
    return GmSizes{t + obca_even(OBCA_INST_DOUBLES), (int)t, g};
}

/* What follows from the shape alone, before the runtime is asked anything.  lds_bytes / lds_bytes_mw include the scratch of
   the second-order correction where it lives in LDS (soc_lds / soc_lds_mw != 0: its offset there); *_ok: the family's row
   slots and one CU's LDS hold the shape. */
struct Caps {
    int N, n_obs, n_max, R_max, inst_off, inst_off_gm, soc_lds, soc_lds_mw;
    long long lds_bytes, lds_bytes_mw, lds_bytes_gm, gm_doubles;
    bool wave_ok, mw_ok, gm_ok;
};
constexpr bool fits_cu(long long dyn_bytes) { return dyn_bytes + OBCA_LDS_STATIC_BYTES <= OBCA_LDS_CU_BYTES; }
constexpr Caps caps(int N, int nO, int M) {
    const ObcaShapeSizes z = obca_shape_sizes(N, nO, M);
    const GmSizes gm = gm_sizes(N, nO, M);
    const long long wave = 8 * z.lds_doubles, mw = wave + 8 * (OBCA_ZK_DOUBLES(N) + OBCA_HYB_DOUBLES(z.R_max));
    const bool wave_ok = fits_cu(wave) && wave_row_slots(z.R_max) != 0, mw_ok = fits_cu(mw) && mw_row_slots(z.R_max) != 0;
    const int soc_lds = wave_ok ? obca_soc_lds_wave(N, nO, M) : 0, soc_lds_mw = mw_ok ? obca_soc_lds_mw(N, nO, M) : 0;
    const long long lds_gm = 8 * (gm.lds_doubles + OBCA_ZK_DOUBLES(N));
    return Caps{N, nO, z.n_max, z.R_max, z.inst_off, gm.inst_off, soc_lds, soc_lds_mw,
                wave + (soc_lds ? 8 * obca_soc_doubles(N, nO, M) : 0), mw + (soc_lds_mw ? 8 * obca_soc_doubles(N, nO, M) : 0),
                lds_gm, gm.ws_doubles, wave_ok, mw_ok, fits_cu(lds_gm)};
}

/* The handle's knobs (obca_set_mode, obca_set_shape_specialisation, obca_set_two_sided_sweep, OBCA_LDS_PAD), whether the library
   holds an instantiation for exactly this shape, and whether the HBM workspace could not be allocated once */
struct Knobs {
    int mode;                 /* 0 auto, 1 one wavefront (LDS), 2 lane, 3 four wavefronts (LDS), 4 four wavefronts (HBM workspace), 5 one wavefront (HBM workspace) */
    bool specialise, has_wave_shape, has_mw_shape;
    int two_sided;            /* -1: where the one-wavefront LDS kernels cannot run the shape, 0: never, 1: always */
    long long lds_pad;
    bool gm_ws_failed;
};
/* Kernels whose LDS request the runtime refused (hipFuncSetAttribute at obca_create): a refused family is not offered */
enum Refused : unsigned { REFUSED_WAVE = 1, REFUSED_MW = 2, REFUSED_MW_SHAPE = 4, REFUSED_GM = 8 };
constexpr unsigned refusal_of(Kernel k) {
    return k <= K_WAVE_SHAPE ? REFUSED_WAVE : k <= K_MW_R5 ? REFUSED_MW : k == K_MW_SHAPE ? REFUSED_MW_SHAPE : k <= K_GM1 ? REFUSED_GM : 0u;
}
/* dynamic LDS kernel k asks for with this shape (knobs aside); 0: the shape is never planned onto it */
constexpr long long kernel_lds(const Caps& c, Kernel k) {
    return k == K_WAVE_SHAPE || (k <= K_WAVE_R6 && k == wave_kernel(c.R_max)) ? (c.wave_ok ? c.lds_bytes : 0)
         : k == K_MW_SHAPE || ((k == K_MW_R3 || k == K_MW_R5) && k == mw_kernel(c.R_max)) ? (c.mw_ok ? c.lds_bytes_mw : 0)
         : k == K_GM || k == K_GM1 ? (c.gm_ok ? c.lds_bytes_gm : 0) : 0;
}

constexpr bool wave_offered(const Caps& c, unsigned refused) { return c.wave_ok && !(refused & REFUSED_WAVE); }
constexpr bool mw_offered(const Caps& c, unsigned refused) { return c.mw_ok && !(refused & REFUSED_MW); }
constexpr bool gm_offered(const Caps& c, unsigned refused) { return c.gm_ok && !(refused & REFUSED_GM); }

/* obca_set_mode / OBCA_MODE: mode m (0 .. 5) can run this shape */
constexpr bool mode_available(const Caps& c, unsigned refused, int m) {
    return m == 0 || m == 2 || (m == 1 && wave_offered(c, refused)) || (m == 3 && mw_offered(c, refused)) ||
           ((m == 4 || m == 5) && gm_offered(c, refused));
}

/* ObcaLaunch.two_sided of the LDS-resident and the four-wavefront kernels (obca_set_two_sided_sweep) */
constexpr int sweep_word(const Caps& c, const Knobs& k, unsigned refused) { return k.two_sided < 0 ? (wave_offered(c, refused) ? 0 : 1) : k.two_sided; }

/* Auto mode, shapes beyond the one-wavefront LDS kernel (> 384 rows): ONE wavefront per instance with the row state in the HBM
   workspace (gm1) where an instance has at most three obstacles, the four-wavefront LDS kernel otherwise.  Measured (round 5,
   tools/gpu_gm1_shapes.py, 8192 instances of the C3 generator): three obstacles / 6 rows per stage N = 12 / 16 / 20 / 26:
   114.6 / 151.6 / 178.7 / 255.5 ms against 152.9 / 182.8 / 194.0 / 270.7 ms on four wavefronts (with few rows per stage the
   stage-serial sweep dominates, and four times as many instances in flight hide its latency); five obstacles / 14 rows per stage
   N = 8 ... 14: 187 ... 276 ms against 131 ... 214 ms (the local blocks of five obstacles keep four wavefronts busy); four
   obstacles / 10 rows per stage, obca_mpc6 / 8, N = 10 ... 20: 140 ... 302 ms against 107 ... 179 ms; three obstacles with the
   fixed-time variants gain like the free-time one (tools/gpu_gm1_four.py).  Same words as the four-wavefront kernels with the
   one-sided sweep.  Only the MEASURED region (round 6, advisor): horizons up to N = 26 that the four-wavefront LDS kernel could
   run as well.  Longer horizons and shapes beyond the LDS keep the kernels they had before gm1 existed (four wavefronts: LDS
   resident where it fits, HBM workspace otherwise) until someone measures them. */
#define OBCA_GM1_MAX_N 26

/* The launch: rc = OBCA_OK or OBCA_E_LDS (the mode's kernel cannot hold the shape); inst_off / soc_lds / two_sided: what the
   descriptor must carry for this kernel; lds: dynamic LDS bytes; needs_ws: the handle's HBM workspace must exist. */
struct Plan { int rc; Kernel kernel; int threads; long long lds; int inst_off, soc_lds, two_sided; bool needs_ws, specialised; };

/* A function of the shape, the mode and the knobs -- never of the batch size: the answer to an instance must not depend on how
   many neighbours it was submitted with -- and, once the workspace could not be allocated (gm_ws_failed, sticky), of that fact:
   auto mode then stops choosing gm1 where an LDS-resident kernel, which needs no workspace, holds the shape.
   (Measured: four wavefronts per instance would shorten launches of B <= 256 by 10-12 %, with OBCA_MODE=3 at batch sizes
   <= 256 -- callers that want that latency ask for it, as the obca() class does.) */
constexpr Plan plan(const Caps& c, const Knobs& k, unsigned refused) {
    const bool wave = wave_offered(c, refused), mw = mw_offered(c, refused), gm = gm_offered(c, refused);
    const bool beyond_wave = k.mode == 0 && !wave;
    // the lane kernel (working set in an HBM workspace of its own, one instance per lane) serves every shape: measured on MI355X
    // it is latency bound (every access is an L2/HBM round trip at one wave per SIMD) and 4-10x slower where both run
    Plan p{OBCA_OK, K_LANE, 64, 0, c.inst_off, c.soc_lds, sweep_word(c, k, refused), false, false};
    if (!mode_available(c, refused, k.mode)) { p.rc = OBCA_E_LDS; return p; }
    const bool gm1 = k.mode == 5 || (beyond_wave && mw && gm && c.n_obs <= 3 && c.N <= OBCA_GM1_MAX_N && !k.gm_ws_failed);
    if (gm1 || k.mode == 4 || (beyond_wave && !mw && gm)) {           // rows and O(rows) arrays in the handle's HBM workspace
        p.kernel = gm1 ? K_GM1 : K_GM; p.threads = gm1 ? 64 : 256; p.lds = c.lds_bytes_gm;
        p.inst_off = c.inst_off_gm; p.soc_lds = 0; p.needs_ws = true;
        if (gm1) p.two_sided = 0;
    } else if (k.mode == 3 || (beyond_wave && mw)) {                  // four wavefronts (one CU) per instance, LDS resident
        p.specialised = k.specialise && k.has_mw_shape && !(refused & REFUSED_MW_SHAPE);
        p.kernel = p.specialised ? K_MW_SHAPE : mw_kernel(c.R_max); p.threads = 256; p.lds = c.lds_bytes_mw;
        p.soc_lds = c.soc_lds_mw;
    } else if (k.mode != 2 && wave) {                                 // one wavefront per instance, rows in its registers
        p.specialised = k.specialise && k.has_wave_shape;
        p.kernel = p.specialised ? K_WAVE_SHAPE : wave_kernel(c.R_max); p.lds = c.lds_bytes + k.lds_pad;
    }
    return p;
}

}  // namespace obca_select

#endif
