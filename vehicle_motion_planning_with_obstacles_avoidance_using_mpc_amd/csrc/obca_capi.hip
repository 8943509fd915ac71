// obca_capi.hip -- host side of libobca_mpc.so: the C ABI declared in include/obca_mpc.h.
// Plain pointers and sizes only; every failure is a return code (no exception leaves this file).

#include <hip/hip_runtime.h>
#include <new>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include "obca_device.h"
#include "obca_lpi_core.h"
#include "obca_select.h"

extern "C" __global__ void obca_ipm_kernel_r4(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);
extern "C" __global__ void obca_ipm_kernel_r5(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);
extern "C" __global__ void obca_ipm_kernel_r6(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);
extern "C" __global__ void obca_ipm_kernel_mw_r3(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);          // four wavefronts per instance (obca_kernel_mw.hip)
extern "C" __global__ void obca_ipm_kernel_mw_r5(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);
extern "C" __global__ void obca_ipm_kernel_gm(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);             // four wavefronts, rows in an HBM workspace
extern "C" __global__ void obca_ipm_kernel_gm1(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);            // one wavefront, rows in an HBM workspace
// compile-time-shape instantiations of the one-wavefront kernel (csrc/obca_kernel_s*.hip; list: csrc/obca_device.h OBCA_SHAPES)
#define OBCA_DECLARE_SHAPE_KERNEL(N_, O_, M_) extern "C" __global__ void obca_ipm_kernel_s##N_##_##O_##_##M_(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);
OBCA_SHAPES(OBCA_DECLARE_SHAPE_KERNEL)
#define OBCA_DECLARE_MW_SHAPE_KERNEL(N_, O_, M_) extern "C" __global__ void obca_ipm_kernel_mw_s##N_##_##O_##_##M_(ObcaLaunch A, ObcaLaunch A2, ObcaLaunch A3);
OBCA_MW_SHAPES(OBCA_DECLARE_MW_SHAPE_KERNEL)
typedef void (*obca_wave_kernel_t)(ObcaLaunch, ObcaLaunch, ObcaLaunch);
extern "C" __global__ void obca_lpi_kernel(ObcaLaunch A, double* ws, unsigned long long stride, const int* offm, int ipw);

namespace sel = obca_select;

struct obca_handle {
    obca_dims dims;
    int32_t M;
    int32_t offm[OBCA_MAX_OBST + 1];
    sel::Caps cap;            /* what the shape alone decides: sizes, LDS requests, which kernel families hold it */
    sel::Knobs knobs;         /* mode, specialise, two_sided, lds_pad (dev knob OBCA_LDS_PAD: occupancy experiments), gm_ws_failed */
    unsigned refused;         /* sel::Refused: families whose LDS request the runtime refused */
    obca_wave_kernel_t kernel[sel::K_COUNT];   /* id -> function; K_WAVE_SHAPE / K_MW_SHAPE: the instantiation for exactly this shape, or nullptr */
    double* gm_ws;            /* HBM workspace of the gm kernels, allocated on first use: max_batch slices of cap.gm_doubles */
    double* prof;
    double* warm_z;           /* obca_set_warm_start */
    const int32_t* warm_use;
    double warm_mu;
    double *cert_z, *cert_y;  /* obca_set_certificate_buffers */
    double* soc_ws;           /* scratch of the second-order correction (wave kernels), max_batch x soc_stride doubles */
    double* ws;               /* lane kernel workspace, allocated on first use */
    size_t ws_stride;
    int* d_offm;
    int64_t ws_doubles;
};

namespace {

bool dims_ok(const obca_dims* d) {
    if (!d) return false;
    if (d->N < 1 || d->N > 127) return false;     // the wave kernel only ever sees N < 64 (rows / LDS), the lane kernel any
    if (d->n_obs < 1 || d->n_obs > OBCA_MAX_OBST) return false;
    for (int i = 0; i < d->n_obs; ++i)
        if (d->m[i] < 1 || d->m[i] > OBCA_MAX_EDGES) return false;
    return true;
}

int rows_per_stage(const obca_dims* d) {          // M: half-space rows of all obstacles
    int M = 0;
    for (int i = 0; i < d->n_obs; ++i) M += d->m[i];
    return M;
}

}  // namespace

extern "C" int64_t obca_lds_bytes(const obca_dims* d) {
    if (!dims_ok(d)) return -1;
    return 8 * obca_shape_sizes(d->N, d->n_obs, rows_per_stage(d)).lds_doubles;
}

extern "C" int obca_create(const obca_dims* d, obca_handle** out) {
    if (!out) return OBCA_E_INVAL;
    *out = nullptr;
    if (!dims_ok(d) || d->max_batch < 1) return OBCA_E_INVAL;
    obca_handle* h = new (std::nothrow) obca_handle;
    if (!h) return OBCA_E_NOMEM;
    h->dims = *d;
    h->M = rows_per_stage(d);
    h->offm[0] = 0;
    for (int i = 0; i < OBCA_MAX_OBST; ++i) h->offm[i + 1] = h->offm[i] + (i < d->n_obs ? d->m[i] : 0);
    h->cap = sel::caps(d->N, d->n_obs, h->M);
    h->gm_ws = nullptr;
    ObcaDeviceGuard guard(d->device);
    if (!guard.ok) { delete h; return OBCA_E_HIP; }
    for (int k = 0; k < sel::K_COUNT; ++k) h->kernel[k] = nullptr;          // (K_LANE stays empty: other arguments, its own launch)
    h->kernel[sel::K_WAVE_R4] = obca_ipm_kernel_r4; h->kernel[sel::K_WAVE_R5] = obca_ipm_kernel_r5; h->kernel[sel::K_WAVE_R6] = obca_ipm_kernel_r6;
    h->kernel[sel::K_MW_R3] = obca_ipm_kernel_mw_r3; h->kernel[sel::K_MW_R5] = obca_ipm_kernel_mw_r5;
    h->kernel[sel::K_GM] = obca_ipm_kernel_gm; h->kernel[sel::K_GM1] = obca_ipm_kernel_gm1;
#define OBCA_MATCH_MW_SHAPE_KERNEL(N_, O_, M_) if (d->N == N_ && d->n_obs == O_ && h->M == M_) h->kernel[sel::K_MW_SHAPE] = obca_ipm_kernel_mw_s##N_##_##O_##_##M_;
    OBCA_MW_SHAPES(OBCA_MATCH_MW_SHAPE_KERNEL)
#define OBCA_MATCH_SHAPE_KERNEL(N_, O_, M_) if (d->N == N_ && d->n_obs == O_ && h->M == M_) h->kernel[sel::K_WAVE_SHAPE] = obca_ipm_kernel_s##N_##_##O_##_##M_;
    OBCA_SHAPES(OBCA_MATCH_SHAPE_KERNEL)
    // every kernel this shape can be planned onto may ask for its LDS; one whose request the runtime refuses is simply not
    // offered (the lane kernel serves every shape) -- of the four-wavefront family, a refused instantiation alone is dropped.
    // (The one-wavefront instantiations are in the loop on purpose: every listed one stays below 64 KiB today, so none asks; one
    // that did and was refused would take the family with it, as the generic kernel of the same LDS request would.)
    h->refused = 0;
    for (int k = 0; k < sel::K_COUNT; ++k) {
        const int64_t lds = sel::kernel_lds(h->cap, (sel::Kernel)k);
        const unsigned family = sel::refusal_of((sel::Kernel)k);
        if (!h->kernel[k] || lds <= 64 * 1024 || (h->refused & (family | (k == sel::K_MW_SHAPE ? sel::REFUSED_MW : 0u)))) continue;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(h->kernel[k]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            h->refused |= family;
        }
    }
    sel::Knobs& kn = h->knobs;
    kn.mode = 0;
    kn.has_wave_shape = h->kernel[sel::K_WAVE_SHAPE] != nullptr;
    kn.has_mw_shape = h->kernel[sel::K_MW_SHAPE] != nullptr;
    kn.gm_ws_failed = false;
    kn.specialise = true;
    if (const char* e = getenv("OBCA_SPECIALISE")) kn.specialise = atoi(e) != 0;
    kn.lds_pad = 0;
    if (const char* e = getenv("OBCA_LDS_PAD")) { const long v = atol(e); if (v > 0 && h->cap.lds_bytes + v <= 64 * 1024) kn.lds_pad = v; }
    kn.two_sided = -1;
    if (const char* e = getenv("OBCA_TWO_SIDED")) { const int v = atoi(e); if (v >= -1 && v <= 1) kn.two_sided = v; }
    if (const char* e = getenv("OBCA_MODE")) {
        const int m = atoi(e);                                     // out of range or not available for this shape: auto
        if (sel::mode_available(h->cap, h->refused, m)) kn.mode = m;
    }
    h->ws = nullptr; h->d_offm = nullptr;
    h->ws_stride = ((size_t)d->max_batch + 63) / 64 * 64;
    h->ws_doubles = lpi::carve(d->N, d->n_obs, h->M, h->cap.n_max, h->cap.R_max).total;
    h->prof = nullptr;
    h->warm_z = nullptr; h->warm_use = nullptr; h->warm_mu = 0.0;
    h->cert_z = nullptr; h->cert_y = nullptr;
    h->soc_ws = nullptr;
    if (sel::wave_offered(h->cap, h->refused) || sel::mw_offered(h->cap, h->refused) || sel::gm_offered(h->cap, h->refused)) {
        const size_t stride = (size_t)h->cap.n_max + 2 * (size_t)h->cap.R_max + 2 * (size_t)(d->N + 1) * d->n_obs;
        if (hipMalloc(&h->soc_ws, sizeof(double) * stride * (size_t)d->max_batch) != hipSuccess) { h->soc_ws = nullptr; delete h; return OBCA_E_NOMEM; }
    }
    *out = h;
    return OBCA_OK;
}

extern "C" void obca_destroy(obca_handle* h) {
    if (!h) return;
    ObcaDeviceGuard guard(h->dims.device);
    if (h->ws) (void)hipFree(h->ws);
    if (h->gm_ws) (void)hipFree(h->gm_ws);
    if (h->soc_ws) (void)hipFree(h->soc_ws);
    if (h->d_offm) (void)hipFree(h->d_offm);
    delete h;
}

extern "C" int obca_set_mode(obca_handle* h, int mode) {
    if (!h || mode < 0 || mode > 5) return OBCA_E_INVAL;
    if (!sel::mode_available(h->cap, h->refused, mode)) return OBCA_E_LDS;
    h->knobs.mode = mode;
    return OBCA_OK;
}

extern "C" int64_t obca_primal_size(const obca_dims* d) {
    if (!dims_ok(d)) return -1;
    return (int64_t)(d->N + 1) * (3 + rows_per_stage(d) + 4 * d->n_obs) + 2 * d->N + 1;
}

extern "C" int obca_set_warm_start(obca_handle* h, double* z, const int32_t* use, double mu_init) {
    if (!h || (z && !(mu_init > 0.0))) return OBCA_E_INVAL;
    h->warm_z = z; h->warm_use = z ? use : nullptr; h->warm_mu = mu_init;
    return OBCA_OK;
}

extern "C" int64_t obca_dual_size(const obca_dims* d) {
    if (!dims_ok(d)) return -1;
    return (int64_t)obca_shape_sizes(d->N, d->n_obs, rows_per_stage(d)).R_max + 2 * (int64_t)(d->N + 1) * d->n_obs;
}

extern "C" int obca_set_certificate_buffers(obca_handle* h, double* z, double* y) {
    if (!h) return OBCA_E_INVAL;
    h->cert_z = z; h->cert_y = y;
    return OBCA_OK;
}

extern "C" int obca_set_shape_specialisation(obca_handle* h, int on) {
    if (!h || on < 0 || on > 1) return OBCA_E_INVAL;
    h->knobs.specialise = on != 0;
    return OBCA_OK;
}

extern "C" int obca_shape_is_specialised(const obca_handle* h) {
    if (!h) return OBCA_E_INVAL;
    return sel::plan(h->cap, h->knobs, h->refused).specialised ? 1 : 0;
}

extern "C" int obca_set_two_sided_sweep(obca_handle* h, int on) {
    if (!h || on < -1 || on > 1) return OBCA_E_INVAL;
    h->knobs.two_sided = on;
    return OBCA_OK;
}

extern "C" void obca_set_profile_buffer(obca_handle* h, double* prof) { if (h) h->prof = prof; }

int obca_internal_fill_launch(obca_handle* h, const int32_t* variant, int32_t B,
                              const double* x0, const double* u0, const double* xref,
                              const double* A, const double* b, const double* Ts, const double* term,
                              const obca_params* p,
                              double* xopt, double* uopt, double* ts_opt, int32_t* status, int32_t* iters,
                              double* info, ObcaLaunch* out, int64_t* lds_bytes, int* wave_ok) {
    if (!h || !variant || !x0 || !u0 || !xref || !A || !b || !Ts || !p || !xopt || !uopt || !ts_opt || !status ||
        !iters || !out)
        return OBCA_E_INVAL;
    if (B < 0 || B > h->dims.max_batch) return OBCA_E_INVAL;
    if (p->struct_size != (uint32_t)sizeof(obca_params)) return OBCA_E_INVAL;      // another layout, or never initialised (obca_params_init)
    ObcaLaunch& L = *out;
    memset(&L, 0, sizeof(L));
    L.B = B; L.N = h->dims.N; L.nO = h->dims.n_obs; L.M = h->M; L.n_max = h->cap.n_max; L.R_max = h->cap.R_max; L.inst_off = h->cap.inst_off;
    L.two_sided = sel::sweep_word(h->cap, h->knobs, h->refused);
    for (int i = 0; i <= OBCA_MAX_OBST; ++i) L.offm[i] = h->offm[i];
    L.variant = variant; L.x0 = x0; L.u0 = u0; L.xref = xref; L.A = A; L.b = b; L.Ts = Ts; L.term = term;
    L.xopt = xopt; L.uopt = uopt; L.ts_opt = ts_opt; L.status = status; L.iters = iters; L.info = info; L.prof = h->prof;
    L.warm_z = h->warm_z; L.warm_use = h->warm_use; L.warm_mu = h->warm_mu;
    L.cert_z = h->cert_z; L.cert_y = h->cert_y;
    L.soc_ws = h->soc_ws; L.soc_lds = h->cap.soc_lds;
    auto cpw = [](ObcaWeightsDev& d, const obca_weights& s) {
        // the reference's double loops use Q[i,j] for every (i,j): only the symmetric part matters
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) {
                d.Q[3 * a + c] = 0.5 * (s.Q[3 * a + c] + s.Q[3 * c + a]);
                d.P[3 * a + c] = 0.5 * (s.P[3 * a + c] + s.P[3 * c + a]);
            }
        for (int a = 0; a < 2; ++a)
            for (int c = 0; c < 2; ++c) {
                d.R1[2 * a + c] = 0.5 * (s.R1[2 * a + c] + s.R1[2 * c + a]);
                d.R2[2 * a + c] = 0.5 * (s.R2[2 * a + c] + s.R2[2 * c + a]);
            }
    };
    cpw(L.prm.free_time, p->free_time);
    cpw(L.prm.fixed_time, p->fixed_time);
    for (int j = 0; j < 2; ++j) { L.prm.xL[j] = p->xL[j]; L.prm.xU[j] = p->xU[j]; L.prm.uL[j] = p->uL[j]; L.prm.uU[j] = p->uU[j]; }
    const double Lc = p->ego[0] + p->ego[2], Wc = p->ego[1] + p->ego[3];       // src/obca.py:1019-1026
    L.prm.gego[0] = Lc / 2; L.prm.gego[1] = Wc / 2; L.prm.gego[2] = Lc / 2; L.prm.gego[3] = Wc / 2;
    L.prm.off = Lc / 2 - p->ego[2];
    L.prm.dmin = p->dmin;
    L.prm.opt.tol = p->tol > 0 ? p->tol : 1e-8;
    L.prm.opt.rho = p->rho > 0 ? p->rho : 1e4;
    L.prm.opt.feas_tol = p->feas_tol > 0 ? p->feas_tol : 1e-6;
    L.prm.opt.max_iter_free = p->max_iter_free > 0 ? p->max_iter_free : 3000;
    L.prm.opt.max_iter_fixed = p->max_iter_fixed > 0 ? p->max_iter_fixed : 1000;
    L.prm.opt.max_soc = p->max_soc == 0 ? OBCA_MAX_SOC : (p->max_soc < 0 ? 0 : p->max_soc);
    if (!obca_resolve_starts(&L.prm.opt, p->start_order, p->single_start, p->patience, p->retry_iter, h->dims.N, p->dodge, p->terminal_screen)) return OBCA_E_INVAL;
    if (!obca_resolve_time_bound(&L.prm.opt, p->time_bound)) return OBCA_E_INVAL;
    if (lds_bytes) *lds_bytes = h->cap.lds_bytes;
    if (wave_ok) *wave_ok = sel::wave_offered(h->cap, h->refused) ? 1 : 0;
    return OBCA_OK;
}

extern "C" int obca_solve_batch(obca_handle* h, const int32_t* variant, int32_t B,
                                const double* x0, const double* u0, const double* xref,
                                const double* A, const double* b, const double* Ts, const double* term,
                                const obca_params* p,
                                double* xopt, double* uopt, double* ts_opt, int32_t* status, int32_t* iters,
                                double* info, void* hip_stream) {
    ObcaLaunch L;
    const int rc = obca_internal_fill_launch(h, variant, B, x0, u0, xref, A, b, Ts, term, p, xopt, uopt, ts_opt, status,
                                             iters, info, &L, nullptr, nullptr);
    if (rc != OBCA_OK) return rc;
    if (B == 0) return OBCA_OK;
    ObcaDeviceGuard guard(h->dims.device);
    if (!guard.ok) return OBCA_E_HIP;
    // which kernel, with what: a function of the shape, the mode and the knobs -- never of the batch size -- and, after a failed
    // workspace allocation, of that fact (csrc/obca_select.h: plan)
    sel::Plan plan = sel::plan(h->cap, h->knobs, h->refused);
    if (plan.rc != OBCA_OK) return plan.rc;
    // (OBCA_FAIL_WORKSPACE_ALLOC in the environment: the allocation is treated as failed -- the only way to exercise the branch below
    // on a 288 GB device; tests/test_gpu_edge_cases.py)
    if (plan.needs_ws && !h->gm_ws &&
        (getenv("OBCA_FAIL_WORKSPACE_ALLOC") != nullptr ||
         hipMalloc(&h->gm_ws, sizeof(double) * (size_t)h->cap.gm_doubles * (size_t)h->dims.max_batch) != hipSuccess)) {
        (void)hipGetLastError();
        h->gm_ws = nullptr;
        // auto mode with an LDS-resident alternative: run that instead of failing the call (it needs no workspace); an explicit
        // mode 4 / 5 and shapes only the workspace kernels hold report the failure
        if (!(h->knobs.mode == 0 && sel::mw_offered(h->cap, h->refused))) return OBCA_E_NOMEM;
        h->knobs.gm_ws_failed = true;
        plan = sel::plan(h->cap, h->knobs, h->refused);       // (mode 0 is always available: the second plan cannot fail)
    }
    L.inst_off = plan.inst_off; L.soc_lds = plan.soc_lds; L.two_sided = plan.two_sided;
    if (plan.kernel != sel::K_LANE) {
        if (plan.needs_ws) { L.gm_ws = h->gm_ws; L.gm_stride = h->cap.gm_doubles; }
        // the kernels run the further passes of the start ladder (penalty escalation, next starts) themselves, from their own copy of the descriptor
        ObcaLaunch L2 = L;
        hipLaunchKernelGGL(h->kernel[plan.kernel], dim3(B), dim3(plan.threads), (size_t)plan.lds, (hipStream_t)hip_stream, L, L2, L2);
    } else {
        if (!h->ws || !h->d_offm) {
            if (!h->ws && hipMalloc(&h->ws, sizeof(double) * (size_t)h->ws_doubles * h->ws_stride) != hipSuccess) { h->ws = nullptr; return OBCA_E_NOMEM; }
            if (!h->d_offm && hipMalloc(&h->d_offm, sizeof(int) * (OBCA_MAX_OBST + 1)) != hipSuccess) { h->d_offm = nullptr; return OBCA_E_NOMEM; }
            if (hipMemcpy(h->d_offm, h->offm, sizeof(int) * (OBCA_MAX_OBST + 1), hipMemcpyHostToDevice) != hipSuccess) return OBCA_E_HIP;
        }
        int ipw = 64;                               // one wave per SIMD (256 CUs x 4) before the waves get fatter
        while (ipw > 1 && (B + ipw - 1) / ipw < 1024) ipw >>= 1;
        hipLaunchKernelGGL(obca_lpi_kernel, dim3((B + ipw - 1) / ipw), dim3(64), 0, (hipStream_t)hip_stream, L, h->ws,
                           (unsigned long long)h->ws_stride, h->d_offm, ipw);
    }
    if (hipGetLastError() != hipSuccess) return OBCA_E_HIP;
    return OBCA_OK;
}

extern "C" const char* obca_strerror(int code) {
    switch (code) {
        case OBCA_OK: return "ok";
        case OBCA_E_INVAL: return "invalid argument or shape beyond compiled limits";
        case OBCA_E_NOMEM: return "out of host memory";
        case OBCA_E_HIP: return "HIP runtime call failed";
        case OBCA_E_LDS: return "instance does not fit in 160 KiB of LDS";
        default: return "unknown error";
    }
}

extern "C" const char* obca_version(void) { return "obca_mpc 0.18 (gfx950)"; }
extern "C" void obca_params_init(obca_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
}
