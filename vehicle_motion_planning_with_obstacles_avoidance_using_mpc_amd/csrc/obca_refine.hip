// obca_refine.hip -- obca_plan_refine of include/obca_mpc.h: the step between the two stages of the open-loop planner, on the
// device.  Stage 1's plans go in (obca_solve_batch's xopt, ts_opt, status), stage 2's reference, step and variant mask come
// out; the arithmetic is csrc/obca_refine_core.h.
//
// Layout: lane gl < B (N2 + 1), N2 = ratio N, computes output point gl % (N2 + 1) of instance gl / (N2 + 1) with the core
// function, its successor point included (for the yaw), so that no lane waits for another: no shuffle, no LDS, no stack
// frame.  The output is [B,3,N2+1]: a wavefront's three stores run along the last axis, 8 contiguous bytes per lane.  Every
// lane decides for itself whether its instance is refined (a scan of the instance's 3 (N + 1) <= 384 knots, the same
// addresses in all lanes of the instance: cache hits after the first).  The lane of point 0 writes ts_out and variant_out.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_refine_core.h"

namespace {

constexpr int BLOCK = 256;

struct RefineArgs {
    int64_t lanes;
    int32_t N, ratio, variant_ok;
    const double *x, *ts;
    const int32_t* status;
    double *xref, *ts_out;
    int32_t* variant_out;
};

__global__ void __launch_bounds__(BLOCK) refine_kernel(RefineArgs P) {
    const int64_t gl = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (gl >= P.lanes) return;
    const int N1 = P.N + 1, P2 = P.ratio * P.N + 1;
    const int64_t inst = gl / P2;
    const int j = (int)(gl - inst * P2);
    const double* x = P.x + inst * 3 * N1;
    const double ts = P.ts[inst];
    const bool ok = refine::usable(x, P.N, ts, P.status ? P.status[inst] : 0);
    double o[3];
    refine::point(x, P.N, P.ratio, j, ok, o);
    double* xr = P.xref + inst * 3 * P2 + j;
    xr[0] = o[0]; xr[P2] = o[1]; xr[2 * (int64_t)P2] = o[2];
    if (j == 0) {
        P.ts_out[inst] = refine::step_out(P.N, P.ratio, ts, ok);
        if (P.variant_out) P.variant_out[inst] = ok ? P.variant_ok : 0;
    }
}

}  // namespace

extern "C" int obca_plan_refine(int32_t B, int32_t N, int32_t ratio, const double* x, const double* ts, const int32_t* status,
                                int32_t variant_ok, double* xref_out, double* ts_out, int32_t* variant_out, int32_t device,
                                void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (refine::args_check(B, N, ratio, x, ts, variant_ok, xref_out, ts_out) != 0 || device < 0) return OBCA_E_INVAL;
    RefineArgs P;
    P.lanes = (int64_t)B * (ratio * N + 1);
    P.N = N; P.ratio = ratio; P.variant_ok = variant_ok;
    P.x = x; P.ts = ts; P.status = status; P.xref = xref_out; P.ts_out = ts_out; P.variant_out = variant_out;
    const int64_t blocks = (P.lanes + BLOCK - 1) / BLOCK;
    if (blocks > 0x7fffffff) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(refine_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, P);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
