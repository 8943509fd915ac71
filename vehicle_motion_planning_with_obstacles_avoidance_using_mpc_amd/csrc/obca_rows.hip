// obca_rows.hip -- obstacle rows of moving rectangles for batch callers (obca_moving_rows_batch of include/obca_mpc.h):
// the rows the closed loop's harness builds for its sensed boxes (rollout::moving_box_rows in csrc/obca_rollout_core.h),
// for B instances x N + 1 stages x n_box boxes at once, plus the static rows copied into every stage.
//
// Layout: lane gl < B (N+1) n_box builds the four rows of box gl % n_box at (instance, stage) gl / n_box with the core
// function (one lane per (instance, stage, box), so that builder and harness share that function): the lane writes its own 64 bytes of A as four
// 16-byte vector stores (every row starts at an even number of doubles) and its 32 bytes of b as four 8-byte ones.
// Neighbouring lanes write neighbouring pieces, so a wavefront's stores of one (instance, stage) cover one contiguous
// range and every cache line is written whole -- but one store instruction strides 64 B from lane to lane, it is not the
// lane-contiguous pattern of a transposed layout (one row per lane), which would have four lanes repeat the vertices.
// Lane gl < B (N+1) Ms copies static row gl % Ms of (instance, stage) gl / Ms: here one instruction's lanes are
// contiguous (16 B of A, 8 B of b each).  No LDS, no stack frame: the core keeps the vertices in registers.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_rollout_core.h"

namespace {

constexpr int BLOCK = 256;

struct RowsArgs {
    int64_t n_moving, n_static;        // lanes with a box / with a static row
    int32_t N1, Ms, n_box, M;
    double h, r;
    const double *As, *bs, *boxes, *Ts;
    double *A, *b;
};

__global__ void __launch_bounds__(BLOCK) moving_rows_kernel(RowsArgs P) {
    const int64_t gl = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (gl < P.n_moving) {
        const int64_t bk = gl / P.n_box;                                 // (instance, stage)
        const int j = (int)(gl - bk * P.n_box);
        const int64_t inst = bk / P.N1;
        const int kk = (int)(bk - inst * P.N1);
        double Ar[8], br[4];
        rollout::moving_box_rows(P.boxes + (inst * P.n_box + j) * rollout::DYN_W, P.Ts[inst], kk, P.h, P.r, Ar, br);
        double2* Ao = reinterpret_cast<double2*>(P.A + (bk * P.M + P.Ms + 4 * j) * 2);
        double* bo = P.b + bk * P.M + P.Ms + 4 * j;
        Ao[0] = make_double2(Ar[0], Ar[1]); Ao[1] = make_double2(Ar[2], Ar[3]);
        Ao[2] = make_double2(Ar[4], Ar[5]); Ao[3] = make_double2(Ar[6], Ar[7]);
        bo[0] = br[0]; bo[1] = br[1]; bo[2] = br[2]; bo[3] = br[3];
    }
    if (gl < P.n_static) {
        const int64_t bk = gl / P.Ms;
        const int q = (int)(gl - bk * P.Ms);
        const int64_t inst = bk / P.N1;
        reinterpret_cast<double2*>(P.A)[bk * P.M + q] = reinterpret_cast<const double2*>(P.As)[inst * P.Ms + q];
        P.b[bk * P.M + q] = P.bs[inst * P.Ms + q];
    }
}

}  // namespace

extern "C" int obca_moving_rows_batch(int32_t B, int32_t N, int32_t Ms, int32_t n_box, const double* static_A,
                                      const double* static_b, const double* boxes, const double* Ts, double half_window,
                                      double margin, double* A, double* b, int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect (NaN fails the comparisons)
    if (B < 1 || N < 1 || N > (1 << 20) || Ms < 0 || Ms > OBCA_MAX_OBST * OBCA_MAX_EDGES || n_box < 0 || n_box > OBCA_MAX_OBST ||
        Ms + 4 * n_box < 1 || device < 0 || !A || !b || (Ms > 0 && (!static_A || !static_b)) || (n_box > 0 && (!boxes || !Ts)) ||
        !(half_window >= 0.0 && half_window <= 1.0) || !(margin >= 0.0 && margin <= 2.0) ||
        ((uintptr_t)A & 15) != 0 || ((uintptr_t)static_A & 15) != 0)
        return OBCA_E_INVAL;
    RowsArgs P;
    const int64_t stages = (int64_t)B * (N + 1);
    P.n_moving = stages * n_box; P.n_static = stages * Ms;
    P.N1 = N + 1; P.Ms = Ms; P.n_box = n_box; P.M = Ms + 4 * n_box;
    P.h = half_window; P.r = margin;
    P.As = static_A; P.bs = static_b; P.boxes = boxes; P.Ts = Ts; P.A = A; P.b = b;
    const int64_t lanes = P.n_moving > P.n_static ? P.n_moving : P.n_static;
    const int64_t blocks = (lanes + BLOCK - 1) / BLOCK;
    if (blocks > 0x7fffffff) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(moving_rows_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, P);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
