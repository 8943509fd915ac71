// obca_route.hip -- obca_grid_dilate_batch and obca_route_resample of include/obca_mpc.h: the two steps between the batched
// planner (csrc/obca_astar.hip) and a fixed-horizon solve.  The grid is dilated by a disk before the search, so that the
// route keeps off corners a car cannot hug; the route of path_len lattice points is resampled to the N + 1 knots a solve
// tracks.  The arithmetic is csrc/obca_route_core.h.
//
// Dilation: lane gl < B rows cols computes one output cell from at most (2 level + 1)^2 input bytes of its own grid (clipped to
// the grid, so no address outside it is formed); neighbouring lanes read neighbouring bytes and store neighbouring bytes.
//
// Resampling: lane gl < B (N + 1) computes knot gl % (N + 1) of instance gl / (N + 1), its successor included (for the yaw),
// so that no lane waits for another: no shuffle, no LDS.  Every lane walks its instance's route with the running sum of the
// core -- the same addresses in all lanes of the instance (cache hits after the first), the sum order of the host build.
// The output is [B,3,N+1]: a wavefront's three stores run along the last axis.  The lane of knot 0 writes ok.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_route_core.h"

namespace {

constexpr int BLOCK = 256;

struct DilateArgs {
    int64_t lanes;
    int32_t rows, cols, level;
    const uint8_t* grid;
    uint8_t* out;
};

__global__ void __launch_bounds__(BLOCK) dilate_kernel(DilateArgs P) {
    const int64_t gl = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (gl >= P.lanes) return;
    const int cells = P.rows * P.cols;
    const int64_t inst = gl / cells;
    const int cell = (int)(gl - inst * cells), r = cell / P.cols, c = cell - r * P.cols;
    P.out[gl] = route::dilate_cell(P.grid + inst * cells, P.rows, P.cols, r, c, P.level);
}

struct ResampleArgs {
    int64_t lanes;
    int32_t path_max, N;
    const double* path;
    const int32_t* path_len;
    const double *start, *goal;
    double* xref;
    int32_t* ok;
};

__global__ void __launch_bounds__(BLOCK) resample_kernel(ResampleArgs P) {
    const int64_t gl = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (gl >= P.lanes) return;
    const int N1 = P.N + 1;
    const int64_t inst = gl / N1;
    const int k = (int)(gl - inst * N1);
    const double* path = P.path + inst * 3 * P.path_max;
    const double* start = P.start ? P.start + inst * 3 : nullptr;
    const double* goal = P.goal ? P.goal + inst * 3 : nullptr;
    const int L = P.path_len[inst];
    double S;
    const bool ok = route::instance_ok(path, P.path_max, L, start, goal, &S);
    double o[3];
    route::knot(path, P.path_max, L, S, P.N, k, start, goal, ok, o);
    double* xr = P.xref + inst * 3 * N1 + k;
    xr[0] = o[0]; xr[N1] = o[1]; xr[2 * (int64_t)N1] = o[2];
    if (k == 0) P.ok[inst] = ok ? 1 : 0;
}

}  // namespace

extern "C" int obca_grid_dilate_batch(const uint8_t* grid, int32_t B, int32_t rows, int32_t cols, int32_t level, uint8_t* out,
                                      int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (route::dilate_args_check(B, rows, cols, level, grid, out) != 0 || device < 0) return OBCA_E_INVAL;
    DilateArgs P;
    P.lanes = (int64_t)B * rows * cols;
    P.rows = rows; P.cols = cols; P.level = level; P.grid = grid; P.out = out;
    const int64_t blocks = (P.lanes + BLOCK - 1) / BLOCK;
    if (blocks > 0x7fffffff) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, P);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}

extern "C" int obca_route_resample(int32_t B, int32_t path_max, int32_t N, const double* path, const int32_t* path_len,
                                   const double* start, const double* goal, double* xref_out, int32_t* ok_out, int32_t device,
                                   void* hip_stream) {
    if (route::args_check(B, path_max, N, path, path_len, xref_out, ok_out) != 0 || device < 0) return OBCA_E_INVAL;
    ResampleArgs P;
    P.lanes = (int64_t)B * (N + 1);
    P.path_max = path_max; P.N = N; P.path = path; P.path_len = path_len; P.start = start; P.goal = goal;
    P.xref = xref_out; P.ok = ok_out;
    const int64_t blocks = (P.lanes + BLOCK - 1) / BLOCK;
    if (blocks > 0x7fffffff) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, P);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
