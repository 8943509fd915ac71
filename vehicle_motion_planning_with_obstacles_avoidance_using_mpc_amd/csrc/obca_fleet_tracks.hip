// obca_fleet_tracks.hip -- obca_fleet_tracks of include/obca_mpc.h: the step after obca_fleet_step that turns the plans just
// applied into rows per stage for obca_scene_select_staged.  The arithmetic and the serial definition are
// csrc/obca_fleet_tracks_core.h.
//
// Layout: one workgroup of 256 threads per world.
//   usable    wavefront w takes the cars j = w, w + 4, ...: its lanes stride over the 3 (N + 1) words of the plan, one __all
//             decides, lane 0 puts the word into LDS
//   tracks    behind one __syncthreads() the threads stride over the V (N + 1) (car, stage) pairs: one pose, one
//             fleet::car_rows (or the spare), 8 + 4 words stored by the thread that computed them
//   masks     then over the V V mask words
// Every address is formed from an index below its bound: q < V (N + 1) and q < V V.  No thread reads a word another thread
// of the launch writes, except through the LDS flags behind the barrier.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_fleet_tracks_core.h"

namespace {

constexpr int BLOCK = 256, WAVE = 64, WAVES = BLOCK / WAVE;

__global__ void __launch_bounds__(BLOCK) tracks_kernel(struct obca_fleet_tracks D) {
    __shared__ int s_use[fleet::MAX_V];
    const int w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int V = D.V, N1 = D.N + 1;
    const int64_t g = blockIdx.x;

    for (int j = w; j < V; j += WAVES) {                             // wave-uniform
        const int64_t q = g * V + j;
        const double* xo = D.xopt + q * 3 * N1;
        bool fin = true;
        for (int t = lane; t < 3 * N1; t += WAVE) fin = fin && fleet::finite_(xo[t]);
        const bool ok = __all(fin) && tracks::plan_applied(D, q);
        if (lane == 0) s_use[j] = ok ? 1 : 0;
    }
    __syncthreads();

    for (int p = threadIdx.x; p < V * N1; p += BLOCK) {
        const int j = p / N1, kk = p - j * N1;
        const int64_t q = g * V + j;
        double A[2 * tracks::E], b[tracks::E];
        tracks::track_rows(D, q, s_use[j] != 0, kk, A, b);
        double* oA = D.track_A + (q * N1 + kk) * tracks::E * 2;
        double* ob = D.track_b + (q * N1 + kk) * tracks::E;
#pragma unroll
        for (int r = 0; r < 2 * tracks::E; ++r) oA[r] = A[r];
#pragma unroll
        for (int r = 0; r < tracks::E; ++r) ob[r] = b[r];
    }
    for (int p = threadIdx.x; p < V * V; p += BLOCK) {
        const int a = p / V, j = p - a * V;
        D.track_ok[(g * V + a) * V + j] = tracks::mask_word(D, g, a, j, s_use[j] != 0);
    }
}

}  // namespace

extern "C" void obca_fleet_tracks_init(struct obca_fleet_tracks* d) {
    if (d) tracks::init(d);
}

extern "C" int obca_fleet_tracks(const struct obca_fleet_tracks* d, int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (tracks::args_check(d) != 0 || device < 0) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(tracks_kernel, dim3((unsigned)d->G), dim3(BLOCK), 0, (hipStream_t)hip_stream, *d);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
