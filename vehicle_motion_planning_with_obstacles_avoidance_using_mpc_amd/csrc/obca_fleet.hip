// obca_fleet.hip -- obca_fleet_step of include/obca_mpc.h: the step between two solves of the fleet closed loop that turns the
// other cars of a world into pool obstacles of each car and measures what the cars did to each other.  The arithmetic and the
// serial definition are csrc/obca_fleet_core.h.
//
// Layout: one workgroup per world, one wavefront per car (V <= 16, so a block has V * 64 <= 1024 threads and no wavefront beyond
// V exists), lane j = the other car j.
//   measure   lane j < V, j != a of wave a runs fleet::pair_of for the pair (a, j) -- the lower index as the footprint, so the
//             two wavefronts of a pair compute one word; the V values go through LDS and every lane folds them in index order
//             with audit::min_nan (broadcast reads, no atomics): the serial loop's word, the same in every lane, so the flag
//             decision is wave-uniform.  The slot of the car itself holds +inf, which min_nan passes over.
//   flags     lane 0 of wave a writes the car's history word and flag, the wavefront strides over the masked window; the flag
//             as it is after the measurement goes to LDS, and behind one __syncthreads() every wavefront reads the flags of
//             its whole world: the agent slots written in this launch see this launch's flags
//   agents    lane j < V of wave a writes slot Ks + j of rollout (g, a): 8 + 4 + 2 words
// Lanes beyond V form no address.  Every value a lane stores is picked with selects or computed by the lane: no local array
// is indexed with a lane number (that is a stack frame).  The flag a wavefront reads from memory is its own car's alone, and
// only its lane 0 writes it, after the read: no word is read by one wavefront and written by another.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_fleet_core.h"

namespace {

constexpr int WAVE = 64, MAX_BLOCK = fleet::MAX_V * WAVE;

__global__ void __launch_bounds__(MAX_BLOCK) fleet_kernel(obca_fleet D, int32_t measure) {
    __shared__ double s_pair[fleet::MAX_V][fleet::MAX_V];
    __shared__ int s_flag[fleet::MAX_V];
    const int a = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;     // a < V: the block has V wavefronts
    const int V = D.V, K = D.Ks + D.V, S = D.max_steps, N1 = D.N + 1;
    const int64_t g = blockIdx.x, b = g * V + a;
    const bool other = lane < V;

    int flag = D.flags[b];
    const bool moved = measure && D.n_sub > 0 && fleet::stepped(D, b);               // wave-uniform
    double cur = INFINITY;
    if (moved && other && lane != a) cur = fleet::pair_of(D, g, a, lane);
    if (other) s_pair[a][lane] = cur;
    __syncthreads();

    if (moved) {
        double c = INFINITY;
        for (int j = 0; j < V; ++j) c = audit::min_nan(c, s_pair[a][j]);
        const int now = fleet::flag_after(D, flag, c);
        if (lane == 0 && c == c) D.agent_clear_hist[b * S + D.step] = c;
        if (now != flag) {                                           // wave-uniform
            if (lane == 0) D.flags[b] = now;
            loop::mask_rollout_wave(D.variant_out, D.xref_out, b, N1, D.x0[3 * b], D.x0[3 * b + 1], D.x0[3 * b + 2], lane);
        }
        flag = now;
    }
    if (lane == 0) s_flag[a] = flag;
    __syncthreads();
    if (!other) return;

    // ---- agents: slot Ks + lane of rollout (g, a) is car `lane` of the world
    const int64_t bj = g * V + lane, slot = b * K + D.Ks + lane;
    double A[2 * fleet::E], bb[fleet::E], v[2];
    fleet::agent_slot(D, a, lane, D.x0 + 3 * bj, s_flag[lane], D.u0[2 * bj], A, bb, v);
    double* oA = D.pool_A + slot * fleet::E * 2;
    double* ob = D.pool_b + slot * fleet::E;
    double* ov = D.pool_v + slot * 2;
#pragma unroll
    for (int q = 0; q < 2 * fleet::E; ++q) oA[q] = A[q];
#pragma unroll
    for (int q = 0; q < fleet::E; ++q) ob[q] = bb[q];
    ov[0] = v[0]; ov[1] = v[1];
}

}  // namespace

extern "C" void obca_fleet_init(obca_fleet* d) {
    if (d) fleet::init(d);
}

extern "C" int obca_fleet_step(const obca_fleet* d, int32_t measure, int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (fleet::args_check(d, measure) != 0 || device < 0) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(fleet_kernel, dim3((unsigned)d->G), dim3((unsigned)(d->V * WAVE)), 0, (hipStream_t)hip_stream, *d, measure);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
