// obca_pool_tracks.hip -- obca_pool_tracks of include/obca_mpc.h: the step between two solves of a closed loop over scene pools
// that turns timed tracks into the rows of the last Kt pool slots -- now, and at every stage of the next solve -- and measures
// what the car kept from the tracked obstacles.  The arithmetic and the serial definition are csrc/obca_pool_tracks_core.h.
//
// Layout: one wavefront per rollout, four per workgroup; a wavefront beyond B leaves at once.  There is no barrier and no LDS:
// a wavefront shares nothing with its neighbours.
//   states    track j = 0 .. Kt-1 in turn (wave-uniform): the lanes stride over its len knots, one __all decides; the Kt state
//             words are two wave-uniform 64-bit masks (Kt <= 64), so no lane holds a word another lane needs
//   measure   the lanes stride over the Kt (n_sub + 1) (slot, sample) pairs, skipping slots that are not usable; a butterfly
//             of audit::min_nan over the 64 lanes follows -- a NaN wins, otherwise the order plays no part -- so every lane
//             holds the serial fold's word and the flag decision is wave-uniform; lane 0 writes the history word, the flag and
//             the variant, the wavefront strides over the masked window
//   rows      the lanes stride over the Kt (N + 1) (slot, stage) pairs: one pose (a binary search in the track), one
//             fleet::car_rows (or the spare), 8 + 4 words stored by the lane that computed them; the lane of stage 0 also
//             writes the pool slot, its chord velocity, the mask word and the state word
// Every address is formed from an index below its bound: b < B, j < Kt, kk <= N, a knot index below len <= L, and no knot of a
// track is read before its length word and rectangle have passed their check.  The flag a wavefront reads is its own
// rollout's, and only its lane 0 writes it, after the read.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_pool_tracks_core.h"

namespace {

constexpr int BLOCK = 256, WAVE = 64, WAVES = BLOCK / WAVE;

__global__ void __launch_bounds__(BLOCK) pool_tracks_kernel(struct obca_pool_tracks D, int32_t measure) {
    const int lane = threadIdx.x % WAVE;
    const int64_t b = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
    if (b >= D.B) return;                                            // wave-uniform
    const int Kt = D.Kt, N1 = D.N + 1, S = D.max_steps;

    // ---- states
    const bool clock = ptracks::clock_usable(D, b);
    unsigned long long usable = 0, bad = 0;
    for (int j = 0; j < Kt; ++j) {
        const ptracks::Track T = ptracks::track_of(D, b, j);
        const bool frame = ptracks::frame_usable(T, D.L);            // wave-uniform
        bool knots = frame;
        if (frame)
            for (int i = lane; i < T.len; i += WAVE) knots = knots && ptracks::knot_usable(T, i);
        const int st = ptracks::state_word(T.len, frame, __all(knots) != 0, clock);
        if (st == 1) usable |= 1ull << j;
        if (st == -1) bad |= 1ull << j;
    }

    // ---- measure
    if (ptracks::measured(D, measure, b)) {                          // wave-uniform
        double cur = INFINITY;
        if (ptracks::car_there(D, b)) {
            const int ns1 = D.n_sub + 1;
            for (int p = lane; p < Kt * ns1; p += WAVE) {
                const int j = p / ns1, s = p - j * ns1;
                if (!((usable >> j) & 1ull)) continue;
                cur = audit::min_nan(cur, ptracks::sample_clear(D, b, ptracks::track_of(D, b, j), s));
            }
        }
        for (int off = WAVE / 2; off > 0; off >>= 1) cur = audit::min_nan(cur, __shfl_xor(cur, off, WAVE));
        const int was = D.flags[b], now = ptracks::flag_after(D, was, cur);
        if (lane == 0 && cur == cur) D.track_clear_hist[b * S + D.step] = cur;
        if (now != was) {                                            // wave-uniform
            if (lane == 0) D.flags[b] = now;
            loop::mask_rollout_wave(D.variant_out, D.xref_out, b, N1, D.x0[3 * b], D.x0[3 * b + 1], D.x0[3 * b + 2], lane);
        }
    }

    // ---- rows: (slot, stage) pairs
    for (int p = lane; p < Kt * N1; p += WAVE) {
        const int j = p / N1, kk = p - j * N1;
        const ptracks::Track T = ptracks::track_of(D, b, j);
        const bool use = ((usable >> j) & 1ull) != 0;
        const int64_t sj = b * Kt + j;
        double p0[3] = {0.0, 0.0, 0.0}, A[2 * ptracks::E], bb[ptracks::E];
        ptracks::stage_rows(D, b, use, T, kk, p0, A, bb);
        double* oA = D.stage_A + (sj * N1 + kk) * ptracks::E * 2;
        double* ob = D.stage_b + (sj * N1 + kk) * ptracks::E;
#pragma unroll
        for (int r = 0; r < 2 * ptracks::E; ++r) oA[r] = A[r];
#pragma unroll
        for (int r = 0; r < ptracks::E; ++r) ob[r] = bb[r];
        if (kk != 0) continue;
        const int64_t slot = b * D.K + (D.K - Kt) + j;              // stage 0's rows are the pool slot's
        double* pA = D.pool_A + slot * ptracks::E * 2;
        double* pb = D.pool_b + slot * ptracks::E;
#pragma unroll
        for (int r = 0; r < 2 * ptracks::E; ++r) pA[r] = A[r];
#pragma unroll
        for (int r = 0; r < ptracks::E; ++r) pb[r] = bb[r];
        double p1[3] = {0.0, 0.0, 0.0}, v[2];
        if (use) ptracks::pose_at(T, ptracks::stage_time(D, b, 1), p1);
        ptracks::chord_velocity(D, b, use, p0, p1, v);
        D.pool_v[slot * 2] = v[0];
        D.pool_v[slot * 2 + 1] = v[1];
        D.stage_ok[sj] = ptracks::ok_word(D, use);
        D.track_state[sj] = use ? 1 : (((bad >> j) & 1ull) ? -1 : 0);
    }
}

}  // namespace

extern "C" void obca_pool_tracks_init(struct obca_pool_tracks* d) {
    if (d) ptracks::init(d);
}

extern "C" int obca_pool_tracks(const struct obca_pool_tracks* d, int32_t measure, int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (ptracks::args_check(d, measure) != 0 || device < 0) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    const unsigned blocks = (unsigned)((d->B + WAVES - 1) / WAVES);
    hipLaunchKernelGGL(pool_tracks_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, *d, measure);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
