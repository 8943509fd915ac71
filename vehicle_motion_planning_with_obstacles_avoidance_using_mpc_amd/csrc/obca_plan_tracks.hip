// obca_plan_tracks.hip -- obca_plan_tracks of include/obca_mpc.h: a batch of open-loop plans measured against timed tracks
// themselves -- the track's own rectangle at the track's pose at every sample's time -- with the running minimum
// obca_scene_select_staged re-ranks on.  The arithmetic and the serial definition are csrc/obca_plan_tracks_core.h.
//
// Layout: one wavefront per plan, four per workgroup; a wavefront beyond B leaves at once.  There is no barrier and no LDS:
// a wavefront shares nothing with its neighbours.
//   states    track j = 0 .. Kt-1 in turn (wave-uniform): the lanes stride over its len knots, one __all decides; the Kt state
//             words are two wave-uniform 64-bit masks (Kt <= 64); lane j writes track_state[b,j]
//   poses     the lanes stride over the N (n_sub + 1) (interval, sample) pairs, plus one for x0: one __any says whether the
//             plan has a finite sample pose at all
//   measure   the usable tracks in turn (wave-uniform): the lanes stride over the same samples with a lane-local
//             audit::min_nan, a butterfly of audit::min_nan over the 64 lanes follows -- a NaN wins, otherwise the order plays
//             no part -- so every lane holds the serial fold's word; lane j keeps track j's word, and the fold over the tracks
//             is a wave-uniform scalar
//   outputs   lane j < Kt writes track_clear[b,j] and folds score[b,K-Kt+j], lane 0 writes track_min[b]
// Every address is formed from an index below its bound: b < B, j < Kt, a sample's interval s < N (knots s and s + 1 <= N), a
// knot index below len <= L, and no knot of a track is read before its length word and rectangle have passed their check.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_plan_tracks_core.h"

namespace {

constexpr int BLOCK = 256, WAVE = 64, WAVES = BLOCK / WAVE;

__global__ void __launch_bounds__(BLOCK) plan_tracks_kernel(struct obca_plan_tracks D) {
    const int lane = threadIdx.x % WAVE;
    const int64_t b = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
    if (b >= D.B) return;                                            // wave-uniform
    const int Kt = D.Kt;

    // ---- states
    const bool clock = plantracks::clock_usable(D, b);
    unsigned long long usable = 0, bad = 0;
    for (int j = 0; j < Kt; ++j) {
        const ptracks::Track T = plantracks::track_of(D, b, j);
        const bool frame = ptracks::frame_usable(T, D.L);            // wave-uniform
        bool knots = frame;
        if (frame)
            for (int i = lane; i < T.len; i += WAVE) knots = knots && ptracks::knot_usable(T, i);
        const int st = ptracks::state_word(T.len, frame, __all(knots) != 0, clock);
        if (st == 1) usable |= 1ull << j;
        if (st == -1) bad |= 1ull << j;
    }
    const bool mine_usable = lane < Kt && ((usable >> lane) & 1ull) != 0;
    if (lane < Kt) D.track_state[b * Kt + lane] = mine_usable ? 1 : (((bad >> lane) & 1ull) ? -1 : 0);

    // ---- poses, measure
    const int np = plantracks::n_samples(D);
    bool ok = plantracks::measured(D, b);                            // wave-uniform
    double fold = INFINITY, mine = INFINITY;                         // mine: track `lane`'s word
    if (ok) {
        bool posed = false;
        for (int p = lane; p < np; p += WAVE) {
            double pose[3], when;
            posed = plantracks::sample_of(D, b, p, pose, &when) || posed;
        }
        ok = __any(posed) != 0;
    }
    if (ok)
        for (int j = 0; j < Kt; ++j) {
            if (!((usable >> j) & 1ull)) continue;                   // wave-uniform
            const ptracks::Track T = plantracks::track_of(D, b, j);
            double cur = INFINITY;
            for (int p = lane; p < np; p += WAVE) cur = audit::min_nan(cur, plantracks::sample_clear(D, b, T, p));
            for (int off = WAVE / 2; off > 0; off >>= 1) cur = audit::min_nan(cur, __shfl_xor(cur, off, WAVE));
            if (lane == j) mine = cur;
            fold = audit::min_nan(fold, cur);
        }
    ok = ok && fold == fold;

    // ---- outputs
    if (lane < Kt) {
        D.track_clear[b * Kt + lane] = ok ? mine : NAN;
        if (ok && D.score && mine_usable) {
            double* sc = D.score + b * D.K + (D.K - Kt) + lane;
            *sc = plantracks::score_fold(*sc, mine);
        }
    }
    if (lane == 0) D.track_min[b] = ok ? fold : NAN;
}

}  // namespace

extern "C" void obca_plan_tracks_init(struct obca_plan_tracks* d) {
    if (d) plantracks::init(d);
}

extern "C" int obca_plan_tracks(const struct obca_plan_tracks* d, int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (plantracks::args_check(d) != 0 || device < 0) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    const unsigned blocks = (unsigned)((d->B + WAVES - 1) / WAVES);
    hipLaunchKernelGGL(plan_tracks_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, *d);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
