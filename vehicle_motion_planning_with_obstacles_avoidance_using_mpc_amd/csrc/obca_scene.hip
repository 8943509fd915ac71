// obca_scene.hip -- obca_scene_select of include/obca_mpc.h: the step in front of a solve that decides which obstacles of a
// pool of up to 64 the solve sees, and gathers their rows.  The arithmetic is csrc/obca_scene_core.h.
//
// Layout: one wavefront per instance, lane = pool obstacle (hence K <= 64), blocks of 256 = four instances.  Every lane
// loops over the samples for its own obstacle (all lanes read the same poses: cache hits after the first).  Ranking: the
// scores go through LDS (4 x 64 doubles per block, this call's values beside them for min_clear) and every lane counts the
// scores that beat its own -- broadcast reads, no atomics.  The slot of a selected lane is the popcount of the 64-bit ballot
// of selected lanes below it, so sel comes out ascending.  Gather: the wavefront strides over its instance's
// (N + 1) n_sel E output rows, so the stores run along the last axis: one 16-byte store per row of A_out, one 8-byte store
// per b_out.  Wavefronts beyond the batch run through the two barriers and touch no memory.
//
// obca_scene_select_staged launches scene_kernel<true>: the last Kt lanes of the wavefront may read a track (rows per stage)
// in place of their pool rows.  Those lanes score with scene::score_track (E a compile-time constant there too: the two row
// sets of an interval live in registers), the others with scene::score_obstacle -- the wavefront runs the two paths one after
// the other.  The gather of a selected staged slot copies the track's stage rows.  obca_scene_select launches
// scene_kernel<false>, in which every staged branch is compiled out.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_scene_core.h"

namespace {

constexpr int BLOCK = 256, WAVE = 64, PER_BLOCK = BLOCK / WAVE;

struct SceneArgs {
    int32_t B, K, E, N, n_sel, n_sub, accumulate;
    double ego[4];
    const double *pool_A, *pool_b, *pool_v, *Ts, *x, *x0;
    const int32_t *variant, *status;
    double* score;
    int32_t* sel;
    double *A_out, *b_out;
    int32_t *variant_out, *ok_out;
    double* min_clear;
    // obca_scene_select_staged only
    int32_t Kt, stage_group;
    const double *stage_A, *stage_b;
    const int32_t* stage_ok;
};

template <bool STAGED>
__global__ void __launch_bounds__(BLOCK) scene_kernel(SceneArgs P) {
    __shared__ double s_score[PER_BLOCK][WAVE], s_cur[PER_BLOCK][WAVE];
    __shared__ int32_t s_sel[PER_BLOCK][scene::MAX_SEL];
    const int w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t inst = (int64_t)blockIdx.x * PER_BLOCK + w;
    const bool live = inst < P.B;                                    // wave-uniform
    const bool mine = live && lane < P.K;
    const int K = P.K, E = P.E, N1 = P.N + 1, n_sel = P.n_sel;

    const double* pA = live ? P.pool_A + inst * K * E * 2 : nullptr;
    const double* pb = live ? P.pool_b + inst * K * E : nullptr;
    const double* pv = live && P.pool_v ? P.pool_v + inst * K * 2 : nullptr;
    const double Ts = live && P.pool_v ? P.Ts[inst] : 0.0;
    const int variant = live ? (P.variant ? P.variant[inst] : 6) : 0;
    const int status = live && P.status ? P.status[inst] : 0;

    // the track of a staged lane, and the instance's stage_ok words for the gather
    const double *sA = nullptr, *sb = nullptr;
    const int32_t* s_ok = nullptr;
    if constexpr (STAGED) {
        if (live && P.Kt > 0) s_ok = P.stage_ok + inst * P.Kt;
        const int t = mine ? scene::staged_slot(lane, K, P.Kt, s_ok) : -1;
        if (t >= 0) {
            sA = scene::track_A_of(P.stage_A, inst / P.stage_group, P.Kt, t, N1, E);
            sb = scene::track_b_of(P.stage_b, inst / P.stage_group, P.Kt, t, N1, E);
        }
    }

    // usable pool: every obstacle's numbers and the step length
    bool fin = !mine || scene::obstacle_finite(pA + 2 * lane * E, pb + lane * E, pv ? pv + 2 * lane : nullptr, E);
    if constexpr (STAGED) fin = fin && (!sA || scene::track_finite(sA, sb, N1, E));
    bool usable = live && __all(fin) && (!pv || scene::finite_(Ts));
    const bool measured = usable && (!P.accumulate || scene::active(variant, status));

    double cur = INFINITY, sc = INFINITY;
    if (measured && mine) {
        int n_pose = 0;
        if (STAGED && sA)
            cur = scene::score_track_obstacle(E, sA, sb, P.x + inst * 3 * N1, P.N, P.x0 ? P.x0 + inst * 3 : nullptr, P.n_sub,
                                              variant == 4, P.ego, &n_pose);
        else
            cur = scene::score_obstacle(E, pA + 2 * lane * E, pb + lane * E, pv ? pv + 2 * lane : nullptr, Ts, P.x + inst * 3 * N1, P.N,
                                        P.x0 ? P.x0 + inst * 3 : nullptr, P.n_sub, variant == 4, P.ego, &n_pose);
        if (n_pose == 0) cur = NAN;                                  // no finite pose: the same in every lane
    }
    if (measured && __any(mine && cur != cur)) usable = false;
    const bool rank_it = measured && usable;
    if (rank_it && mine) {
        sc = P.accumulate ? scene::score_min(P.score[inst * K + lane], cur) : cur;
        P.score[inst * K + lane] = sc;
    }
    s_score[w][lane] = sc;                                           // +inf beyond K: never read below K's loop
    s_cur[w][lane] = cur;
    __syncthreads();

    // selection: ranked anew, or the one passed in
    bool changed = false;
    if (rank_it) {
        const bool chosen = mine && scene::rank_of(s_score[w], K, lane) < n_sel;
        const unsigned long long mask = __ballot(chosen);
        const int slot = __popcll(mask & ((1ull << lane) - 1ull));
        bool differs = false;
        if (chosen) {
            differs = !P.accumulate || P.sel[inst * n_sel + slot] != lane;
            s_sel[w][slot] = lane;
        }
        changed = __any(differs);
        if (chosen && differs) P.sel[inst * n_sel + slot] = lane;
    } else if (live) {
        bool ok = true;
        if (usable && lane < n_sel) {                                // accumulate, not measured: keep the selection passed in
            const int32_t v = P.sel[inst * n_sel + lane];
            const int32_t below = lane > 0 ? P.sel[inst * n_sel + lane - 1] : -1;
            ok = v >= 0 && v < K && v > below;
            s_sel[w][lane] = v;
        }
        usable = usable && __all(ok);
        if (!usable && lane < n_sel) P.sel[inst * n_sel + lane] = lane;
    }
    if (live && lane == 0) {
        P.variant_out[inst] = changed ? variant : 0;
        P.ok_out[inst] = usable ? 1 : 0;
        if (P.min_clear) {
            double mc = NAN;
            if (rank_it) {
                mc = INFINITY;
                for (int j = 0; j < K; ++j) mc = audit::dmin_(mc, s_cur[w][j]);
            }
            P.min_clear[inst] = mc;
        }
    }
    __syncthreads();

    // gather
    if (!live) return;
    const int per_stage = n_sel * E, rows = N1 * per_stage;
    double* Ao = P.A_out + inst * rows * 2;
    double* bo = P.b_out + inst * rows;
    for (int q = lane; q < rows; q += WAVE) {
        const int kk = q / per_stage, c = q - kk * per_stage, slot = c / E, r = c - slot * E;
        double a[2], b;
        const int i = usable ? s_sel[w][slot] : 0;
        const int t = (STAGED && usable) ? scene::staged_slot(i, K, P.Kt, s_ok) : -1;
        if (STAGED && t >= 0)
            scene::out_row_track(scene::track_A_of(P.stage_A, inst / P.stage_group, P.Kt, t, N1, E),
                                 scene::track_b_of(P.stage_b, inst / P.stage_group, P.Kt, t, N1, E), E, r, kk, a, &b);
        else
            scene::out_row(pA, pb, pv, Ts, E, i, r, kk, usable, a, &b);
        *reinterpret_cast<double2*>(Ao + 2 * q) = make_double2(a[0], a[1]);
        bo[q] = b;
    }
}

int launch(const SceneArgs& P, bool staged, int32_t device, void* hip_stream) {
    const int64_t blocks = ((int64_t)P.B + PER_BLOCK - 1) / PER_BLOCK;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    if (staged)
        hipLaunchKernelGGL(scene_kernel<true>, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, P);
    else
        hipLaunchKernelGGL(scene_kernel<false>, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, P);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}

SceneArgs pack(const double ego[4], int32_t B, int32_t K, int32_t E, int32_t N, int32_t n_sel, int32_t n_sub, int32_t accumulate,
               const double* pool_A, const double* pool_b, const double* pool_v, const double* Ts, const double* x, const double* x0,
               const int32_t* variant, const int32_t* status, double* score, int32_t* sel, double* A_out, double* b_out,
               int32_t* variant_out, int32_t* ok_out, double* min_clear) {
    SceneArgs P;
    P.B = B; P.K = K; P.E = E; P.N = N; P.n_sel = n_sel; P.n_sub = n_sub; P.accumulate = accumulate;
    for (int q = 0; q < 4; ++q) P.ego[q] = ego[q];
    P.pool_A = pool_A; P.pool_b = pool_b; P.pool_v = pool_v; P.Ts = Ts; P.x = x; P.x0 = x0;
    P.variant = variant; P.status = status; P.score = score; P.sel = sel; P.A_out = A_out; P.b_out = b_out;
    P.variant_out = variant_out; P.ok_out = ok_out; P.min_clear = min_clear;
    P.Kt = 0; P.stage_group = 1; P.stage_A = nullptr; P.stage_b = nullptr; P.stage_ok = nullptr;
    return P;
}

}  // namespace

extern "C" int obca_scene_select(const double ego[4], int32_t B, int32_t K, int32_t E, int32_t N, int32_t n_sel, int32_t n_sub,
                                 int32_t accumulate, const double* pool_A, const double* pool_b, const double* pool_v,
                                 const double* Ts, const double* x, const double* x0, const int32_t* variant,
                                 const int32_t* status, double* score, int32_t* sel, double* A_out, double* b_out,
                                 int32_t* variant_out, int32_t* ok_out, double* min_clear, int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (scene::args_check(B, K, E, N, n_sel, n_sub, accumulate, ego, pool_A, pool_b, pool_v, Ts, x, score, sel, A_out, b_out,
                          variant_out, ok_out) != 0 || device < 0)
        return OBCA_E_INVAL;
    return launch(pack(ego, B, K, E, N, n_sel, n_sub, accumulate, pool_A, pool_b, pool_v, Ts, x, x0, variant, status, score, sel, A_out,
                       b_out, variant_out, ok_out, min_clear), false, device, hip_stream);
}

extern "C" int obca_scene_select_staged(const double ego[4], int32_t B, int32_t K, int32_t E, int32_t N, int32_t n_sel, int32_t n_sub,
                                        int32_t accumulate, const double* pool_A, const double* pool_b, const double* pool_v,
                                        const double* Ts, const double* x, const double* x0, const int32_t* variant,
                                        const int32_t* status, int32_t Kt, int32_t stage_group, const double* stage_A,
                                        const double* stage_b, const int32_t* stage_ok, double* score, int32_t* sel, double* A_out,
                                        double* b_out, int32_t* variant_out, int32_t* ok_out, double* min_clear, int32_t device,
                                        void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (scene::args_check(B, K, E, N, n_sel, n_sub, accumulate, ego, pool_A, pool_b, pool_v, Ts, x, score, sel, A_out, b_out,
                          variant_out, ok_out) != 0 || scene::staged_args_check(B, K, Kt, stage_group, stage_A, stage_b, stage_ok) != 0 ||
        device < 0)
        return OBCA_E_INVAL;
    SceneArgs P = pack(ego, B, K, E, N, n_sel, n_sub, accumulate, pool_A, pool_b, pool_v, Ts, x, x0, variant, status, score, sel, A_out,
                       b_out, variant_out, ok_out, min_clear);
    P.Kt = Kt; P.stage_group = stage_group; P.stage_A = stage_A; P.stage_b = stage_b; P.stage_ok = stage_ok;
    return launch(P, true, device, hip_stream);
}
