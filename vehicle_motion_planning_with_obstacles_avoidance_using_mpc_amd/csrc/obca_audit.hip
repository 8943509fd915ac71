// obca_audit.hip -- collision audit (obca_plan_clearance, obca_plan_sweep, obca_rollouts_audit of include/obca_mpc.h): true
// clearance of batched plans (at the knots; swept between them) and of closed-loop rollouts in fp64, and the clearance repair's
// round (obca_plan_tighten: measure, grow the rows), from the geometry core csrc/obca_audit_core.h.  Read-only towards the
// solver and the rollouts: the kernels only read their outputs and state and write the caller's output buffers.
//
// Layout: the lanes of a wavefront are cut into segments of seg = next power of two >= the items of one instance (plan:
// its N + 1 stages, plan sweep: its N intervals, rollout: its max_steps intervals; at most 64), one instance per segment;
// a lane walks the items sub, sub + seg, ... of its instance (for an interval: its samples in order, both ends of every
// sub-interval in registers), then the segment reduces min / arg-min with xor shuffles that never leave it (seg_reduce).
//
// The three plan calls take the same batch: audit::PlanBatch of csrc/obca_plan_batch.h, which validates it once
// (plan_batch_init) and is the only code that indexes x / A / b -- for the kernels here and for the host shims of
// tests/native alike.  Every entry point is: its own checks, the batch's (plan calls), its own fields, launch_segments.
// Every check comes before the first HIP call, so a refused call has no side effect.
#include <hip/hip_runtime.h>
#include <math.h>
#include "obca_device.h"
#include "obca_plan_batch.h"

// defined in obca_rollout.hip (internal, not part of the C ABI): the handle's device-state descriptor, its shape and the
// parameters of its last obca_rollouts_reset; OBCA_E_INVAL when the handle has not been reset
int obca_internal_rollouts_view(const obca_rollouts* r, rollout::Dev* D, obca_rollout_dims* dims, obca_params* params);

namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;

using audit::PlanBatch;

struct PlanArgs {
    PlanBatch P;
    double* min_clear;
    int32_t *arg_stage, *arg_obst;
    double* stage_obst;
};

struct SweepArgs {
    PlanBatch P;
    int32_t n_sub;
    double *min_clear, *lower_bound;
    int32_t *arg_interval, *arg_obst, *first_collision;
    double* interval_min;
};

struct TightenArgs {
    PlanBatch P;
    int32_t n_sub, certified;
    double target, gain, grow_max;
    const int32_t* status;
    double *grow, *b_out;
    int32_t* variant_out;
    double* min_clear;
};

struct AuditArgs {
    rollout::Dev D;
    int32_t n_static;
    int32_t m[OBCA_MAX_OBST];
    double ego[4];
    double dmin;
    int32_t n_sub, seg, log_seg;
    double *min_clear, *lower_bound;
    int32_t *arg_step, *arg_obst, *first_collision, *first_violation;
    double* step_min;
};

using audit::better;

__device__ inline void seg_argmin(double& v, int& s, int& o, int seg) {
    for (int w = seg >> 1; w > 0; w >>= 1) {
        const double v2 = __shfl_xor(v, w, WAVE);
        const int s2 = __shfl_xor(s, w, WAVE), o2 = __shfl_xor(o, w, WAVE);
        if (better(v2, s2, o2, v, s, o)) { v = v2; s = s2; o = o2; }
    }
}

// v op its partner's v, halving the distance until every lane of the segment holds the segment's value
template <class T, class Op>
__device__ inline T seg_reduce(T v, int seg, Op op) {
    for (int w = seg >> 1; w > 0; w >>= 1) v = op(v, __shfl_xor(v, w, WAVE));
    return v;
}

__device__ inline double seg_min(double v, int seg) { return seg_reduce(v, seg, [](double a, double b) { return fmin(a, b); }); }
__device__ inline double seg_max(double v, int seg) { return seg_reduce(v, seg, [](double a, double b) { return fmax(a, b); }); }
// a NaN in the segment wins
__device__ inline double seg_min_nan(double v, int seg) { return seg_reduce(v, seg, [](double a, double b) { return audit::min_nan(a, b); }); }
// smallest index >= 0, -1 if none: as unsigned, -1 is the largest
__device__ inline int seg_min_nonneg(int v, int seg) { return (int)seg_reduce((unsigned)v, seg, [](unsigned a, unsigned b) { return b < a ? b : a; }); }
__device__ inline int seg_or(int v, int seg) { return seg_reduce(v, seg, [](int a, int b) { return a | b; }); }

// the instance of this lane's segment and the lane's place in it.  Whole segments are live (inst < B) or not, so the
// shuffles of a reduction stay uniform.
struct Lane {
    int64_t inst;
    int sub;
};

__device__ inline Lane lane_of(const PlanBatch& P) {
    const int64_t gl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    return {gl >> P.log_seg, (int)(gl & (P.seg - 1))};
}

__global__ void __launch_bounds__(BLOCK) plan_clearance_kernel(PlanArgs G) {
    const PlanBatch& P = G.P;
    const auto [inst, sub] = lane_of(P);
    const bool live = inst < P.B;
    double best = INFINITY;
    int bs = 0x7fffffff, bo = 0x7fffffff;
    if (live) {
        const int v = audit::plan_variant(P, inst);
        const size_t st0 = audit::plan_first(P, inst);
        for (int k = sub; k <= P.N; k += P.seg) {
            double p[3], C[4][2];
            audit::plan_pose(P, inst, k, p);
            audit::car_corners(p[0], p[1], p[2], P.ego, C);
            const audit::PlanRows R = audit::plan_rows(P, st0, k, v, 0);
            for (int i = 0; i < P.n_obs; ++i) {
                const double d = audit::plan_distance<OBCA_MAX_EDGES>(C, R.A0 + 2 * P.off[i], R.b0 + P.off[i], P.m[i]);
                if (G.stage_obst) G.stage_obst[(st0 + k) * P.n_obs + i] = d;
                if (better(d, k, i, best, bs, bo)) { best = d; bs = k; bo = i; }
            }
        }
    }
    seg_argmin(best, bs, bo, P.seg);
    if (live && sub == 0) {
        G.min_clear[inst] = best;
        G.arg_stage[inst] = bs;
        G.arg_obst[inst] = bo;
    }
}

// one lane per (instance, interval): audit::plan_interval on the plan's own arrays, the rows of both stages read in place
__global__ void __launch_bounds__(BLOCK) plan_sweep_kernel(SweepArgs G) {
    const PlanBatch& P = G.P;
    const auto [inst, sub] = lane_of(P);
    const bool live = inst < P.B;
    audit::PlanSweepAcc acc;
    audit::plan_acc_init(acc);
    if (live) {
        const int v = audit::plan_variant(P, inst);
        const audit::PlanScene sc = audit::plan_scene(P);
        const size_t st0 = audit::plan_first(P, inst);
        for (int s = sub; s < P.N; s += P.seg) {
            double p0[3], p1[3];
            audit::plan_pose(P, inst, s, p0);
            audit::plan_pose(P, inst, s + 1, p1);
            const audit::PlanRows R = audit::plan_rows(P, st0, s, v);
            const audit::PlanIntervalResult I = audit::plan_interval<OBCA_MAX_EDGES>(sc, p0, p1, R.A0, R.b0, R.A1, R.b1, G.n_sub);
            if (G.interval_min) G.interval_min[(size_t)inst * P.N + s] = I.min_val;
            audit::plan_acc_add(acc, s, I);
        }
    }
    seg_argmin(acc.best, acc.bs, acc.bo, P.seg);
    acc.lower = seg_min_nan(acc.lower, P.seg);
    acc.coll = seg_min_nonneg(acc.coll, P.seg);
    if (live && sub == 0) {
        G.min_clear[inst] = acc.best;
        G.lower_bound[inst] = acc.lower;
        G.arg_interval[inst] = acc.bs;
        G.arg_obst[inst] = acc.bo;
        G.first_collision[inst] = acc.coll;
    }
}

// Clearance repair (audit::plan_tighten_* of csrc/obca_audit_core.h).  plan_sweep_kernel's layout: lane `sub` of a segment
// owns the intervals s = sub, sub + seg, ... of its instance and with interval s the stage s (with interval N - 1 stage N as
// well).  Two phases, because whether the instance is repaired at all (a NaN anywhere passes it through) and obca_mpc4's
// need (the largest over all intervals) are known only after every interval is measured:
//   1  d[s,i] of the lane's intervals, parked in b_out[inst, s, off[i]] -- the first row of obstacle i at stage s, which
//      this lane alone reads back and overwrites in phase 2 (hence b_out must not alias b) -- and the segment's min_clear
//   2  per obstacle: need[s,i] from the parked d; stage s wants need[s-1,i] as well, which is the left lane's of the same
//      pass, or for lane 0 the last lane's of the pass before (kept in `carry`): one rotate-by-one shuffle inside the
//      segment, in which the last lane sends its carry and every other lane its current need.
// Every shuffle sits outside the per-instance conditions and the pass loops have the same trip count in every lane, so
// all 64 lanes reach each one.
__global__ void __launch_bounds__(BLOCK) plan_tighten_kernel(TightenArgs G) {
    const PlanBatch& P = G.P;
    const auto [inst, sub] = lane_of(P);
    const bool live = inst < P.B;
    const int N = P.N, seg = P.seg;
    const int v = live ? audit::plan_variant(P, inst) : 0;
    const bool v4 = audit::plan_reads_stage0(v);                 // its need is the largest over all intervals, at every stage
    const bool active = live && audit::plan_tighten_active(v, G.status[inst]);
    const size_t st0 = live ? audit::plan_first(P, inst) : 0;
    const audit::PlanScene sc = audit::plan_scene(P);
    double mc = active ? INFINITY : NAN;
    if (active) {
        const double rmax = audit::car_radius(P.ego);
        for (int s = sub; s < N; s += seg) {
            double p0[3], p1[3];
            audit::plan_pose(P, inst, s, p0);
            audit::plan_pose(P, inst, s + 1, p1);
            const audit::PlanRows R = audit::plan_rows(P, st0, s, v);
            for (int i = 0; i < P.n_obs; ++i) {
                const double d = audit::plan_tighten_distance<OBCA_MAX_EDGES>(sc, i, p0, p1, R.A0, R.b0, R.A1, R.b1, G.n_sub,
                                                                              G.certified, rmax);
                G.b_out[(st0 + s) * P.M + P.off[i]] = d;
                mc = audit::min_nan(mc, d);
            }
        }
    }
    mc = seg_min_nan(mc, seg);
    const bool ok = active && mc == mc;                          // repaired; otherwise passed through
    int rose = 0;
    for (int i = 0; i < P.n_obs; ++i) {
        const int o = P.off[i];
        double nmax = 0.0;
        if (ok)
            for (int s = sub; s < N; s += seg)
                nmax = fmax(nmax, audit::plan_tighten_need(G.b_out[(st0 + s) * P.M + o], G.target, G.gain));
        nmax = seg_max(nmax, seg);
        double carry = 0.0;
        for (int s0 = 0; s0 < N; s0 += seg) {
            const int s = s0 + sub;
            const bool has = live && s < N;
            const double nd = (ok && has) ? audit::plan_tighten_need(G.b_out[(st0 + s) * P.M + o], G.target, G.gain) : 0.0;
            const double left = __shfl(sub == seg - 1 ? carry : nd, (sub - 1) & (seg - 1), seg);
            carry = nd;
            if (has) {
                const size_t k = st0 + s;
                const audit::PlanRows own = audit::plan_rows(P, st0, s, 0);          // variant 0: stage s's and s + 1's own rows
                rose |= audit::plan_tighten_stage(own.A0 + 2 * o, own.b0 + o, P.m[i], v4 ? nmax : fmax(left, nd), G.grow_max, ok,
                                                  G.grow + k * P.n_obs + i, G.b_out + k * P.M + o);
                if (s == N - 1)
                    rose |= audit::plan_tighten_stage(own.A1 + 2 * o, own.b1 + o, P.m[i], v4 ? nmax : nd, G.grow_max, ok,
                                                      G.grow + (k + 1) * P.n_obs + i, G.b_out + (k + 1) * P.M + o);
            }
        }
    }
    rose = seg_or(rose, seg);
    if (live && sub == 0) {
        G.variant_out[inst] = rose ? v : 0;
        if (G.min_clear) G.min_clear[inst] = mc;
    }
}

// boxes of rollout b at knot kn: the recorded history where the harness recorded it, else the harness's update law
// from the previous knot (the last knot), else (knot 0 of a rollout that never stepped) the tuple itself
__device__ inline void boxes_at(const AuditArgs& G, int b, int kn, int steps, int flags, double box[OBCA_MAX_DYN][3]) {
    const rollout::Dev& D = G.D;
    const int nd = D.n_dyn, S = D.S;
    const bool recorded = kn < steps || (kn == steps && flags == OBCA_DONE_FAILED && kn < S);
    for (int i = 0; i < nd; ++i) {
        const double* info = D.dyn + ((size_t)b * nd + i) * rollout::DYN_W;
        if (recorded) {
            const double* rec = D.dh + (((size_t)b * S + kn) * nd + i) * 4;
            box[i][0] = rec[0]; box[i][1] = rec[1]; box[i][2] = rec[2];
        } else if (kn >= 1) {
            const double* rec = D.dh + (((size_t)b * S + kn - 1) * nd + i) * 4;
            audit::box_next_knot(info, rec[0], rec[1], kn, D.Tc[(size_t)b * S + kn - 1], box[i]);
        } else {
            box[i][0] = info[0]; box[i][1] = info[1]; box[i][2] = (0.0 >= info[9]) ? 1.0 : 0.0;
        }
    }
}

__global__ void __launch_bounds__(BLOCK) rollouts_audit_kernel(AuditArgs G) {
    const rollout::Dev& D = G.D;
    const int gl = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = gl >> G.log_seg, sub = gl & (G.seg - 1);
    const bool live = b < D.B;
    const int S = D.S;
    double best = INFINITY, lower = INFINITY;
    int bs = 0x7fffffff, bo = 0x7fffffff, coll = -1, viol = -1;
    if (live) {
        int steps = D.k[b];
        steps = steps < 0 ? 0 : (steps > S ? S : steps);
        const int flags = D.flags[b];
        const int n_int = steps > 0 ? steps : 1;
        audit::Scene sc;
        sc.ego = G.ego;
        sc.n_static = G.n_static;
        sc.m = G.m;
        sc.As = D.As + (size_t)b * D.Ms * 2;
        sc.bs = D.bs + (size_t)b * D.Ms;
        sc.nd = D.n_dyn;
        sc.dyn = D.dyn + (size_t)b * D.n_dyn * rollout::DYN_W;
        const double viol_at = G.dmin - audit::VIOL_TOL;
        for (int s = sub; s < S; s += G.seg) {
            if (s >= n_int) {
                if (G.step_min) G.step_min[(size_t)b * S + s] = INFINITY;
                continue;
            }
            const bool single = steps == 0;
            const double* p0 = D.xc + ((size_t)b * (S + 1) + s) * 3;
            const double* p1 = single ? p0 : p0 + 3;
            double b0[OBCA_MAX_DYN][3], b1[OBCA_MAX_DYN][3];
            boxes_at(G, b, s, steps, flags, b0);
            if (single) {
                for (int i = 0; i < D.n_dyn; ++i) for (int q = 0; q < 3; ++q) b1[i][q] = b0[i][q];
            } else {
                boxes_at(G, b, s + 1, steps, flags, b1);
            }
            const audit::IntervalResult R = audit::audit_interval<OBCA_MAX_EDGES>(sc, p0, p1, b0, b1, single ? 0 : G.n_sub);
            if (G.step_min) G.step_min[(size_t)b * S + s] = R.min_val;
            if (better(R.min_val, s, R.min_obst, best, bs, bo)) { best = R.min_val; bs = s; bo = R.min_obst; }
            lower = fmin(lower, R.lower);
            if (coll < 0 && R.min_val < 0.0) coll = s;
            if (viol < 0 && R.d0 < viol_at) viol = s;
            if (viol < 0 && !single && s + 1 == n_int && R.d1 < viol_at) viol = s + 1;
        }
    }
    seg_argmin(best, bs, bo, G.seg);
    lower = seg_min(lower, G.seg);
    coll = seg_min_nonneg(coll, G.seg);
    viol = seg_min_nonneg(viol, G.seg);
    if (live && sub == 0) {
        G.min_clear[b] = best;
        G.lower_bound[b] = lower;
        G.arg_step[b] = bs;
        G.arg_obst[b] = bo;
        G.first_collision[b] = coll;
        G.first_violation[b] = viol;
    }
}

// one segment of seg lanes per instance; OBCA_E_INVAL (before any HIP call) when that is more blocks than one launch takes
template <class Args>
int launch_segments(void (*kernel)(Args), const Args& args, int64_t instances, int seg, int device, void* hip_stream) {
    const int64_t blocks = (instances * seg + BLOCK - 1) / BLOCK;
    if (blocks > 0x7fffffff) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, args);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}

}  // namespace

extern "C" int obca_plan_clearance(const double ego[4], int32_t n_obs, const int32_t* m, int32_t N, int32_t B,
                                   const int32_t* variant, const double* x, const double* A, const double* b,
                                   double* min_clear, int32_t* arg_stage, int32_t* arg_obst, double* stage_obst,
                                   int32_t device, void* hip_stream) {
    PlanArgs G;
    if (device < 0 || !min_clear || !arg_stage || !arg_obst ||
        audit::plan_batch_init(&G.P, ego, n_obs, m, N, B, variant, x, A, b, (int64_t)N + 1) != OBCA_OK)
        return OBCA_E_INVAL;
    G.min_clear = min_clear; G.arg_stage = arg_stage; G.arg_obst = arg_obst; G.stage_obst = stage_obst;
    return launch_segments(plan_clearance_kernel, G, B, G.P.seg, device, hip_stream);
}

extern "C" int obca_plan_sweep(const double ego[4], int32_t n_obs, const int32_t* m, int32_t N, int32_t B,
                               const int32_t* variant, const double* x, const double* A, const double* b, int32_t n_sub,
                               double* min_clear, double* lower_bound, int32_t* arg_interval, int32_t* arg_obst,
                               int32_t* first_collision, double* interval_min, int32_t device, void* hip_stream) {
    SweepArgs G;
    if (device < 0 || n_sub < 1 || n_sub > (1 << 16) || !min_clear || !lower_bound || !arg_interval || !arg_obst ||
        !first_collision || audit::plan_batch_init(&G.P, ego, n_obs, m, N, B, variant, x, A, b, N) != OBCA_OK)
        return OBCA_E_INVAL;
    G.n_sub = n_sub;
    G.min_clear = min_clear; G.lower_bound = lower_bound; G.arg_interval = arg_interval; G.arg_obst = arg_obst;
    G.first_collision = first_collision; G.interval_min = interval_min;
    return launch_segments(plan_sweep_kernel, G, B, G.P.seg, device, hip_stream);
}

extern "C" int obca_plan_tighten(const double ego[4], int32_t n_obs, const int32_t* m, int32_t N, int32_t B,
                                 const int32_t* variant, const int32_t* status, const double* x, const double* A,
                                 const double* b, int32_t n_sub, int32_t certified, double target, double gain,
                                 double grow_max, double* grow, double* b_out, int32_t* variant_out, double* min_clear,
                                 int32_t device, void* hip_stream) {
    TightenArgs G;
    if (device < 0 || n_sub < 1 || n_sub > (1 << 16) || !variant || !status || !grow || !b_out || !variant_out || b_out == b ||
        (certified != 0 && certified != 1) || !isfinite(target) || !(gain > 0.0 && gain <= 8.0) ||
        !(grow_max >= 0.0 && grow_max <= 2.0) || audit::plan_batch_init(&G.P, ego, n_obs, m, N, B, variant, x, A, b, N) != OBCA_OK)
        return OBCA_E_INVAL;
    G.n_sub = n_sub; G.certified = certified;
    G.target = target; G.gain = gain; G.grow_max = grow_max;
    G.status = status;
    G.grow = grow; G.b_out = b_out; G.variant_out = variant_out; G.min_clear = min_clear;
    return launch_segments(plan_tighten_kernel, G, B, G.P.seg, device, hip_stream);
}

extern "C" int obca_rollouts_audit(obca_rollouts* r, int32_t n_sub, double* min_clear, double* lower_bound,
                                   int32_t* arg_step, int32_t* arg_obst, int32_t* first_collision,
                                   int32_t* first_violation, double* step_min, void* hip_stream) {
    if (!r || n_sub < 1 || n_sub > (1 << 16) || !min_clear || !lower_bound || !arg_step || !arg_obst || !first_collision ||
        !first_violation)
        return OBCA_E_INVAL;
    AuditArgs G;
    obca_rollout_dims dims;
    obca_params prm;
    const int rc = obca_internal_rollouts_view(r, &G.D, &dims, &prm);       // host-side copy; no HIP call
    if (rc != OBCA_OK) return rc;
    if (!audit::ego_ok(prm.ego) || !(prm.dmin == prm.dmin)) return OBCA_E_INVAL;
    G.n_static = dims.n_static;
    for (int i = 0; i < OBCA_MAX_OBST; ++i) G.m[i] = i < dims.n_static ? dims.m_static[i] : 0;
    for (int j = 0; j < 4; ++j) G.ego[j] = prm.ego[j];
    G.dmin = prm.dmin;
    G.n_sub = n_sub;
    audit::segment_of(G.D.S, &G.seg, &G.log_seg);
    G.min_clear = min_clear; G.lower_bound = lower_bound; G.arg_step = arg_step; G.arg_obst = arg_obst;
    G.first_collision = first_collision; G.first_violation = first_violation; G.step_min = step_min;
    return launch_segments(rollouts_audit_kernel, G, G.D.B, G.seg, dims.device, hip_stream);
}
