// obca_plan_batch.h -- the batch of plans every plan-level audit call takes (obca_plan_clearance, obca_plan_sweep,
// obca_plan_tighten of include/obca_mpc.h): x [B,3,N+1], A [B,N+1,M,2], b [B,N+1,M] with M = sum(m), variant [B] or NULL.
// One descriptor, its one validation and the only code that indexes x / A / b.  No HIP runtime call: compiles for the
// device (obca_audit.hip) and for the host (tests/native/audit_host.cpp, plan_sweep_host.cpp, plan_tighten_host.cpp), so
// kernels and host shims share the indexing as they share the geometry of obca_audit_core.h.
#ifndef OBCA_PLAN_BATCH_H
#define OBCA_PLAN_BATCH_H

#include "obca_audit_core.h"

namespace audit {

constexpr int SEG_MAX = 64;                // a segment never leaves its wavefront

struct PlanBatch {
    int32_t B, N, n_obs, M;
    int32_t m[OBCA_MAX_OBST], off[OBCA_MAX_OBST];     // rows of obstacle i and its first row within a stage; 0 beyond n_obs
    double ego[4];
    int32_t seg, log_seg;                  // lanes per instance: the next power of two >= its items, at most SEG_MAX
    const int32_t* variant;
    const double *x, *A, *b;
};

inline bool ego_ok(const double* ego) {
    if (!ego) return false;
    for (int j = 0; j < 4; ++j)
        if (!isfinite(ego[j])) return false;
    return ego[0] + ego[2] > 0.0 && ego[1] + ego[3] > 0.0;
}

inline void segment_of(int64_t items, int32_t* seg, int32_t* log_seg) {
    int s = 1, l = 0;
    while (s < items && s < SEG_MAX) { s <<= 1; ++l; }
    *seg = s; *log_seg = l;
}

// The one validation of a batch.  items = what a lane walks per instance (N + 1 stages for the knot audit, N intervals for
// sweep and tighten).  OBCA_OK with *P filled, or OBCA_E_INVAL; nothing else happens.
inline int plan_batch_init(PlanBatch* P, const double* ego, int32_t n_obs, const int32_t* m, int32_t N, int32_t B,
                           const int32_t* variant, const double* x, const double* A, const double* b, int64_t items) {
    if (!ego_ok(ego) || n_obs < 1 || n_obs > OBCA_MAX_OBST || !m || N < 1 || N > (1 << 20) || B < 1 || !x || !A || !b)
        return OBCA_E_INVAL;
    P->M = 0;
    for (int i = 0; i < OBCA_MAX_OBST; ++i) {
        P->m[i] = 0; P->off[i] = 0;
        if (i >= n_obs) continue;
        if (m[i] < 1 || m[i] > OBCA_MAX_EDGES) return OBCA_E_INVAL;
        P->m[i] = m[i];
        P->off[i] = P->M;
        P->M += m[i];
    }
    P->B = B; P->N = N; P->n_obs = n_obs;
    for (int j = 0; j < 4; ++j) P->ego[j] = ego[j];
    segment_of(items, &P->seg, &P->log_seg);
    P->variant = variant; P->x = x; P->A = A; P->b = b;
    return OBCA_OK;
}

AU_FN PlanScene plan_scene(const PlanBatch& P) {
    PlanScene sc;
    sc.ego = P.ego; sc.n_obs = P.n_obs; sc.m = P.m; sc.off = P.off;
    return sc;
}

AU_FN int plan_variant(const PlanBatch& P, int64_t inst) { return P.variant ? P.variant[inst] : 0; }

// obca_mpc4 reads stage 0's rows at every stage
AU_FN bool plan_reads_stage0(int v) { return v == 4; }

// the first stage of instance inst in a [B,N+1,...] array: its stage k is at plan_first(P, inst) + k
AU_FN size_t plan_first(const PlanBatch& P, int64_t inst) { return (size_t)inst * (P.N + 1); }

AU_FN void plan_pose(const PlanBatch& P, int64_t inst, int k, double p[3]) {
    const int N1 = P.N + 1;
    const double* xb = P.x + (size_t)inst * 3 * N1;
    p[0] = xb[k]; p[1] = xb[N1 + k]; p[2] = xb[2 * N1 + k];
}

struct PlanRows {
    const double *A0, *b0, *A1, *b1;       // the rows [M,2], [M] at the two ends of an interval; of one stage: both its own
};

// the rows a plan of variant v is held to over interval s -> s + span of the instance whose stages begin at `first`
// (plan_first; a caller computes it once per instance): span 1 an interval's two ends, span 0 stage s alone.  Variant 4's
// ends are the same pointers, which plan_obstacle_move reads as "the rows stand still".
AU_FN PlanRows plan_rows(const PlanBatch& P, size_t first, int s, int v, int span = 1) {
    const size_t k0 = first + (plan_reads_stage0(v) ? 0 : s);
    const size_t k1 = plan_reads_stage0(v) ? k0 : k0 + span;
    PlanRows R;
    R.A0 = P.A + k0 * P.M * 2; R.b0 = P.b + k0 * P.M;
    R.A1 = P.A + k1 * P.M * 2; R.b1 = P.b + k1 * P.M;
    return R;
}

}  // namespace audit
#endif
