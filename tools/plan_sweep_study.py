"""Swept audit of batched plans (audit.plan_sweep / obca_plan_sweep): what the plans of the batch workloads do between
their knots, and what the audit costs.

    python tools/plan_sweep_study.py [--c2 8192] [--c3 2048] [--n-sub 16] [--out profiles/r10_plan_sweep.json]

Workloads: the C2 headline batch; both C3 halves (gated: obca_mpc6 against five obstacles with rows per stage, free:
obca_mpc4 against the three static ones); demo9's open-loop free-time plans at N = 10 ... 74; and a C3-gated batch whose
moving-box rows come from solver.moving_rows, solved once with the boxes' own rows and once with the swept, inflated rows
(half_window = margin = 0.5), both audited against the boxes' own rows.  For each: audit.plan_summary of the feasible
plans at n_sub and at the knots (so: how many plans are clear at every knot and collide between two), and the median
kernel time of the sweep over HIP events."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed_sweep(x, A, b, m, n_sub, ego, variant, repeats):
    """the sweep's outputs and its kernel time: HIP events around audit.plan_sweep on device-resident inputs, after one
    untimed launch"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import plan_sweep
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device="cuda").contiguous()
    x, A, b, variant = t(x), t(A), t(b), t(variant, torch.int32)
    plan_sweep(x, A, b, m, n_sub=n_sub, ego=ego, variant=variant, per_interval=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sw = plan_sweep(x, A, b, m, n_sub=n_sub, ego=ego, variant=variant, per_interval=True)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sw, {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "repeats": repeats}


def study(name, x, A, b, m, variant, feas, n_sub, ego, repeats):
    """x [B,3,N+1] (device or host), the rows the plans are measured against, feas [B] bool: the summary of the feasible
    plans"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import plan_clearance, plan_summary
    feas = np.asarray(feas.cpu() if hasattr(feas, "cpu") else feas, bool)
    sel = torch.as_tensor(np.flatnonzero(feas), device="cuda")
    pick = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device="cuda")[sel].contiguous()
    xs, As, bs, vs = pick(x), pick(A), pick(b), pick(variant, torch.int32)
    sw, ms = timed_sweep(xs, As, bs, m, n_sub, ego, vs, repeats)
    kn = plan_clearance(xs, As, bs, m, ego=ego, variant=vs)
    torch.cuda.synchronize()
    res = {"workload": name, "plans": int(len(feas)), "feasible": int(feas.sum()), "N": int(xs.shape[2]) - 1, "n_sub": n_sub,
           "summary": plan_summary(sw, kn), "sweep_ms": ms}
    print(json.dumps(res), flush=True)
    return res


def c3_gated_with_boxes(B, N, procs):
    """the gated C3 instances in seed order, with their moving boxes as obca_moving_rows_batch's tuples"""
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    ins, i = [], 0
    while len(ins) < B:
        parts = sc._spawn_chunks("c3", [(i + j * 64, 64) for j in range(procs)], (N,))
        i += procs * 64
        for part in parts:
            ins += [q for _, q in part if q["gated"]]
    ins = ins[:B]
    Ms = sum(ins[0]["m"][:3])
    boxes = np.zeros((B, 2, 13))
    for r, q in enumerate(ins):
        for j, d in enumerate(q["dyn"]):
            boxes[r, j, :6] = d["cx"], d["cy"], d["th"], 3.0, 3.0, d["v"]
            boxes[r, j, 11], boxes[r, j, 12] = math.cos(d["th"]), math.sin(d["th"])
    st = lambda k: np.stack([q[k] for q in ins])
    return dict(m=ins[0]["m"], x0=st("x0"), u0=st("u0"), xref=st("xref"), term=st("term"), Ts=np.array([q["Ts_fix"] for q in ins]),
                static_A=np.stack([q["A"][0, :Ms] for q in ins]), static_b=np.stack([q["b"][0, :Ms] for q in ins]), boxes=boxes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2", type=int, default=8192)
    ap.add_argument("--c3", type=int, default=2048)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--demo9", default="10,20,30,40,50,66,74")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams, moving_rows, pack_reference_call
    ego, out = sc.EGO, []

    def solve(bt, N, A=None, b=None):
        s = BatchSolver(N, bt["m"], max_batch=len(bt["x0"]))
        r = s.solve(bt["variant"], bt["x0"], bt["u0"], bt["xref"], bt["A"] if A is None else A, bt["b"] if b is None else b, bt["Ts"],
                    bt["term"], SolverParams())
        torch.cuda.synchronize()
        s.close()
        return r

    bt = sc.make_batch(a.c2, 5, procs=a.procs)
    r = solve(bt, 5)
    out.append(study("C2 headline: obca_mpc4, N = 5, 3 obstacles", r.xopt, bt["A"], bt["b"], bt["m"], bt["variant"], r.feas, a.n_sub, ego, a.repeats))
    for gated in (True, False):
        bt = sc.make_batch_c3(a.c3, 20, gated=gated, procs=a.procs)
        r = solve(bt, 20)
        out.append(study("C3 %s half: obca_mpc%d, N = 20, %d obstacles" % ("gated" if gated else "free", 6 if gated else 4, len(bt["m"])),
                         r.xopt, bt["A"], bt["b"], bt["m"], bt["variant"], r.feas, a.n_sub, ego, a.repeats))

    g = c3_gated_with_boxes(a.c3, 20, a.procs)
    g["variant"] = np.full(a.c3, 6, np.int32)
    A0, b0 = moving_rows(g["static_A"], g["static_b"], g["boxes"], g["Ts"], 20)                 # the boxes' own rows
    A1, b1 = moving_rows(g["static_A"], g["static_b"], g["boxes"], g["Ts"], 20, half_window=0.5, margin=0.5)
    for name, A, b in (("plain rows", A0, b0), ("swept rows (half_window 0.5, margin 0.5)", A1, b1)):
        r = solve(g, 20, A, b)
        out.append(study("C3 gated, rows from moving_rows, solved with %s, audited against the boxes' own rows" % name, r.xopt, A0, b0,
                         g["m"], g["variant"], r.feas, a.n_sub, ego, a.repeats))

    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.closed_loop import closedLoop
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.demo_setting import problemSetting
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.obca import obca
    for N in [int(v) for v in a.demo9.split(",") if v]:
        cl = closedLoop(problemSetting("demo9"), solver=obca())
        cl.N_free = N
        cl.mpc_openLoop_freeTime()
        m, _, _, _, A, b, _, _ = pack_reference_call(4, cl.Ts, N, cl.x0, np.zeros((3, N + 1)), cl.nObs, cl.vObs, cl.AObs, cl.bObs, cl.u0)
        x = np.asarray(cl.xOpt, float)[None]
        if not (bool(cl.feas) and np.isfinite(x).all()):
            out.append({"workload": "demo9 open loop, obca_mpc4, N = %d" % N, "plans": 1, "feasible": 0})
            print(json.dumps(out[-1]), flush=True)
            continue
        out.append(study("demo9 open loop, obca_mpc4, N = %d" % N, x, np.asarray(A)[None], np.asarray(b)[None], m, np.array([4], np.int32),
                         np.array([True]), a.n_sub, ego, a.repeats))

    res = {"how": "audit.plan_summary of the feasible plans at n_sub samples per interval, `collisions_between_clear_knots` against "
                  "audit.plan_clearance of the same plans; sweep_ms: HIP events around audit.plan_sweep(per_interval=True) on "
                  "device-resident inputs, after one untimed launch",
           "device": torch.cuda.get_device_name(0), "workloads": out}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
