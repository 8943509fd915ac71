"""Clearance repair of batched plans (clear.solve_clear / obca_plan_tighten) on the workloads and seeds of
tools/plan_sweep_study.py: what the repair reaches, what it loses and what it costs.

    python tools/plan_repair_study.py [--c2 8192] [--c3 4096] [--rounds 4] [--gain 1.0] [--out profiles/r11_plan_repair.json]

Workloads: the C2 headline batch; both C3 halves; the C3-gated batch with rows from solver.moving_rows, solved with the
swept, inflated rows (half_window = margin = 0.5) and measured against the boxes' own rows; demo9's open-loop free-time
plans at N = 20 ... 74.  For each: feasible plans clear (smallest of n_sub + 1 samples per interval >= target, against the
ORIGINAL rows) before and after, plans a re-solve made infeasible (their round-0 plan is kept), the histogram of re-solves
per instance, the largest grow, arg_obst of what still collides split into static / moving obstacles, and the wall time of
solve_clear against one plain solve of the same instances (HIP events, median of --repeats after one untimed run)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, repeats):
    import torch
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, float(np.median(ms))


def study(name, N, m, args, A_ref, b_ref, n_static, a, ego):
    """args: BatchSolver.solve's positional arguments (A, b at 4, 5: the rows the plans are solved with and repaired on);
    A_ref / b_ref: the rows this study judges the plans against (None: the same); n_static: obstacles below this index stand
    still"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import plan_sweep
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.clear import solve_clear
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    B = len(args[1])
    s = BatchSolver(N, m, max_batch=B)
    dev = lambda t, dt=torch.float64: torch.as_tensor(t, dtype=dt, device="cuda").contiguous()
    args = [dev(args[0], torch.int32)] + [dev(t) for t in args[1:8]] + [args[8]]
    A_ref, b_ref = (args[4], args[5]) if A_ref is None else (dev(A_ref), dev(b_ref))     # the judge's rows
    kw = dict(ego=ego, rounds=a.rounds, n_sub=a.n_sub, target=a.target, gain=a.gain, grow_max=a.grow_max)
    run = lambda: solve_clear(s, *args, **kw)
    base, plain_ms = timed(lambda: s.solve(*args), a.repeats)
    feas0 = base.feas.clone()
    sw0 = plan_sweep(base.xopt, A_ref, b_ref, m, n_sub=a.n_sub, ego=ego, variant=args[0])
    mc0 = sw0["min_clear"].clone()
    (held, info), clear_ms = timed(run, a.repeats)
    sw1 = plan_sweep(held.xopt, A_ref, b_ref, m, n_sub=a.n_sub, ego=ego, variant=args[0])
    torch.cuda.synchronize()
    s.close()
    f0, f1 = feas0.cpu().numpy(), held.feas.cpu().numpy()
    c0, c1 = (mc0 >= a.target).cpu().numpy() & f0, (sw1["min_clear"] >= a.target).cpu().numpy() & f1
    ru = info["rounds_used"].cpu().numpy()
    still = f1 & ~c1
    ao = sw1["arg_obst"].cpu().numpy()[still]
    res = {"workload": name, "plans": B, "N": N, "feasible": int(f0.sum()), "clear_before": int(c0.sum()), "clear_after": int(c1.sum()),
           "held_infeasible": int((~f1).sum()) - int((~f0).sum()), "driver_clear": int(info["clear"].sum().item()),
           "clear_lost": int((c0 & ~c1).sum()), "rounds_histogram": np.bincount(ru, minlength=a.rounds + 1).tolist(),
           "rounds_histogram_of_repaired": np.bincount(ru[c1 & ~c0], minlength=a.rounds + 1).tolist(),
           "largest_grow": float(info["grow"].max().item()), "still_short": int(still.sum()),
           "still_short_against_static": int((ao < n_static).sum()), "still_short_against_moving": int((ao >= n_static).sum()),
           "worst_before": float(np.nanmin(np.where(f0, mc0.cpu().numpy(), np.nan))) if f0.any() else None,
           "worst_after": float(np.nanmin(np.where(f1, sw1["min_clear"].cpu().numpy(), np.nan))) if f1.any() else None,
           "iters_sum_plain": int(base.iters.sum().item()), "iters_sum_clear": int(held.iters.sum().item()),
           "plain_solve_ms": plain_ms, "solve_clear_ms": clear_ms, "cost_multiple": clear_ms / plain_ms}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2", type=int, default=8192)
    ap.add_argument("--c3", type=int, default=4096)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--target", type=float, default=0.0)
    ap.add_argument("--gain", type=float, default=1.0)
    ap.add_argument("--grow-max", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--demo9", default="20,30,40,50,66,74")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tools.plan_sweep_study import c3_gated_with_boxes
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import SolverParams, moving_rows, pack_reference_call
    ego, out = sc.EGO, []
    pos = lambda bt, A=None, b=None: (bt["variant"], bt["x0"], bt["u0"], bt["xref"], bt["A"] if A is None else A,
                                      bt["b"] if b is None else b, bt["Ts"], bt["term"], SolverParams())
    if a.c2:
        bt = sc.make_batch(a.c2, 5, procs=a.procs)
        out.append(study("C2 headline: obca_mpc4, N = 5, 3 obstacles", 5, bt["m"], pos(bt), None, None, 3, a, ego))
    if a.c3:
        for gated in (True, False):
            bt = sc.make_batch_c3(a.c3, 20, gated=gated, procs=a.procs)
            out.append(study("C3 %s half: obca_mpc%d, N = 20, %d obstacles" % ("gated" if gated else "free", 6 if gated else 4, len(bt["m"])),
                             20, bt["m"], pos(bt), None, None, 3, a, ego))
        g = c3_gated_with_boxes(a.c3, 20, a.procs)
        g["variant"] = np.full(a.c3, 6, np.int32)
        A1, b1 = moving_rows(g["static_A"], g["static_b"], g["boxes"], g["Ts"], 20, half_window=0.5, margin=0.5)
        A0, b0 = moving_rows(g["static_A"], g["static_b"], g["boxes"], g["Ts"], 20)             # the boxes' own rows
        out.append(study("C3 gated, solved with and repaired on moving_rows(0.5, 0.5), judged against the boxes' own rows", 20, g["m"],
                         pos(g, A1, b1), A0, b0, 3, a, ego))

    class Recorder:
        def obca_mpc4(self, *args, start_order=None):
            self.args = args
            return np.zeros((3, args[4] + 1)), np.zeros((2, args[4])), False, float(args[0])

    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.closed_loop import closedLoop
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.demo_setting import problemSetting
    for N in [int(v) for v in a.demo9.split(",") if v]:
        rec = Recorder()
        cl = closedLoop(problemSetting("demo9"), solver=rec)
        cl.N_free = N
        cl.mpc_openLoop_freeTime()
        Ts, P, Q, R, _, x0, xL, xU, uL, uU, xref, nObs, vObs, AObs, bObs, dmin, cego, u0 = rec.args
        m, x0v, u0v, xr, A, b, Tsv, term = pack_reference_call(4, Ts, N, x0, xref, nObs, vObs, AObs, bObs, u0)
        prm = SolverParams(Q_free=Q, R_free=R, P_free=P, xL=xL, xU=xU, uL=uL, uU=uU, ego=cego, dmin=dmin, start_order="x0")
        out.append(study("demo9 open loop, obca_mpc4, N = %d" % N, N, m,
                         (np.array([4], np.int32), x0v[None], u0v[None], xr[None], A[None], b[None], np.array([Tsv]), term[None], prm),
                         None, None, len(m), a, tuple(float(v) for v in cego)))

    res = {"how": "clear.solve_clear(rounds, n_sub, target, gain, grow_max) against one BatchSolver.solve of the same instances; clear = "
                  "audit.plan_sweep's min_clear >= target against the original rows; times: HIP events, median of `repeats` after one "
                  "untimed run", "rounds": a.rounds, "n_sub": a.n_sub, "target": a.target, "gain": a.gain, "grow_max": a.grow_max,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "workloads": out}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
