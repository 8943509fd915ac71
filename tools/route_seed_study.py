"""Route-seeded open-loop planning measured: what stage 1 of openloop.TwoStagePlanner reaches from a route reference
(openloop.route_references: dilated map -> A* route -> N_free + 1 knots) against the start/goal-only reference, and what
building the reference costs.

    python tools/route_seed_study.py [--worlds 4096] [--horizons 10,50,74] [--demos demo1,demo8,demo9] [--out profiles/FILE.json]

Workloads: the named demos, one instance each, at every horizon, and one seeded batch of scenarios.make_world_c5 worlds with two
moving boxes at the first horizon.  Arms, same worlds and parameters:
  start_goal_x0   the start/goal-only reference with the start ladder's x0 rung first -- ``plan`` without xref_free, the
                  yardstick
  route           the plain A* route's reference (dilation 0), the caller's start order ("default": the reference window first)
  route_dilated   the route on the grid dilated by --dilation cells, the plain route where that search finds none
For each arm: feasible stage-1 plans, stage-1 iterations (sum and per instance for a demo), feasible after stage 2 (ratio 1:
N_fix = N_free, so that every horizon up to 127 fits), and audit.plan_sweep / plan_clearance / plan_summary of the feasible
stage-1 plans against the static rows.  Times: HIP events around each step of the reference on device-resident inputs --
dilation, the search on the dilated grid, the search on the plain grid, resampling -- median of --time-repeats calls after
one untimed call."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.two_stage_study import swept, timed  # noqa: E402


def reference_times(grids, sc, gc, N, start, goal, dilation, repeats):
    """median ms of each step of route_references, each timed on its own"""
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import openloop, planner
    gd, t_dil = timed(lambda: planner.dilate_batch(grids, dilation), repeats)
    _, t_search_d = timed(lambda: planner.plan_batch(gd, sc, gc), repeats)
    (path, plen), t_search = timed(lambda: planner.plan_batch(grids, sc, gc), repeats)
    _, t_res = timed(lambda: openloop.route_reference(path, plen, N, start, goal), repeats)
    _, t_all = timed(lambda: openloop.route_references(grids, sc, gc, N, start, goal, dilation=dilation), repeats)
    return {"dilate_ms": t_dil, "search_dilated_ms": t_search_d, "search_plain_ms": t_search, "resample_ms": t_res,
            "route_references_ms": t_all, "path_max": int(path.shape[2]), "longest_route": int(plen.max().item())}


def study(name, settings, n_free, a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import openloop
    args = openloop.from_settings(settings)
    B, Ms = len(settings), sum(args.m_static)
    pl = openloop.TwoStagePlanner(n_free, 1, args.m_static, args.n_box, max_batch=B)
    dev = pl.device
    kw = {k: (v if k == "params" else torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous()) for k, v in args.kwargs().items()}
    grids, sc, gc = openloop.route_arguments(settings)
    grids = torch.as_tensor(grids, device=dev)               # the cells stay host arrays: planner.plan_batch uploads them
    A1 = kw["static_A"][:, None].expand(B, n_free + 1, Ms, 2)
    b1 = kw["static_b"][:, None].expand(B, n_free + 1, Ms)
    var4 = torch.full((B,), 4, dtype=torch.int32, device=dev)
    res = {"workload": name, "plans": B, "N_free": n_free, "arms": {}}
    for arm, dil in (("start_goal_x0", None), ("route", 0), ("route_dilated", a.dilation)):
        r = {}
        xref = None
        if dil is not None:
            xref, ok, source = openloop.route_references(grids, sc, gc, n_free, kw["start"], kw["goal"], dilation=dil)
            r["source_counts"] = np.bincount(source.cpu().numpy(), minlength=3).tolist()       # fallback, plain, dilated
        p, ms = timed(lambda: pl.plan(xref_free=xref, **kw), a.repeats)
        torch.cuda.synchronize()
        it = p.free.iters.cpu().numpy()
        r.update({"feasible_stage1": int(p.free.feas.sum().item()), "iters_stage1": int(it.sum()),
                  "iters_stage1_of_feasible": int(it[p.free.feas.cpu().numpy()].sum()),
                  "status_stage1_counts": {str(int(k)): int(v) for k, v in zip(*np.unique(p.free.status.cpu().numpy(), return_counts=True))},
                  "feasible_stage2": int(p.feas.sum().item()), "plan_ms": ms,
                  "stage1_plans_against_static_rows": swept(p.free.xopt, A1, b1, args.m_static, var4, p.free.feas, a.n_sub, args.params.ego)})
        if B == 1:
            r["ts_opt_stage1"] = float(p.free.ts_opt[0].item())
        res["arms"][arm] = r
    res["reference_times"] = reference_times(grids, sc, gc, n_free, kw["start"], kw["goal"], a.dilation, a.time_repeats)
    pl.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--horizons", default="10,50,74")
    ap.add_argument("--demos", default="demo1,demo8,demo9")
    ap.add_argument("--dilation", type=int, default=1)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--time-repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.demo_setting import problemSetting
    horizons = [int(v) for v in a.horizons.split(",") if v]
    out = []
    for d in [v for v in a.demos.split(",") if v]:
        for n in horizons:
            out.append(study("%s open loop" % d, [problemSetting(d)], n, a))
            print(json.dumps(out[-1]), flush=True)
    if a.worlds:
        out.append(study("C5 worlds, two moving boxes", [sc.make_world_c5(i, n_dyn=2) for i in range(a.worlds)], horizons[0], a))
        print(json.dumps(out[-1]), flush=True)
    doc = {"how": "openloop.TwoStagePlanner.plan at ratio 1 on device-resident inputs, three references for stage 1 (see the tool's docstring); "
                  "plan_ms: HIP events, median of `repeats` after one untimed run; sweeps: audit.plan_sweep (n_sub + 1 samples per interval) and "
                  "plan_clearance (knots) of the FEASIBLE stage-1 plans against the static rows; reference_times: HIP events around each step, "
                  "median of `time_repeats` after one untimed call",
           "dilation": a.dilation, "n_sub": a.n_sub, "repeats": a.repeats, "time_repeats": a.time_repeats,
           "device": torch.cuda.get_device_name(0), "workloads": out}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
