"""The batched two-stage open-loop planner (openloop.TwoStagePlanner) measured: what each stage reaches, how the refined
plans do between their knots, and what the device path costs against the host-driven one.

    python tools/two_stage_study.py [--worlds 4096] [--host-sample 64] [--n-free 10] [--ratio 2] [--out profiles/FILE.json]
    python tools/two_stage_study.py --host-only ...      # the host-driven timing alone (runs on a tree without openloop.py)

Workloads: the checked-in demos, one instance each, and one seeded batch of scenarios.make_world_c5 worlds with two moving
boxes.  For each: feasible counts after either stage, how many instances obca_mpc6 / obca_mpc8 answered, iterations,
audit.plan_sweep / plan_clearance / plan_summary of the feasible stage-1 plans against the static rows and of the feasible
stage-2 plans against the rows they were solved with (clear at every knot, colliding between two, the worst cut), and time:
HIP events around ``plan`` on device-resident inputs, median of --repeats after one untimed run, against the host-driven
path -- closedLoop.mpc_openLoop_freeTime + mpc_openLoop_fixTime through the drop-in obca() class, one instance per call,
wall clock around the two calls, same repeats; for the batch a sample of --host-sample worlds, scaled to the batch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEMOS = "demo1,demo2,demo3,demo4,demo5,demo6,demo7,demo8,demo9,demo10,demo11"


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


def host_driven(make_settings, n_free, ratio, repeats):
    """the host mirror on fresh settings per run: (median ms of a run over all settings, feasible after stage 1 / 2 of the
    last run)"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.closed_loop import closedLoop
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.obca import obca
    solver = obca()
    ms, feas = [], None
    for _ in range(repeats + 1):
        loops = [closedLoop(s, solver=solver) for s in make_settings()]
        f1 = f2 = 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        for cl in loops:
            cl.N_free, cl.N_fix = n_free, ratio * n_free
            cl.mpc_openLoop_freeTime()
            if not cl.feas:
                continue                         # no plan to refine: the driver stops here, as the device path masks it
            f1 += 1
            cl.mpc_openLoop_fixTime()
            f2 += bool(cl.feas)
        ms.append((time.perf_counter() - t) * 1e3)
        feas = (f1, f2)
    return float(np.median(ms[1:])), feas


def swept(x, A, b, m, variant, keep, n_sub, ego):
    """plan_summary of the plans ``keep`` selects (None when it selects none)"""
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import plan_clearance, plan_summary, plan_sweep
    if not bool(keep.any()):
        return None
    x, A, b = x[keep].contiguous(), A[keep].contiguous(), b[keep].contiguous()
    var = None if variant is None else variant[keep].contiguous()
    return plan_summary(plan_sweep(x, A, b, m, n_sub=n_sub, ego=ego, variant=var), plan_clearance(x, A, b, m, ego=ego, variant=var))


def device_study(name, settings, a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import openloop
    args = openloop.from_settings(settings)
    B = len(settings)
    pl = openloop.TwoStagePlanner(a.n_free, a.ratio, args.m_static, args.n_box, max_batch=B)
    kw = {k: (v if k == "params" else torch.as_tensor(v, dtype=torch.float64, device=pl.device).contiguous())
          for k, v in args.kwargs().items()}
    p, ms = timed(lambda: pl.plan(**kw), a.repeats)
    torch.cuda.synchronize()
    Nf, Ms = a.n_free, sum(args.m_static)
    ego = args.params.ego
    A1 = kw["static_A"][:, None].expand(B, Nf + 1, Ms, 2)
    b1 = kw["static_b"][:, None].expand(B, Nf + 1, Ms)
    var4 = torch.full((B,), 4, dtype=torch.int32, device=pl.device)
    vf = p.variant_fix.cpu().numpy()
    res = {"workload": name, "plans": B, "N_free": a.n_free, "N_fix": a.ratio * a.n_free, "m_static": args.m_static, "n_box": args.n_box,
           "feasible_stage1": int(p.free.feas.sum().item()), "feasible_stage2": int(p.feas.sum().item()),
           "stage2_skipped": int((vf == 0).sum()), "answered_by_obca_mpc6": int((vf == 6).sum()),
           "answered_by_obca_mpc8": int((vf == 8).sum()),
           "feasible_by_obca_mpc6": int(((p.variant_fix == 6) & p.feas).sum().item()),
           "feasible_by_obca_mpc8": int(((p.variant_fix == 8) & p.feas).sum().item()),
           "iters_stage1": int(p.free.iters.sum().item()), "iters_stage2": int(p.fix.iters.sum().item()),
           "stage1_plans_against_static_rows": swept(p.free.xopt, A1, b1, args.m_static, var4, p.free.feas, a.n_sub, ego),
           "stage2_plans_against_A_fix": swept(p.fix.xopt, p.A_fix, p.b_fix, args.m_static + [4] * args.n_box, None, p.feas, a.n_sub, ego),
           "device_plan_ms": ms}
    pl.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--n-free", type=int, default=10)
    ap.add_argument("--ratio", type=int, default=2)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--demos", default=DEMOS)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.demo_setting import problemSetting
    work = [("%s open loop" % d, (lambda d=d: [problemSetting(d)]), 1, 1) for d in a.demos.split(",") if d]
    if a.worlds:
        n = min(a.host_sample, a.worlds)
        work.append(("C5 worlds, two moving boxes", None, a.worlds, n))
    out = []
    for name, make, B, n_host in work:
        res = {"workload": name, "plans": B}
        if make is None:
            worlds = [sc.make_world_c5(i, n_dyn=2) for i in range(B)]
            make_host = lambda n=n_host: [sc.make_world_c5(i, n_dyn=2) for i in range(n)]
        else:
            worlds, make_host = make(), make
        if not a.host_only:
            res = device_study(name, worlds, a)
        if not a.no_host:
            ms, feas = host_driven(make_host, a.n_free, a.ratio, a.repeats)
            res.update({"host_driven_sample": n_host, "host_driven_sample_ms": ms, "host_driven_ms_scaled_to_batch": ms * B / n_host,
                        "host_driven_scaled": n_host != B, "host_driven_feasible_stage1_stage2": list(feas)})
            if "device_plan_ms" in res:
                res["host_over_device"] = res["host_driven_ms_scaled_to_batch"] / res["device_plan_ms"]
        print(json.dumps(res), flush=True)
        out.append(res)
    doc = {"how": "openloop.TwoStagePlanner.plan on device-resident inputs, HIP events, median of `repeats` after one untimed run; sweeps: "
                  "audit.plan_sweep (n_sub + 1 samples per interval) and plan_clearance (knots) of the FEASIBLE plans of a stage; host-driven: "
                  "closedLoop.mpc_openLoop_freeTime + mpc_openLoop_fixTime through obca(), one instance per call, wall clock, same repeats, "
                  "the batch's figure from a sample of its first worlds scaled by plans / sample",
           "n_free": a.n_free, "ratio": a.ratio, "n_sub": a.n_sub, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "workloads": out}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
