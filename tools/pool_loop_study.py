"""The closed loop over scene pools (scene.PoolLoop, scene.drive_maps) measured: where a step's time goes, closed-loop steps
per second from maps, and the same rollouts through the closed loop that existed (rollouts.DeviceRollouts).

    python tools/pool_loop_study.py [--worlds 4096] [--small 64] [--steps 40] [--time-bound reference|path] [--out profiles/FILE.json]

Worlds: tools/grid_pool_study.py's -- 11 x 40 maps, rows 0 and 10 occupied, two boxes; start cell (5, 3), goal cell (5, 38),
start pose (3, 5, 0), goal (38, 5).  N = 5, obca_mpc4, Ts = 0.1, K = 16, n_sel = 4, dilation 1, measured intervals at
n_sub = 8, never stopped, max_steps = --steps, the free-time problem's time bound --time-bound (include/obca_mpc.h:
time_bound; "reference" is the signed sum under which a route that descends is infeasible).  Per batch size (--worlds, and --small to see the launch-bound end):
  step_ms           one step split into select / solve / advance by HIP events on the stream (the three public calls of
                    PoolLoop's step, issued by this tool between events): median over the steps after one untimed step,
                    and the share of rollouts still running at the median step
  drive_maps        scene.drive_maps end to end, HIP events, median of --repeats runs after one untimed run: ms, the steps
                    driven (sum of read()["steps"]) and steps per second; flags at the end
  device_rollouts   on the worlds whose cover has at most 8 rectangles (grid_pool with K = 8: every pool padded to eight
                    obstacles of 4 rows, so one handle shape m = [4] * 8 serves them all): DeviceRollouts in lock-step mode
                    on the same starts, goals and routes, all 8 obstacles in every solve; and PoolLoop (K = 8, n_sel = 4) on
                    the same worlds: ms per run, steps, steps per second, flags
Host time is in none of the event figures except as gaps on the stream: a step that is launch-bound shows as select + solve
+ advance well below the wall clock per step, which is reported beside them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.grid_pool_study import worlds  # noqa: E402
from tools.two_stage_study import timed  # noqa: E402

N, TS, K, N_SEL, N_SUB = 5, 0.1, 16, 4, 8
START_CELL, GOAL_CELL, START_POSE, GOAL_POSE = (5, 3), (5, 38), (3.0, 5.0, 0.0), (38.0, 5.0, 0.0)


def flag_counts(flags):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
    c = np.bincount(np.asarray(flags), minlength=5)
    return {_lib.FLAG_NAMES[i]: int(c[i]) for i in range(5)}


def inputs(B, seed):
    import torch
    grids = worlds(B, 11, 40, 2, seed)
    cells = lambda c: np.tile(np.array(c, np.int32), (B, 1))
    pose = lambda p: torch.as_tensor(np.tile(np.array(p, float), (B, 1)), device="cuda")
    return torch.as_tensor(grids, device="cuda"), cells(START_CELL), cells(GOAL_CELL), pose(START_POSE), pose(GOAL_POSE)


def step_split(lp, steps):
    """PoolLoop's step (rounds = 0) issued here call by call with an event after each: [steps, 3] ms and the wall clock"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    ms, running = [], []
    lp.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        s = scene.select(lp.pool_A, lp.pool_b, lp.xref, lp.n_sel, pool_v=lp.pool_v, Ts=lp.Ts, x0=lp.x0, variant=lp.variant_out,
                         n_sub=lp.select_n_sub, ego=lp.ego, device=lp.device)
        var = torch.where(s["ok"] != 0, lp.variant_out, 0).to(torch.int32)
        ev[1].record()
        lp._held = r = lp.solver.solve(var, lp.x0, lp.u0, lp.xref, s["A"], s["b"], lp.Ts, lp.term, lp._cparams, out=lp._held)
        ev[2].record()
        lp._last = (r, s["sel"])
        for name, t in (("status", r.status), ("iters", r.iters), ("ts_opt", r.ts_opt), ("xopt", r.xopt), ("uopt", r.uopt), ("sel", s["sel"])):
            setattr(lp._desc, name, t.data_ptr())
        lp._advance(1)
        ev[3].record()
        ms.append(ev)
        running.append(lp.flags == 0)
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0) / steps
    t = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(3)] for e in ms])
    run = np.array([float(r.double().mean().item()) for r in running])
    med = np.median(t[1:], axis=0)                                 # the first step is the untimed one
    return {"select_ms": float(med[0]), "solve_ms": float(med[1]), "advance_ms": float(med[2]), "sum_ms": float(med.sum()),
            "wall_ms_per_step": wall, "running_share_at_median_step": float(run[len(run) // 2]),
            "solve_ms_first_timed_step": float(t[1, 1]), "solve_ms_last_step": float(t[-1, 1])}


def study(B, a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.openloop import route_search
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.rollouts import DeviceRollouts, PackedWorlds
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams
    g, sc, gc, start, goal = inputs(B, a.seed)
    params = SolverParams(xL=(0.0, 0.0), xU=(39.0, 10.0), time_bound=a.time_bound)
    kw = dict(variant=4, params=params, max_steps=a.steps, n_sub=N_SUB)
    solver = BatchSolver(N, [4] * N_SEL, B)
    out = {"B": B}

    drive = lambda: scene.drive_maps(solver, g, sc, gc, start, goal, TS, K, pad=0.5, dilation=1, **kw)
    (lp, info), ms = timed(drive, a.repeats)
    rd = lp.read()
    steps = int(rd["steps"].sum().item())
    out["drive_maps"] = {"ms": ms, "steps": steps, "steps_per_s": steps / (ms * 1e-3), "flags": flag_counts(rd["flags"].cpu().numpy()),
                         "masked": int((info["path_len"] == 0).sum().item()),
                         "min_clear_of_goal_rollouts": float(rd["min_clear"][rd["flags"] == 1].min().item()) if (rd["flags"] == 1).any() else None}
    out["step_ms"] = step_split(lp, a.steps)

    # the worlds a handle fits: at most 8 rectangles
    pool8 = scene.grid_pool(g, 8, pad=0.5)
    path, plen, _ = route_search(g, sc, gc, dilation=1)
    keep = ((pool8["ok"] != 0) & (plen >= 1)).cpu().numpy()
    idx = np.flatnonzero(keep)
    n8 = len(idx)
    out["device_rollouts"] = {"worlds": n8}
    if n8:
        ti = torch.as_tensor(idx, device="cuda")
        pA, pb = pool8["pool_A"][ti].contiguous(), pool8["pool_b"][ti].contiguous()
        pw = PackedWorlds()
        pw.m_static, pw.n_dyn, pw.sense_dis, pw.xL, pw.xU = [4] * 8, 0, 10.0, (0.0, 0.0), (39.0, 10.0)
        pw.start, pw.goal = start[ti].cpu().numpy(), goal[ti, :2].cpu().numpy()
        pw.path, pw.path_len = path[ti].cpu().numpy(), plen[ti].cpu().numpy().astype(np.int32)
        pw.static_A, pw.static_b, pw.dyn = pA.reshape(n8, 32, 2).cpu().numpy(), pb.reshape(n8, 32).cpu().numpy(), np.zeros((n8, 0, 13))
        dr = DeviceRollouts(pw, N=N, params=params, Ts0=TS, max_steps=a.steps)
        dr.set_mode("lockstep")

        def run_dr():
            dr.reset()
            return dr.run()
        _, ms_dr = timed(run_dr, a.repeats)
        o = dr.read()
        st = int(o["steps"].sum().item())
        out["device_rollouts"]["lockstep_all_8"] = {"ms": ms_dr, "steps": st, "steps_per_s": st / (ms_dr * 1e-3),
                                                    "flags": flag_counts(o["flags"].cpu().numpy())}
        dr.close()
        s8 = BatchSolver(N, [4] * N_SEL, n8)
        lp8 = scene.PoolLoop(s8, pA, pb, start[ti], goal[ti], path[ti], plen[ti], TS, **kw)

        def run_lp():
            lp8.reset()
            return lp8.run()
        _, ms_lp = timed(run_lp, a.repeats)
        o = lp8.read()
        st = int(o["steps"].sum().item())
        out["device_rollouts"]["pool_loop_4_of_8"] = {"ms": ms_lp, "steps": st, "steps_per_s": st / (ms_lp * 1e-3),
                                                      "flags": flag_counts(o["flags"].cpu().numpy())}
        s8.close()
    solver.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--small", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--time-bound", choices=("reference", "path"), default="reference")
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    doc = {"how": "see the tool's docstring; ms: HIP events", "device": torch.cuda.get_device_name(0), "N": N, "K": K, "n_sel": N_SEL,
           "n_sub": N_SUB, "steps": a.steps, "time_bound": a.time_bound, "repeats": a.repeats, "seed": a.seed, "batches": []}
    for B in (a.worlds, a.small):
        if B > 0:
            doc["batches"].append(study(B, a))
            print(json.dumps(doc["batches"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
