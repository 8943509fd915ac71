"""The fleet closed loop (scene.FleetLoop, obca_fleet_step) measured: what the fleet step costs per loop step beside select,
solve and advance, and what the cars of a world do to each other under the two ``see`` and the two ``predict`` modes.

    python tools/fleet_study.py [--rollouts 4096] [--steps 16] [--repeats 5] [--out profiles/FILE.json]

Corridor: two walls of 4 rows (y <= -3 and y >= 13 over x in [-5, 45]); straight routes of 10 points 0.6 m apart driven at
Ts = 1.5 s, N = 5, n_sel = 3, margin 0.1, intervals measured at n_sub = 8, never stopped, goal within 1 m.
  timing     G V = --rollouts, V in (2, 4, 8): the cars of a world in head-on pairs, pair p on the line y = 5 p / ... (lanes
             2.5 m apart, starts 16.5 m apart).  One loop step split into select / solve / advance / fleet by HIP events on
             the stream (FleetLoop's own calls, issued by this tool between events): medians over the steps after one untimed
             step.  Then whole runs of --steps steps, FleetLoop against a plain PoolLoop over the same routes with the V agent
             slots left as spares (the loop as it was before obca_fleet_step existed: no code of it changed), ALTERNATING,
             --repeats each after one untimed pair: median and min .. max of the run time.
  behaviour  families of worlds of two cars, every (see, predict) combination on each: how many cars end at their goals,
             how many solves fail, and the smallest agent_clear.  head-on: the cars towards each other, starts 9 .. 18 m apart
             in steps of 0.5 m, lateral offset 0, 0.5, 1, 2 m (from 12.8 m down the routes make the cars swap places).
             crossing: car 1 crosses car 0's line at a right angle 3 .. 6.5 m ahead of car 0's start, starting 3 .. 5.5 m
             below the line.
Host time is in none of the event figures except as gaps on the stream; the wall clock per step is reported beside them."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, TS, N_SEL, N_SUB, MARGIN, POINTS, SPACING, GOAL_TOL2 = 5, 1.5, 3, 8, 0.1, 10, 0.6, 1.0
FLAG_NAMES = ("run", "goal", "cap", "failed", "collision")


def walls():
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.model_obstacle import obstacleModel
    polys = [[[45, 13], [-5, 13], [-5, 14], [45, 14], [45, 13]], [[-5, -3], [45, -3], [45, -4], [-5, -4], [-5, -3]]]
    A, b = obstacleModel().obstacle_H_Represent(2, [5, 5], polys)
    return A.reshape(2, 4, 2), b[:, 0].reshape(2, 4)


def route(x, y, heading):
    i = np.arange(POINTS)
    p = np.zeros((3, POINTS))
    p[0], p[1], p[2] = x + SPACING * i * np.cos(heading), y + SPACING * i * np.sin(heading), heading
    return p


def pack(worlds):
    """worlds: a list of lists of routes [3,POINTS] (one list per world, all of one length V)"""
    A, b = walls()
    paths = np.stack([r for w in worlds for r in w])
    B = len(paths)
    return dict(pool_A=np.tile(A, (B, 1, 1, 1)), pool_b=np.tile(b, (B, 1, 1)), start=paths[:, :, 0].copy(), goal=paths[:, :2, -1].copy(),
                path=paths, path_len=np.full(B, POINTS, np.int32))


def timing_worlds(G, V):
    rng = np.random.default_rng(V)
    out = []
    for _ in range(G):
        dx = rng.uniform(-0.5, 0.5)
        out.append([route(3.0 + dx, 2.5 * (a // 2), 0.0) if a % 2 == 0 else route(19.5 + dx, 2.5 * (a // 2), np.pi) for a in range(V)])
    return out


def fleet_loop(solver, w, V, steps, **kw):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    return scene.FleetLoop(solver, V, w["pool_A"], w["pool_b"], w["start"], w["goal"], w["path"], w["path_len"], TS, margin=MARGIN,
                           agent_n_sub=N_SUB, n_sub=N_SUB, max_steps=steps, goal_tol2=GOAL_TOL2, **kw)


def plain_loop(solver, w, V, steps):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    B = len(w["start"])
    sA = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]])
    sb = np.array([-100.0, -100.0, 101.0, 101.0])
    pool_A = np.concatenate([w["pool_A"], np.tile(sA, (B, V, 1, 1))], axis=1)
    pool_b = np.concatenate([w["pool_b"], np.tile(sb, (B, V, 1))], axis=1)
    return scene.PoolLoop(solver, pool_A, pool_b, w["start"], w["goal"], w["path"], w["path_len"], TS, pool_v=np.zeros((B, 2 + V, 2)),
                          variant=8, n_sub=N_SUB, max_steps=steps, goal_tol2=GOAL_TOL2)


def step_split(lp, steps):
    """FleetLoop's step issued here call by call with an event after each: medians of select / solve / advance / fleet ms"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    lp.reset()
    torch.cuda.synchronize()
    evs, t0 = [], time.perf_counter()
    for k in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        lp.x_prev.copy_(lp.x0)
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
        lp._fleet_step(1, k)
        ev[4].record()
        evs.append(ev)
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0) / steps
    t = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(4)] for e in evs])
    med = np.median(t[1:], axis=0)
    return {"select_ms": float(med[0]), "solve_ms": float(med[1]), "advance_ms": float(med[2]), "fleet_ms": float(med[3]),
            "fleet_ms_min_max": [float(t[1:, 3].min()), float(t[1:, 3].max())], "sum_ms": float(med.sum()), "wall_ms_per_step": wall}


def run_ms(lp):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lp.reset()
    e0.record()
    lp.run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def flag_counts(flags):
    c = np.bincount(np.asarray(flags), minlength=5)
    return {FLAG_NAMES[i]: int(c[i]) for i in range(5)}


def timing(B, V, a):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    w = pack(timing_worlds(B // V, V))
    solver = BatchSolver(N, [4] * N_SEL, B)
    fl, pl = fleet_loop(solver, w, V, a.steps), plain_loop(solver, w, V, a.steps)
    out = {"V": V, "G": B // V, "step_ms": step_split(fl, a.steps)}
    run_ms(fl), run_ms(pl)                                         # one untimed pair
    tf, tp = [], []
    for _ in range(a.repeats):                                     # alternating
        tf.append(run_ms(fl))
        tp.append(run_ms(pl))
    stat = lambda t: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))}
    rf, rp = fl.read(), pl.read()
    out["run_fleet"], out["run_plain_spares"] = stat(tf), stat(tp)
    out["run_fleet"].update(flags=flag_counts(rf["flags"].cpu().numpy()), steps=int(rf["steps"].sum().item()),
                            agent_min_clear=float(rf["agent_min_clear"].min().item()))
    out["run_plain_spares"].update(flags=flag_counts(rp["flags"].cpu().numpy()), steps=int(rp["steps"].sum().item()))
    solver.close()
    return out


def behaviour(a):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    fam = {"head_on": [[route(3.0, 5.0, 0.0), route(3.0 + d, 5.0 + dy, np.pi)] for d in np.arange(9.0, 18.25, 0.5) for dy in (0.0, 0.5, 1.0, 2.0)],
           "crossing": [[route(3.0, 5.0, 0.0), route(3.0 + dx, 5.0 - below, np.pi / 2)] for dx in np.arange(3.0, 6.75, 0.5)
                        for below in np.arange(3.0, 5.75, 0.5)]}
    out = {}
    for name, worlds in fam.items():
        w = pack(worlds)
        B = len(w["start"])
        solver = BatchSolver(N, [4] * N_SEL, B)
        out[name] = {"worlds": len(worlds), "cars": B, "modes": {}}
        for see, predict in itertools.product(("all", "lower"), ("velocity", "static")):
            r = fleet_loop(solver, w, 2, a.steps, see=see, predict=predict).run().read()
            flags, mc = r["flags"].cpu().numpy(), r["agent_min_clear"].cpu().numpy()
            both = (flags.reshape(-1, 2) == 1).all(axis=1)
            out[name]["modes"]["%s/%s" % (see, predict)] = {
                "flags": flag_counts(flags), "worlds_with_both_at_goal": int(both.sum()), "agent_min_clear": float(mc.min()),
                "worlds_with_contact": int((mc.reshape(-1, 2).min(axis=1) < 0.0).sum()),
                "agent_min_clear_of_worlds_with_both_at_goal": float(mc.reshape(-1, 2)[both].min()) if both.any() else None}
        solver.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    doc = {"how": "see the tool's docstring; ms: HIP events", "device": torch.cuda.get_device_name(0), "N": N, "n_sel": N_SEL, "Ts": TS,
           "n_sub": N_SUB, "margin": MARGIN, "steps": a.steps, "repeats": a.repeats, "timing": [], "behaviour": None}
    for V in (2, 4, 8):
        doc["timing"].append(timing(a.rollouts, V, a))
        print(json.dumps(doc["timing"][-1]), flush=True)
    doc["behaviour"] = behaviour(a)
    print(json.dumps(doc["behaviour"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
