"""The fleet's prediction by plans (scene.FleetLoop(predict="plan"), obca_fleet_tracks, obca_scene_select_staged) measured: what
the staged select and the tracks call cost per loop step beside the velocity loop, whether the re-templated kernel costs
obca_scene_select anything, and what the cars of a world do to each other under the two predictions.

    python tools/fleet_plan_study.py [--rollouts 4096] [--steps 16] [--repeats 5] [--parent-lib PATH] [--out profiles/FILE.json]

The corridor, the routes and the loop parameters are tools/fleet_study.py's (N = 5, Ts = 1.5 s, n_sel = 3, margin 0.1, n_sub = 8).
  timing     G V = --rollouts, V in (2, 4, 8), fleet_study's head-on pairs.  One loop step split by HIP events into select /
             solve / advance / fleet (/ tracks), the velocity loop and the plan loop ALTERNATING, --repeats each after one
             untimed pair: the median over the repeats of the per-run medians, and min .. max of them.  Then whole runs of
             --steps steps, alternating the same way.
  select_ab  (--parent-lib: a libobca_mpc.so built from the parent commit) obca_scene_select itself, this build against the
             parent's, on the pools of the V = 4 fleet after one step: single launches between events, ALTERNATING, 300 each
             after 20 untimed; median, and the 10th .. 90th percentile of each as the launch spread of the session.
  behaviour  families of worlds of two cars under predict velocity / plan and see lower / all: fleet_study's head-on and
             crossing families, and a cut-in family (car 0 drives `straight` points along +x at y = 6.5 from x = 3, then turns to
             -pi/4 across the lane of car 1, which drives 14 points along +x at y = 3.5 from x1; x1 = 0.5 .. 2.5 in steps of 0.25,
             straight = 3 .. 6): cars at their goals, failed cars, worlds with contact, the smallest agent_clear."""
import argparse
import ctypes
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import fleet_study as fs  # noqa: E402

PATH_MAX = 14


def pack(worlds):
    """worlds: a list of lists of (route [3,n], n <= PATH_MAX), one list per world, all of one length V"""
    A, b = fs.walls()
    cars = [c for w in worlds for c in w]
    B = len(cars)
    path, plen = np.zeros((B, 3, PATH_MAX)), np.zeros(B, np.int32)
    for q, r in enumerate(cars):
        n = r.shape[1]
        path[q, :, :n], path[q, :, n:], plen[q] = r, r[:, -1:], n
    return dict(pool_A=np.tile(A, (B, 1, 1, 1)), pool_b=np.tile(b, (B, 1, 1)), start=path[:, :, 0].copy(),
                goal=np.stack([path[q, :2, plen[q] - 1] for q in range(B)]), path=path, path_len=plen)


def cut_in_route(straight, turned=7, heading=-np.pi / 4):
    pts = [(3.0 + fs.SPACING * i, 6.5, 0.0) for i in range(straight)]
    for i in range(1, turned + 1):
        pts.append((pts[straight - 1][0] + fs.SPACING * i * np.cos(heading), 6.5 + fs.SPACING * i * np.sin(heading), heading))
    return np.array(pts).T


def lane_route(x1, points=14):
    i = np.arange(points)
    p = np.zeros((3, points))
    p[0], p[1] = x1 + fs.SPACING * i, 3.5
    return p


def step_split_plan(lp, steps):
    """FleetLoop(predict="plan")'s step issued here call by call with an event after each: medians of select / solve / advance /
    fleet / tracks ms"""
    import torch
    lp.reset()
    torch.cuda.synchronize()
    evs, t0 = [], time.perf_counter()
    for k in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        lp.x_prev.copy_(lp.x0)
        ev[0].record()
        s = lp._select()
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
        lp._tracks(k)
        ev[5].record()
        evs.append(ev)
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0) / steps
    t = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(5)] for e in evs])
    med = np.median(t[1:], axis=0)
    return {"select_ms": float(med[0]), "solve_ms": float(med[1]), "advance_ms": float(med[2]), "fleet_ms": float(med[3]),
            "tracks_ms": float(med[4]), "sum_ms": float(med.sum()), "wall_ms_per_step": wall}


def spread(rows, key):
    v = [r[key] for r in rows]
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def timing(B, V, a):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    w = fs.pack(fs.timing_worlds(B // V, V))
    solver = BatchSolver(fs.N, [4] * fs.N_SEL, B)
    fv, fp = fs.fleet_loop(solver, w, V, a.steps), fs.fleet_loop(solver, w, V, a.steps, predict="plan")
    fs.step_split(fv, a.steps), step_split_plan(fp, a.steps)       # one untimed pair
    sv, sp = [], []
    for _ in range(a.repeats):                                     # alternating
        sv.append(fs.step_split(fv, a.steps))
        sp.append(step_split_plan(fp, a.steps))
    out = {"V": V, "G": B // V,
           "velocity_step_ms": {k: spread(sv, k) for k in ("select_ms", "solve_ms", "advance_ms", "fleet_ms", "sum_ms")},
           "plan_step_ms": {k: spread(sp, k) for k in ("select_ms", "solve_ms", "advance_ms", "fleet_ms", "tracks_ms", "sum_ms")}}
    fs.run_ms(fv), fs.run_ms(fp)
    tv, tp = [], []
    for _ in range(a.repeats):
        tv.append(fs.run_ms(fv))
        tp.append(fs.run_ms(fp))
    stat = lambda t: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))}
    rv, rp = fv.read(), fp.read()
    out["run_velocity"], out["run_plan"] = stat(tv), stat(tp)
    for name, r in (("run_velocity", rv), ("run_plan", rp)):
        out[name].update(flags=fs.flag_counts(r["flags"].cpu().numpy()), steps=int(r["steps"].sum().item()),
                         agent_min_clear=float(r["agent_min_clear"].min().item()))
    solver.close()
    return out


def select_ab(parent_path, B, a, launches=300, warm=20):
    """obca_scene_select of this build and of the parent's on the same buffers, alternating single launches"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    V = 4
    w = fs.pack(fs.timing_worlds(B // V, V))
    solver = BatchSolver(fs.N, [4] * fs.N_SEL, B)
    lp = fs.fleet_loop(solver, w, V, a.steps).run(1)
    child = _lib.load()
    parent = ctypes.CDLL(parent_path)
    parent.obca_scene_select.argtypes = child.obca_scene_select.argtypes
    parent.obca_scene_select.restype = ctypes.c_int
    dev = lp.device
    K, E, N1, n_sel = lp.K, lp.E, lp.N + 1, lp.n_sel
    f = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    score, sel, A, b, vo, ok, mc = f(B, K), i(B, n_sel), f(B, N1, n_sel * E, 2), f(B, N1, n_sel * E), i(B), i(B), f(B)
    ego = (ctypes.c_double * 4)(*lp.ego)
    p = _lib.ptr
    args = (ego, B, K, E, lp.N, n_sel, 1, 0, p(lp.pool_A), p(lp.pool_b), p(lp.pool_v), p(lp.Ts), p(lp.xref), p(lp.x0), p(lp.variant_out),
            None, p(score), p(sel), p(A), p(b), p(vo), p(ok), p(mc), _lib.device_index(dev), _lib.stream_ptr(dev))
    t = {"this": [], "parent": []}
    for n in range(warm + launches):
        for name, lib in (("this", child), ("parent", parent)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert lib.obca_scene_select(*args) == 0
            e1.record()
            e1.synchronize()
            if n >= warm:
                t[name].append(e0.elapsed_time(e1))
    solver.close()
    q = lambda v: {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
    return {"B": B, "K": K, "launches_each": launches, "this_build": q(t["this"]), "parent_build": q(t["parent"])}


def behaviour(a):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    r = lambda *p: fs.route(*p)
    fam = {"head_on": [[r(3.0, 5.0, 0.0), r(3.0 + d, 5.0 + dy, np.pi)] for d in np.arange(9.0, 18.25, 0.5) for dy in (0.0, 0.5, 1.0, 2.0)],
           "crossing": [[r(3.0, 5.0, 0.0), r(3.0 + dx, 5.0 - below, np.pi / 2)] for dx in np.arange(3.0, 6.75, 0.5)
                        for below in np.arange(3.0, 5.75, 0.5)],
           "cut_in": [[cut_in_route(straight), lane_route(x1)] for x1 in np.arange(0.5, 2.75, 0.25) for straight in (3, 4, 5, 6)]}
    out = {}
    for name, worlds in fam.items():
        w = pack(worlds)
        B = len(w["start"])
        solver = BatchSolver(fs.N, [4] * fs.N_SEL, B)
        out[name] = {"worlds": len(worlds), "cars": B, "modes": {}}
        for see, predict in itertools.product(("lower", "all"), ("velocity", "plan")):
            res = fs.fleet_loop(solver, w, 2, a.steps, see=see, predict=predict).run().read()
            flags, mc = res["flags"].cpu().numpy(), res["agent_min_clear"].cpu().numpy()
            both = (flags.reshape(-1, 2) == 1).all(axis=1)
            out[name]["modes"]["%s/%s" % (see, predict)] = {
                "flags": fs.flag_counts(flags), "cars_at_goal": int((flags == 1).sum()), "worlds_with_both_at_goal": int(both.sum()),
                "worlds_with_a_failed_car": int((flags.reshape(-1, 2) == 3).any(axis=1).sum()),
                "worlds_with_contact": int((mc.reshape(-1, 2).min(axis=1) < 0.0).sum()), "agent_min_clear": float(mc.min())}
        solver.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    doc = {"how": "see the tool's docstring; ms: HIP events", "device": torch.cuda.get_device_name(0), "N": fs.N, "n_sel": fs.N_SEL,
           "Ts": fs.TS, "n_sub": fs.N_SUB, "margin": fs.MARGIN, "steps": a.steps, "repeats": a.repeats, "timing": [], "select_ab": None,
           "behaviour": None}
    for V in (2, 4, 8):
        doc["timing"].append(timing(a.rollouts, V, a))
        print(json.dumps(doc["timing"][-1]), flush=True)
    if a.parent_lib:
        doc["select_ab"] = select_ab(a.parent_lib, a.rollouts, a)
        print(json.dumps(doc["select_ab"]), flush=True)
    doc["behaviour"] = behaviour(a)
    print(json.dumps(doc["behaviour"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
