"""Obstacles on timed tracks (scene.TrackLoop, obca_pool_tracks) measured: what the call costs per loop step beside the calls it
sits between, and what the staged select costs beside the plain one.

    python tools/track_loop_study.py [--rollouts 4096] [--steps 16] [--repeats 5] [--out profiles/FILE.json]

The corridor and the loop parameters are tools/fleet_study.py's (N = 5, Ts = 1.5 s, n_sel = 3, margin 0.1, n_sub = 8).  Every
rollout drives 10 route points along +x at y = 3.5 and has a track block of its own (group = 1): track 0 is a car-sized
obstacle that drives along +x at y = 6.5 at 0.4 m/s and then turns across the lane at -pi/4 (17 knots, one per 1.5 s), the
other Kt - 1 tracks are the same manoeuvre 40 m and more ahead.  For Kt in (1, 4, 16), three loops over the same pools,
ALTERNATING, --repeats runs each after one untimed round:
  track      TrackLoop(predict="track"): x_prev copy | staged select | solve | advance | obca_pool_tracks
  velocity   TrackLoop(predict="velocity"): the same calls with the plain select
  plain      PoolLoop over the pool TrackLoop holds after its reset (the tracked slots standing): select | solve | advance
One loop step is split by HIP events recorded between the calls; reported are the median over the repeats of the per-run
medians over the steps (the first step of a run left out), and min .. max of the per-run medians."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import fleet_study as fs  # noqa: E402

L = 17


def cut_in_track(x_first, rng):
    """[L,3]: 0.6 m per knot along +x at y = 6.5, from knot 4 on at -pi/4"""
    pts, th = [(x_first + rng.uniform(-0.2, 0.2), 6.5, 0.0)], 0.0
    for i in range(1, L):
        th = 0.0 if i < 4 else -np.pi / 4
        pts.append((pts[-1][0] + fs.SPACING * np.cos(th), pts[-1][1] + fs.SPACING * np.sin(th), th))
    return np.array(pts)


def world(B, Kt):
    rng = np.random.default_rng(Kt)
    w = fs.pack([[fs.route(2.0 + rng.uniform(-0.5, 0.5), 3.5, 0.0)] for _ in range(B)])
    tracks = np.stack([np.stack([cut_in_track(3.0 + 40.0 * j, rng) for j in range(Kt)]) for _ in range(B)])
    track_t = np.tile(fs.TS * np.arange(L), (B, Kt, 1))
    return w, tracks, track_t, np.full((B, Kt), L, np.int32)


def split(lp, steps, tracked):
    """the loop's step issued here call by call with an event after each: per-run medians in ms"""
    import torch
    lp.reset()
    torch.cuda.synchronize()
    evs, t0 = [], time.perf_counter()
    for k in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        if tracked:
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
        if tracked:
            lp._pool_tracks(1, k)
        ev[4].record()
        evs.append(ev)
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0) / steps
    t = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(4)] for e in evs])
    med = np.median(t[1:], axis=0)
    out = {"select_ms": float(med[0]), "solve_ms": float(med[1]), "advance_ms": float(med[2]), "sum_ms": float(med[:3].sum()),
           "wall_ms_per_step": wall}
    if tracked:
        out.update(pool_tracks_ms=float(med[3]), sum_ms=float(med.sum()))
    return out


def spread(rows, key):
    v = [r[key] for r in rows]
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def timing(B, Kt, a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    w, tracks, track_t, track_len = world(B, Kt)
    solver = BatchSolver(fs.N, [4] * fs.N_SEL, B)
    args = (w["pool_A"], w["pool_b"], w["start"], w["goal"], w["path"], w["path_len"], fs.TS)
    kw = dict(n_sub=fs.N_SUB, max_steps=a.steps, goal_tol2=fs.GOAL_TOL2)
    lt = scene.TrackLoop(solver, *args, tracks, track_t, track_len, predict="track", margin=fs.MARGIN, track_n_sub=fs.N_SUB, **kw)
    lv = scene.TrackLoop(solver, *args, tracks, track_t, track_len, predict="velocity", margin=fs.MARGIN, track_n_sub=fs.N_SUB, **kw)
    torch.cuda.synchronize()
    lpl = scene.PoolLoop(solver, lt.pool_A.clone(), lt.pool_b.clone(), w["start"], w["goal"], w["path"], w["path_len"], fs.TS,
                         pool_v=torch.zeros_like(lt.pool_v), variant=8, **kw)
    loops = (("track", lt, True), ("velocity", lv, True), ("plain", lpl, False))
    for _, lp, tracked in loops:                                   # one untimed round
        split(lp, a.steps, tracked)
    rows = {name: [] for name, _, _ in loops}
    for _ in range(a.repeats):                                     # alternating
        for name, lp, tracked in loops:
            rows[name].append(split(lp, a.steps, tracked))
    out = {"Kt": Kt, "B": B, "K": 2 + Kt, "L": L}
    for name, _, tracked in loops:
        keys = ("select_ms", "solve_ms", "advance_ms") + (("pool_tracks_ms",) if tracked else ()) + ("sum_ms", "wall_ms_per_step")
        out[name] = {k: spread(rows[name], k) for k in keys}
    for name, lp in (("track", lt), ("velocity", lv)):
        r = lp.run().read()
        out[name].update(flags=fs.flag_counts(r["flags"].cpu().numpy()), track_min_clear=float(r["track_min_clear"].min().item()))
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
    doc = {"how": "see the tool's docstring; ms: HIP events", "device": torch.cuda.get_device_name(0), "N": fs.N, "n_sel": fs.N_SEL,
           "Ts": fs.TS, "n_sub": fs.N_SUB, "margin": fs.MARGIN, "steps": a.steps, "repeats": a.repeats, "timing": []}
    for Kt in (1, 4, 16):
        doc["timing"].append(timing(a.rollouts, Kt, a))
        print(json.dumps(doc["timing"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
