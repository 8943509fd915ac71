"""Open-loop plans among timed tracks (obca_plan_tracks, scene.solve_tracks) measured: what the call costs beside
obca_scene_select_staged at the same shape, and what ``solve_tracks`` costs beside ``solve_scene`` over the same pools with the
tracked slots standing.

    python tools/track_plan_study.py [--plans 4096] [--launches 20] [--repeats 5] [--out profiles/FILE.json]

The corridor, the tracks and the parameters are tools/track_loop_study.py's (Ts = 1.5 s, n_sel = 3, margin 0.1; every plan has
a track block of its own, L = 17), n_sub = 16.  A plan is the straight line along +x at y = 3.5, 0.6 m per knot.  For Kt in
(1, 4, 16) and N in (5, 20), two calls over the same buffers, ALTERNATING, --repeats runs of --launches launches each after one
untimed round:
  plan_tracks   scene.plan_track_clearance with the select's score (obca_plan_tracks)
  staged        scene.select(..., state=state) with the tracks' stage rows (obca_scene_select_staged, accumulate = 1)
Reported are the median over the repeats of the per-run medians of HIP events around one launch, and min .. max of the per-run
medians.  Then, N = 5: ``solve_tracks`` and ``solve_scene`` (rounds = 2) as whole calls, alternating, the same way."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import fleet_study as fs  # noqa: E402
from tools import track_loop_study as tls  # noqa: E402

N_SUB = 16


_WORLDS = {}


def world(B, Kt):
    """tools/track_loop_study.py's world, built once per Kt"""
    if (B, Kt) not in _WORLDS:
        _WORLDS[(B, Kt)] = tls.world(B, Kt)
    return _WORLDS[(B, Kt)]


def plans(w, N):
    """x [B,3,N+1]: from every rollout's start along +x, fs.SPACING per knot"""
    x = np.repeat(np.asarray(w["start"], float)[:, :, None], N + 1, axis=2)
    x[:, 0] += fs.SPACING * np.arange(N + 1)[None, :]
    return x


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def timed(fn, launches):
    """the median of HIP events around each of ``launches`` calls of fn, ms"""
    import torch
    evs = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs]))


def calls(B, Kt, N, a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    w, tracks, track_t, track_len = world(B, Kt)
    dev = torch.device("cuda")
    tr = [torch.as_tensor(v, device=dev) for v in (tracks, track_t, track_len)]
    x = torch.as_tensor(plans(w, N), device=dev)
    rows = scene.track_rows(*tr, fs.TS, N, w["pool_A"], w["pool_b"], margin=fs.MARGIN)
    kw = dict(pool_v=rows["pool_v"], Ts=fs.TS, variant=8, n_sub=N_SUB, stage_A=rows["stage_A"], stage_b=rows["stage_b"],
              stage_ok=rows["stage_ok"])
    state = scene.select(rows["pool_A"], rows["pool_b"], x, fs.N_SEL, **kw)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    var = torch.full((B,), 8, dtype=torch.int32, device=dev)
    kw["variant"] = var
    fns = {"plan_tracks": lambda: scene.plan_track_clearance(x, *tr, fs.TS, variant=var, status=status, n_sub=N_SUB, score=state["score"]),
           "staged": lambda: scene.select(rows["pool_A"], rows["pool_b"], x, fs.N_SEL, status=status, state=state, **kw)}
    for fn in fns.values():
        timed(fn, a.launches)
    got = {k: [] for k in fns}
    for _ in range(a.repeats):
        for k, fn in fns.items():
            got[k].append(timed(fn, a.launches))
    out = {"Kt": Kt, "N": N, "B": B, "K": 2 + Kt, "L": tls.L, "samples_per_track": N * (N_SUB + 1)}
    out.update({k + "_ms": spread(v) for k, v in got.items()})
    out["ratio"] = out["plan_tracks_ms"]["median"] / out["staged_ms"]["median"]
    return out


def solves(B, Kt, a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    w, tracks, track_t, track_len = world(B, Kt)
    dev = torch.device("cuda")
    tr = [torch.as_tensor(v, device=dev) for v in (tracks, track_t, track_len)]
    solver = BatchSolver(fs.N, [4] * fs.N_SEL, B)
    x0, xref = torch.as_tensor(w["start"], device=dev), torch.as_tensor(plans(w, fs.N), device=dev)
    u0 = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    rows = scene.track_rows(*tr, fs.TS, fs.N, w["pool_A"], w["pool_b"], margin=fs.MARGIN)
    info = {}

    def tracks_fn():
        info["tracks"] = scene.solve_tracks(solver, 8, x0, u0, xref, w["pool_A"], w["pool_b"], fs.TS, *tr, margin=fs.MARGIN, rounds=2,
                                            n_sub=N_SUB)[1]

    def scene_fn():
        info["scene"] = scene.solve_scene(solver, 8, x0, u0, xref, rows["pool_A"], rows["pool_b"], fs.TS,
                                          pool_v=torch.zeros_like(rows["pool_v"]), rounds=2, n_sub=N_SUB)[1]
    fns = {"solve_tracks": tracks_fn, "solve_scene": scene_fn}
    for fn in fns.values():
        timed(fn, 1)
    got = {k: [] for k in fns}
    for _ in range(a.repeats):
        for k, fn in fns.items():
            got[k].append(timed(fn, 1))
    out = {"Kt": Kt, "N": fs.N, "B": B, "rounds": 2}
    out.update({k + "_ms": spread(v) for k, v in got.items()})
    for k, key in (("tracks", "solve_tracks"), ("scene", "solve_scene")):
        out[key + "_clear"] = int(info[k]["clear"].sum().item())
        out[key + "_resolved"] = int((info[k]["rounds_used"] > 0).sum().item())
    solver.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    doc = {"how": "see the tool's docstring; ms: HIP events", "device": torch.cuda.get_device_name(0), "n_sel": fs.N_SEL, "Ts": fs.TS,
           "n_sub": N_SUB, "margin": fs.MARGIN, "launches": a.launches, "repeats": a.repeats, "calls": [], "solves": []}
    for N in (5, 20):
        for Kt in (1, 4, 16):
            doc["calls"].append(calls(a.plans, Kt, N, a))
            print(json.dumps(doc["calls"][-1]), flush=True)
    for Kt in (1, 4, 16):
        doc["solves"].append(solves(a.plans, Kt, a))
        print(json.dumps(doc["solves"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
