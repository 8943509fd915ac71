"""Occupancy grids to scene pools measured: obca_grid_pool against the host core, against the rest of map -> reference, and
scene.solve_maps against the same pools built on the host and uploaded.

    python tools/grid_pool_study.py [--batches 4096,8192] [--boxes 4] [--repeats 21] [--solve-batch 4096] [--out profiles/FILE.json]

Worlds: 11 x 40 maps, rows 0 and 10 occupied, --boxes boxes of height 1..2 and width 1..3 cells with their top row in
[1, 10 - h] and left column in [7, 36 - w]; start cell (5, 3), goal cell (5, 38).  Per batch size:
  grid_pool_ms      scene.grid_pool (K = 64, pad = 0.5), HIP events on a device-resident grid, median of --repeats calls after one
                    untimed call
  host_core_ms      the same maps through the host build of csrc/obca_gridpool_core.h (tests/native/grid_pool_host.cpp), one
                    thread, wall clock, median of 5
  route_ms          planner.dilate_batch (level 1) + planner.plan_batch on the dilated maps: the other kernels of map -> reference
  count             the distribution of the cover's count on the plain and on the dilated maps (is K = 64 enough)
and once, on --solve-batch worlds with N = 10, obca_mpc4, n_sel = 4, K = 16:
  solve_maps_ms     scene.solve_maps, everything on the device
  host_pools_ms     the pools from the host core, uploaded, then openloop.route_references and scene.solve_scene: wall clock
                    around the host part plus HIP events around the device part
and one launch of 64 maps of 255 x 255 (walls and 20 boxes of up to 40 x 40 cells) for the largest grid the kernel takes in practice."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.two_stage_study import timed  # noqa: E402


def worlds(B, rows, cols, n_box, seed, max_h=2, max_w=3):
    rng = np.random.default_rng(seed)
    g = np.zeros((B, rows, cols), np.uint8)
    g[:, 0] = g[:, -1] = 1
    for i in range(B):
        for _ in range(n_box):
            h, w = int(rng.integers(1, max_h + 1)), int(rng.integers(1, max_w + 1))
            r, c = int(rng.integers(1, rows - 1 - h + 1)), int(rng.integers(7, cols - 4 - w + 1))
            g[i, r:r + h, c:c + w] = 1
    return g


def dist(count):
    c = np.asarray(count)
    return {"min": int(c.min()), "median": float(np.median(c)), "p99": float(np.percentile(c, 99)), "max": int(c.max()),
            "over_64": int((c > 64).sum())}


def host_cover(grids, K, pad=0.5):
    from tests import test_grid_pool_core as core
    return core.host_pool(core.load_host(), grids, K, pad=pad)


def wall(fn, repeats=5):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, float(np.median(ts))


def study_batch(B, a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import planner, scene
    grids = worlds(B, 11, 40, a.boxes, a.seed)
    g = torch.as_tensor(grids, device="cuda")
    cells = lambda c: np.tile(np.array(c, np.int32), (B, 1))           # plan_batch takes host arrays
    sc, gc = cells((5, 3)), cells((5, 38))
    pool, ms = timed(lambda: scene.grid_pool(g, 64), a.repeats)
    href, host_ms = wall(lambda: host_cover(grids, 64))
    same = all(np.array_equal(pool[k].cpu().numpy(), href[k]) for k in ("rect", "count", "ok", "pool_A", "pool_b"))
    (gd, _), route_ms = timed(lambda: (lambda d: (d, planner.plan_batch(d, sc, gc)))(planner.dilate_batch(g, 1)), a.repeats)
    pool_d = scene.grid_pool(gd, 64)
    return {"B": B, "grid_pool_ms": ms, "host_core_ms": host_ms, "equal_to_host_core": bool(same), "route_ms": route_ms,
            "count_plain": dist(pool["count"].cpu().numpy()), "count_dilated": dist(pool_d["count"].cpu().numpy())}


def study_solve(a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import openloop, scene
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    B, N, K, n_sel = a.solve_batch, 10, 16, 4
    grids = worlds(B, 11, 40, 2, a.seed + 1)
    g = torch.as_tensor(grids, device="cuda")
    cells = lambda c: np.tile(np.array(c, np.int32), (B, 1))           # plan_batch takes host arrays
    sc, gc = cells((5, 3)), cells((5, 38))
    pose = lambda p: torch.as_tensor(np.tile(np.array(p, float), (B, 1)), device="cuda")
    start, goal = pose((3.0, 5.0, 0.0)), pose((38.0, 5.0, 0.0))
    s = BatchSolver(N, [4] * n_sel, B)
    (res, info), ms = timed(lambda: scene.solve_maps(s, g, sc, gc, start, goal, 0.1, K), a.solve_repeats)

    def host_pools():
        t0 = time.perf_counter()
        h = host_cover(grids, K)
        pA, pb = torch.as_tensor(h["pool_A"], device="cuda"), torch.as_tensor(h["pool_b"], device="cuda")
        torch.cuda.synchronize()
        host_ms = 1e3 * (time.perf_counter() - t0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        xref, _, source = openloop.route_references(g, sc, gc, N, start=start, goal=goal, dilation=1)
        var = torch.where(source != 0, 4, 0).to(torch.int32)
        out = scene.solve_scene(s, var, start, torch.zeros(B, 2, dtype=torch.float64, device="cuda"), xref, pA, pb, 0.1)
        e1.record()
        e1.synchronize()
        return out, host_ms, e0.elapsed_time(e1)
    host_pools()
    runs = [host_pools() for _ in range(a.solve_repeats)]
    res_h = runs[-1][0][0]
    out = {"B": B, "N": N, "K": K, "n_sel": n_sel, "solve_maps_ms": ms, "feasible": int(res.feas.sum().item()),
           "masked": int((info["source"] == 0).sum().item()) + int((info["pool_ok"] == 0).sum().item()),
           "host_pools_ms": {"cover_and_upload": float(np.median([r[1] for r in runs])), "device_part": float(np.median([r[2] for r in runs]))},
           "same_plans": bool(torch.equal(res.status, res_h.status))}
    s.close()
    return out


def study_large(a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    grids = worlds(64, 255, 255, 20, a.seed + 2, max_h=40, max_w=40)
    g = torch.as_tensor(grids, device="cuda")
    pool, ms = timed(lambda: scene.grid_pool(g, 64), a.repeats)
    href, host_ms = wall(lambda: host_cover(grids, 64), 3)
    return {"B": 64, "rows": 255, "cols": 255, "grid_pool_ms": ms, "host_core_ms": host_ms, "count": dist(pool["count"].cpu().numpy()),
            "equal_to_host_core": bool(all(np.array_equal(pool[k].cpu().numpy(), href[k]) for k in ("rect", "count", "ok")))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,8192")
    ap.add_argument("--boxes", type=int, default=4)
    ap.add_argument("--seed", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--solve-batch", type=int, default=4096)
    ap.add_argument("--solve-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    doc = {"how": "see the tool's docstring; ms: HIP events, median of `repeats` calls after one untimed call; host: wall clock",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "boxes": a.boxes, "seed": a.seed, "maps_11x40": []}
    for B in (int(v) for v in a.batches.split(",") if v):
        doc["maps_11x40"].append(study_batch(B, a))
        print(json.dumps(doc["maps_11x40"][-1]), flush=True)
    doc["large"] = study_large(a)
    print(json.dumps(doc["large"]), flush=True)
    doc["solve_maps"] = study_solve(a)
    print(json.dumps(doc["solve_maps"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
