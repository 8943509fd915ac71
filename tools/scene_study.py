"""Scene pools measured: scene.solve_scene on a few selected obstacles against the plain solve on every obstacle of the world.

    python tools/scene_study.py [--batch 8192] [--pools 8,32] [--n-sel 3,4] [--rounds 2] [--cache DIR] [--out profiles/FILE.json]

Worlds: scenarios.make_pool_batch -- the headline workload (N = 5, two walls and one box of 4 rows each) plus K - 3 unit
squares per instance, seed 11.  Arms per pool size K, same worlds and parameters:
  yardstick     K = 8 only: BatchSolver.solve on all 8 obstacles through a [4] * 8 handle (what the project could do before;
                a pool of 32 fits no handle)
  n_sel = 3, 4  scene.solve_scene(rounds) through a [4] * n_sel handle
For each arm: feasible plans, iterations, the kernel the handle's shape resolves to in auto mode (csrc/obca_select.h through the
host build tests/native/select_host.cpp) and whether a compile-time-shape instantiation runs, the smallest sampled clearance
of the feasible plans against the WHOLE pool (scene.pool_clearance, n_sub + 1 samples per interval) with the count below 0
and below dmin at the knots, plans equal to the yardstick's to 1e-6 m, and for solve_scene what the later rounds did:
instances re-solved per round, held plans replaced, clearance before and after.  Times: HIP events on device-resident inputs,
median of --repeats calls after one untimed call -- the whole arm, and the selection kernel alone in both modes.  --cache
keeps the drawn worlds (drawing 8192 of them in Python takes longer than every measurement)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.two_stage_study import timed  # noqa: E402


def worlds(B, K, N, seed, cache):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios
    path = os.path.join(cache, "scene_worlds_B%d_K%d_N%d_seed%d.npz" % (B, K, N, seed)) if cache else None
    if path and os.path.exists(path):
        with np.load(path) as f:
            return {k: f[k] for k in f.files}
    w = {k: v for k, v in scenarios.make_pool_batch(B, K - 3, N, seed).items() if k != "m"}
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez(path, **w)
    return w


def kernel_of(N, n, solver):
    """auto mode's kernel for the shape, by the selection header's own rule, and what the handle says about instantiations"""
    import ctypes
    from tests import native_build, test_select_core as sel
    lib = native_build.build_shim("select_host", [sel.SRC])
    lib.select_kernel_name.restype = ctypes.c_char_p
    p = sel.plan(lib, (N, n, 4 * n))
    return {"kernel_generic": p["kernel"], "specialised": bool(solver.specialised), "lds_bytes": int(solver.lds_bytes)}


def clearance(x, w, feas, n_sub, dmin):
    """the feasible plans against the whole pool: smallest sample, plans with a sample below 0, plans below dmin at a knot"""
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    if not feas.any():
        return None
    _, swept = scene.pool_clearance(x, w["pool_A"], w["pool_b"], variant=w["variant"], n_sub=n_sub)
    _, knots = scene.pool_clearance(x, w["pool_A"], w["pool_b"], variant=w["variant"], n_sub=1)
    swept, knots = swept.cpu().numpy()[feas], knots.cpu().numpy()[feas]
    return {"min_sampled": float(swept.min()), "plans_colliding_sampled": int((swept < 0).sum()),
            "plans_below_dmin_at_a_knot": int((knots < dmin - 1e-6).sum()), "min_at_knots": float(knots.min())}


def study(K, a):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams
    N, B = a.horizon, a.batch
    w = worlds(B, K, N, a.seed, a.cache)
    dev = torch.device("cuda", torch.cuda.current_device())
    w = {k: torch.as_tensor(v, device=dev).contiguous() for k, v in w.items()}
    params = SolverParams()
    res = {"K": K, "plans": B, "N": N, "arms": {}}
    yard = None
    if K <= 8:
        s = BatchSolver(N, [4] * K, B)
        A = w["pool_A"].reshape(B, 1, 4 * K, 2).expand(B, N + 1, 4 * K, 2).contiguous()
        b = w["pool_b"].reshape(B, 1, 4 * K).expand(B, N + 1, 4 * K).contiguous()
        yard, ms = timed(lambda: s.solve(w["variant"], w["x0"], w["u0"], w["xref"], A, b, w["Ts"], w["term"], params), a.repeats)
        feas = yard.feas.cpu().numpy()
        res["arms"]["yardstick"] = dict(kernel_of(N, K, s), feasible=int(feas.sum()), iters=int(yard.iters.sum().item()), ms=ms,
                                        clearance=clearance(yard.xopt, w, feas, a.n_sub, params.dmin))
        s.close()
    for n_sel in a.n_sel:
        s = BatchSolver(N, [4] * n_sel, B)
        run = lambda rounds: scene.solve_scene(s, w["variant"], w["x0"], w["u0"], w["xref"], w["pool_A"], w["pool_b"], w["Ts"],
                                               term=w["term"], params=params, rounds=rounds, n_sub=a.n_sub)
        (r0, i0), ms0 = timed(lambda: run(0), a.repeats)
        (r, info), ms = timed(lambda: run(a.rounds), a.repeats)
        feas0, feas = r0.feas.cpu().numpy(), r.feas.cpu().numpy()
        used = info["rounds_used"].cpu().numpy()
        mc0, mc = info["min_clear_first"].cpu().numpy(), info["min_clear"].cpu().numpy()
        arm = dict(kernel_of(N, n_sel, s), feasible=int(feas.sum()), feasible_round0=int(feas0.sum()), iters=int(r.iters.sum().item()),
                   iters_round0=int(r0.iters.sum().item()), ms=ms, ms_round0_only=ms0,
                   clearance=clearance(r.xopt, w, feas, a.n_sub, params.dmin),
                   clearance_round0=clearance(r0.xopt, w, feas0, a.n_sub, params.dmin),
                   later_rounds={"instances_resolved_n_times": np.bincount(used, minlength=a.rounds + 1).tolist(),
                                 "held_plans_replaced": int((mc > mc0).sum()),
                                 "colliding_before": int((mc0 < 0).sum()), "colliding_after": int((mc < 0).sum()),
                                 "clear": int(info["clear"].sum().item())})
        if yard is not None:
            off = (r.xopt - yard.xopt).abs().amax(dim=(1, 2)).cpu().numpy()
            both = feas & yard.feas.cpu().numpy()
            arm["plans_equal_to_yardstick_1e-6"] = int((off[both] <= 1e-6).sum())
            arm["feasible_where_yardstick_is"] = int(both.sum())
        # the selection kernel alone: mode 0 on the reference, mode 1 on the held plans
        kw = dict(variant=w["variant"], n_sub=a.n_sub)
        st, t0 = timed(lambda: scene.select(w["pool_A"], w["pool_b"], w["xref"], n_sel, x0=w["x0"], **kw), a.time_repeats)
        _, t1 = timed(lambda: scene.select(w["pool_A"], w["pool_b"], r.xopt, n_sel, status=r.status, state=st, **kw), a.time_repeats)
        arm["select_ms"] = {"mode0": t0, "mode1": t1}
        res["arms"]["n_sel_%d" % n_sel] = arm
        s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--horizon", type=int, default=5)
    ap.add_argument("--pools", default="8,32")
    ap.add_argument("--n-sel", default="3,4")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--time-repeats", type=int, default=21)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--draw-only", action="store_true", help="draw and cache the worlds, measure nothing (needs no GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.n_sel = [int(v) for v in a.n_sel.split(",") if v]
    pools = [int(v) for v in a.pools.split(",") if v]
    if a.draw_only:
        for K in pools:
            worlds(a.batch, K, a.horizon, a.seed, a.cache)
        return
    import torch
    out = []
    for K in pools:
        out.append(study(K, a))
        print(json.dumps(out[-1]), flush=True)
    doc = {"how": "scene.solve_scene against BatchSolver.solve on every obstacle, device-resident inputs (see the tool's docstring); ms: HIP "
                  "events, median of `repeats` calls after one untimed call; select_ms: obca_scene_select alone, median of `time_repeats`; "
                  "clearance: scene.pool_clearance of the feasible plans against the whole pool, n_sub + 1 samples per interval",
           "rounds": a.rounds, "n_sub": a.n_sub, "seed": a.seed, "repeats": a.repeats, "time_repeats": a.time_repeats,
           "device": torch.cuda.get_device_name(0), "pools": out}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
