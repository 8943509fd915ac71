"""C5 (4096 closed-loop rollouts, make_world_c5(i, n_dyn=2), N = 5) with the collision stop at n_sub = 16 and exact sensing,
over the opt-in swept, inflated rows: half_window in {0, 0.5} x margin in {0, 0.25, 0.5, 0.75}; (0, 0) is DESIGN 5b's row
"stop + exact sensing".  Per run: the end reasons, the closed-loop steps, the launch time from HIP events (median of
--repeats launches after an untimed one), the audit of the run (collisions, knot violations), and how many first
collisions are against a moving box that was NOT sensed at that step -- swept rows change the rows of sensed boxes only, so
they cannot touch those -- against a sensed one, or against a static obstacle.

    python tools/c5_swept_rows.py [--rollouts 4096] [--n-sub 16] [--out profiles/r09_c5_swept_rows.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def first_collision_obstacles(dr, o, au, n_static):
    """of the rollouts with a collision: the obstacle of the colliding interval's smallest sample.  The stop ends a rollout
    at its first collision, so that interval is the only one below zero and the audit's arg_step / arg_obst name it."""
    fc = au["first_collision"]
    res = {"static": 0, "sensed_box": 0, "unsensed_box": 0, "not_the_run_minimum": 0}
    for b in np.nonzero(fc >= 0)[0]:
        s, ob = int(fc[b]), int(au["arg_obst"][b])
        if int(au["arg_step"][b]) != s:
            res["not_the_run_minimum"] += 1
        elif ob < n_static:
            res["static"] += 1
        elif o["dyn"][b, s, ob - n_static, 3] == 1.0:
            res["sensed_box"] += 1
        else:
            res["unsensed_box"] += 1
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_c5_swept_rows.json"))
    a = ap.parse_args()
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import summary
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.rollouts import FLAG_NAMES, DeviceRollouts, pack_worlds
    B = a.rollouts
    w = pack_worlds([sc.make_world_c5(i, n_dyn=2) for i in range(B)])
    res = {"workload": "C5: %d rollouts, make_world_c5(i, n_dyn=2), N = 5, max_steps 30; collision stop n_sub %d, exact sensing" % (B, a.n_sub),
           "n_sub": a.n_sub, "runs": []}
    for h in (0.0, 0.5):
        for r in (0.0, 0.25, 0.5, 0.75):
            dr = DeviceRollouts(w, N=5, collision_stop=a.n_sub, exact_sensing=True, swept_rows={"half_window": h, "margin": r})
            dr.run()                                                         # code object load, not timed
            ms = []
            for _ in range(a.repeats):
                dr.reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dr.run()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            o = {k: v.cpu().numpy() for k, v in dr.read().items()}
            au = {k: v.cpu().numpy() for k, v in dr.audit(n_sub=a.n_sub, per_step=True).items()}
            sm = summary(au, sc.DMIN)
            run = {"half_window": h, "margin": r,
                   "flags": {FLAG_NAMES[v]: int((o["flags"] == v).sum()) for v in sorted(FLAG_NAMES)},
                   "closed_loop_steps": int(o["steps"].sum()),
                   "fixed_time_steps": int((o["variant"] >= 6).sum()),
                   "run_ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "repeats": a.repeats},
                   "audit_collisions": sm["collisions"], "audit_knot_violations": sm["knot_violations"],
                   "worst_min_clear": sm["worst_min_clear"],
                   "first_collision_against": first_collision_obstacles(dr, o, au, len(w.m_static))}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            del dr
            torch.cuda.synchronize()
    res["how"] = "HIP events around DeviceRollouts.run() (one fused launch), after one untimed run; audit.summary at n_sub; " \
                 "first_collision_against: obstacle of the smallest sample of the first colliding interval, a moving box counted " \
                 "as sensed when dyn_hist marks it sensed at that step"
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps({k: res[k] for k in ("workload", "how", "device")}), flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
