"""C5 (4096 closed-loop rollouts, make_world_c5(i, n_dyn=2), N = 5) three ways: the default, with the collision stop at
n_sub = 16, and with the stop plus exact sensing.  Per run: the end reasons, the closed-loop steps taken and the run's time
from HIP events (median of --repeats runs after an untimed one).  Cross-check: the stop run's collision count equals
audit.summary(...)["collisions"] of the default run at the same n_sub (only intervals of applied steps count).

    python tools/c5_collision_stop.py [--rollouts 4096] [--n-sub 16] [--out profiles/r08_c5_collision_stop.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import summary
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.rollouts import FLAG_NAMES, DeviceRollouts, pack_worlds
    B = a.rollouts
    w = pack_worlds([sc.make_world_c5(i, n_dyn=2) for i in range(B)])
    runs = {"default": {}, "stop": dict(collision_stop=a.n_sub), "stop_exact_sensing": dict(collision_stop=a.n_sub, exact_sensing=True)}
    res = {"workload": "C5: %d rollouts, make_world_c5(i, n_dyn=2), N = 5, max_steps 30" % B, "n_sub": a.n_sub, "runs": {}}
    for name, kw in runs.items():
        dr = DeviceRollouts(w, N=5, **kw)
        dr.run()                                                             # code object load, not timed
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
        r = {"flags": {FLAG_NAMES[v]: int((o["flags"] == v).sum()) for v in sorted(FLAG_NAMES)},
             "closed_loop_steps": int(o["steps"].sum()),
             "run_ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "repeats": a.repeats},
             "audit_of_this_run": summary(au, sc.DMIN)}
        res["runs"][name] = r
        if name == "default":
            applied = o["steps"] > 0
            res["default_audit_collisions"] = int(summary(au, sc.DMIN)["collisions"])
            res["default_audit_collisions_on_applied_steps"] = int(((au["first_collision"] >= 0) & applied).sum())
        del dr
        torch.cuda.synchronize()
    stop = res["runs"]["stop"]["flags"]["collision"]
    res["cross_check"] = {"stop_collisions": stop, "default_audit_collisions": res["default_audit_collisions"],
                          "holds": stop == res["default_audit_collisions_on_applied_steps"] == res["default_audit_collisions"]}
    res["steps_saved_by_the_stop"] = res["runs"]["default"]["closed_loop_steps"] - res["runs"]["stop"]["closed_loop_steps"]
    res["how"] = "HIP events around DeviceRollouts.run() (one fused launch), after one untimed run; audit.summary at n_sub"
    res["device"] = torch.cuda.get_device_name(0)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    if not res["cross_check"]["holds"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
