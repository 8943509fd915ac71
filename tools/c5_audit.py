"""Collision audit of the C5 workload (4096 closed-loop rollouts, make_world_c5(i, n_dyn=2), N = 5): how many rollouts
hit something, where, and what the audit costs.

    python tools/c5_audit.py [--rollouts 4096] [--n-sub 16] [--out profiles/r07_c5_audit.json]

Prints one JSON object: audit.summary at n_sub (samples between the knots) and at n_sub = 1 (knots only), the colliding
rollouts split by where their first collision lies (a knot inside an obstacle vs corner cutting between two knots that
are both clear; on a q8 step -- the lidar gate saw only some of the present boxes, so the solver was handed another box's
vertices with this box's velocity -- or not), and the audit kernel's time from HIP events around the call."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import summary
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.rollouts import DeviceRollouts, pack_worlds
    B = a.rollouts
    w = pack_worlds([sc.make_world_c5(i, n_dyn=2) for i in range(B)])
    dr = DeviceRollouts(w, N=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dr.run()
    torch.cuda.synchronize()
    run_s = time.perf_counter() - t0
    o = {k: v.cpu().numpy() for k, v in dr.read().items()}

    dr.audit(n_sub=a.n_sub)                                                 # first launch (code object load) not timed
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        au = dr.audit(n_sub=a.n_sub, per_step=True)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    au = {k: v.cpu().numpy() for k, v in au.items()}
    kn = {k: v.cpu().numpy() for k, v in dr.audit(n_sub=1, per_step=True).items()}

    # q8 steps: a box present but not sensed while another one was (the solver got rows, but of the wrong box)
    dyn = o["dyn"]                                                          # [B, S, n_dyn, 4] cx, cy, present, sensed
    present, sensed = dyn[..., 2] > 0, dyn[..., 3] > 0
    q8 = (present & ~sensed).any(-1) & sensed.any(-1)
    unsensed = (present & ~sensed).any(-1)                                 # any present box the solver did not see
    coll = np.flatnonzero(au["first_collision"] >= 0)
    split = {"at_a_knot": 0, "between_clear_knots": 0, "on_q8_step": 0, "on_step_with_unsensed_box": 0,
             "hit_moving_box": 0, "hit_static": 0}
    n_static = len(w.m_static)
    for b in coll:
        s = int(au["first_collision"][b])
        if kn["step_min"][b, s] < 0:
            split["at_a_knot"] += 1
        else:
            split["between_clear_knots"] += 1
        if s < q8.shape[1] and q8[b, s]:
            split["on_q8_step"] += 1
        if s < unsensed.shape[1] and unsensed[b, s]:
            split["on_step_with_unsensed_box"] += 1
        # which obstacle the worst sample of that interval touches is the rollout's arg_obst when the interval is the worst
        if int(au["arg_obst"][b]) >= n_static:
            split["hit_moving_box"] += 1
        else:
            split["hit_static"] += 1
    res = {"workload": "C5: %d rollouts, make_world_c5(i, n_dyn=2), N = 5, max_steps 30" % B,
           "n_sub": a.n_sub,
           "summary": summary(au, sc.DMIN),
           "summary_knots_only": summary(kn, sc.DMIN),
           "collisions_by_first_colliding_interval": split,
           "q8_steps": int(q8.sum()), "steps": int((o["variant"] > 0).sum()),
           "rollout_flags": {k: int((o["flags"] == v).sum()) for k, v in (("goal", 1), ("cap", 2), ("failed", 3), ("running", 0))},
           "audit_ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "repeats": a.repeats,
                        "how": "HIP events around DeviceRollouts.audit(n_sub, per_step=True), after one untimed launch"},
           "rollout_run_s": run_s,
           "device": torch.cuda.get_device_name(0)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
