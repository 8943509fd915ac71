"""GPU tier of the fleet closed loop: obca_fleet_step against its serial definition (csrc/obca_fleet_core.h on the host,
tests/test_fleet_core.py), and ``scene.FleetLoop`` against ``scene.PoolLoop`` (the rollouts that see nobody must be its words),
against a parked car, against oncoming traffic and across streams.  N = 5, at most 16 steps.

Words.  Everything the kernel writes is a copy, a flag or arithmetic that csrc/obca_fleet_core.h keeps uncontracted, except
what goes through sin / cos and the distance: the rows and velocities of a car are word for word on ``exact`` worlds (heading
0, dyadic numbers) and within tests/test_fleet_core.py's derived bounds (A_TOL, ROW_TOL, V_TOL: the device's sin / cos
against the host libm's) elsewhere; the pair distance is audit::plan_distance as the library builds it (contracted), compared
at TOL = 1e-9 m, the bound tests/test_gpu_pool_loop.py uses for its rotated-rectangle measurement.  Which history words are
written, the flags and the masked windows are exact everywhere: the worlds keep every distance 1e-3 m and more from the
threshold."""
import numpy as np
import pytest
import torch

from tests import test_fleet_core as core
from tests.descriptor_case import TOL, _np, check_struct_mirror, device_descriptor_call
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib

pytestmark = pytest.mark.gpu

RUN, GOAL, CAP, FAILED, COLLISION = core.RUN, core.GOAL, core.CAP, core.FAILED, core.COLLISION


@pytest.fixture(scope="module")
def host():
    return core.load_host()


# ------------------------------------------------------------------------------------------------ 1. kernel against host core
def device_step(case, measure, rc=0, null=(), device=None, **over):
    """obca_fleet_step itself on the buffers of ``case`` uploaded between sentinels (``device_descriptor_call``)"""
    return device_descriptor_call(case, _lib.load().obca_fleet_step, (measure,), core.READ, core.INT, rc=rc, null=null, device=device,
                                  **over)


def both(host, case, measure, label=""):
    """the call on the device and on the host from the same buffers; the host's result stays in ``case``.  Returns the
    largest deviations (rows, distances)."""
    dev = device_step(case, measure)
    core.step_host(host, case, measure)
    want = dict(case.a)
    want["_car"] = core.car_mask(case)
    return core.compare(case, dev, want, dist_tol=TOL, label=label)


def mixed_world(G, V, Ks, rng, exact, **kw):
    """``core.fill_fleet`` at 3.6 m spacing (neighbours 0.2 m apart at heading 0, overlapping or clear at others) with
    what a running fleet holds: car 1 of every world has ended (GOAL in even worlds, FAILED in odd ones), the last car of the
    last world has no pose, car 0 of world 0 did not step, one input is no number"""
    c = core.fill_fleet(core.Case(G, V, Ks, exact=exact, **kw), rng, spacing=3.625)
    B = G * V
    if V > 1:
        for g in range(G):
            c["flags"][g * V + 1] = GOAL if g % 2 == 0 else FAILED
        c["x0"][B - 1, 1] = np.nan
        c["k"][0] = c.dims["step"]
    if V > 2:
        c["u0"][2, 0] = np.inf
    return c


SHAPES = [(1, 1, 3), (1, 2, 0), (3, 3, 2), (2, 16, 0), (1, 16, 48)]


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rotated"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "G%d_V%d_Ks%d" % s)
def test_kernel_equals_the_host_core(host, shape, exact):
    """both ``see`` modes x both ``predict`` modes x n_sub in {0, 1, 16} x measure 0 and 1 on every shape: the K = 64 edge, the
    1024-thread block, a world count that is no power of two.  The threshold 0.1 m lies below the distances of the exact
    worlds (0.225 m between neighbours) and flags cars of the rotated worlds of 16; no distance of these worlds comes within
    1e-3 m of it (asserted; the host core shows 3e-3 m at the least), so the flags are exact."""
    G, V, Ks = shape
    worst_r = worst_d = 0.0
    n_coll = 0
    for see in (core.SEE_ALL, core.SEE_LOWER):
        for predict in (core.PREDICT_VELOCITY, core.PREDICT_STATIC):
            for n_sub in (0, 1, 16):
                rng = np.random.default_rng(100 * G + V + Ks)               # the same world under every mode
                kw = dict(see=see, predict=predict, n_sub=n_sub, clearance=0.1, margin=0.25, S=4, step=3)
                for measure in (0, 1):
                    c = mixed_world(G, V, Ks, rng, exact, **kw)
                    r, d = both(host, c, measure, label=(see, predict, n_sub, measure))
                    worst_r, worst_d = max(worst_r, r), max(worst_d, d)
                    h = c["agent_clear_hist"]
                    m = (h != core.FILL_X) & np.isfinite(h)
                    assert not np.any(np.abs(h[m] - 0.1) < 1e-3)
                    n_coll += int((c["flags"] == COLLISION).sum())
                    if measure == 0 or n_sub == 0:
                        assert np.all(h == core.FILL_X)
                    elif V > 1:
                        assert np.all(h[1:, 3] != core.FILL_X) and h[0, 3] == core.FILL_X and np.all(h[:, :3] == core.FILL_X)
    print("G %d V %d Ks %d %s: largest |device - host| rows %.3e (bound %.3e), distances %.3e (bound %.0e); %d collision flags"
          % (G, V, Ks, "exact" if exact else "rotated", worst_r, core.ROW_TOL, worst_d, TOL, n_coll))
    if exact:
        assert worst_r == 0.0
    elif V == 16:
        assert n_coll > 0


def test_refused_calls_launch_nothing(host):
    rng = np.random.default_rng(6)
    c = mixed_world(2, 2, 1, rng, False, clearance=0.0)
    for measure in (0, 1):
        for over in core.REFUSED:
            device_step(c, measure, rc=core.E_INVAL, **over)
        for name in core.READ + core.WRITTEN:
            device_step(c, measure, rc=core.E_INVAL, null=(name,))
    device_step(c, 2, rc=core.E_INVAL)
    device_step(c, 1, rc=core.E_INVAL, device=-1)
    assert _lib.load().obca_fleet_step(None, 0, 0, None) == core.E_INVAL
    check_struct_mirror(None, _lib.load().obca_fleet_init, _lib.ObcaFleet)
    assert b"0.18" in _lib.load().obca_version()


# ------------------------------------------------------------------------------------------------ worlds for the loop
from tests import test_fleet_loop_host as fl  # noqa: E402
from tests import test_pool_loop_core as plc  # noqa: E402
from tests import test_scene_core as tsc  # noqa: E402
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scene  # noqa: E402
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver  # noqa: E402

N, S, TS, N_SEL, KS = fl.N, fl.S, fl.TS, fl.N_SEL, fl.KS
HISTORY = ("x_closed", "u_closed", "T_closed", "status", "iters", "clear", "sel")


@pytest.fixture(scope="module")
def hosts():
    return plc.load_host(), tsc.load_host(), core.load_host()


def make_fleet(w, V, **kw):
    B = len(w["start"])
    solver = BatchSolver(N, [4] * N_SEL, B)
    kw.setdefault("max_steps", S)
    kw.setdefault("goal_tol2", fl.GOAL_TOL2)
    lp = scene.FleetLoop(solver, V, w["pool_A"], w["pool_b"], w["start"], w["goal"], w["path"], w["path_len"], TS, **kw)
    return solver, lp


def make_plain(w, n_spare, far=100.0):
    """``scene.PoolLoop`` over the static pool with ``n_spare`` spare slots appended by hand, no car in anybody's pool"""
    B = len(w["start"])
    sA, sb = core.ref_spare_rows(far)
    pool_A = np.concatenate([w["pool_A"], np.tile(sA, (B, n_spare, 1, 1))], axis=1)
    pool_b = np.concatenate([w["pool_b"], np.tile(sb, (B, n_spare, 1))], axis=1)
    solver = BatchSolver(N, [4] * N_SEL, B)
    lp = scene.PoolLoop(solver, pool_A, pool_b, w["start"], w["goal"], w["path"], w["path_len"], TS,
                        pool_v=np.zeros((B, KS + n_spare, 2)), variant=8, max_steps=S, goal_tol2=fl.GOAL_TOL2)
    return solver, lp


def read_np(lp):
    out = lp.read()
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ 2. anchor
def test_rollouts_that_see_nobody_are_pool_loops_words():
    """V = 1 (the only agent slot is a spare), and car 0 of every world under see="lower" (it yields to nobody): every
    history of these rollouts equals, word for word, a plain ``PoolLoop`` over the same static pool with the spare slots
    appended by hand.  The wrapper changes nothing it should not."""
    w = fl.head_on_world(2)
    solver, lp = make_fleet(w, 1, margin=fl.MARGIN)
    got = read_np(lp.run())
    ps, plain = make_plain(w, 1)
    ref = read_np(plain.run())
    for k in ref:
        assert core.same_words(got[k], ref[k]), k
    assert np.all(np.isinf(got["agent_clear"][np.arange(S)[None, :] < got["steps"][:, None]])) and np.all(got["flags"] == GOAL)
    solver.close()
    ps.close()
    solver, lp = make_fleet(w, 2, see="lower", margin=fl.MARGIN)
    got = read_np(lp.run())
    ps, plain = make_plain(w, 2)
    ref = read_np(plain.run())
    for k in HISTORY + ("steps", "flags", "x0", "min_clear"):
        assert core.same_words(got[k][0::2], ref[k][0::2]), k
    assert core.same_words(got["pool_b"][0::2, :KS], ref["pool_b"][0::2, :KS])
    assert not core.same_words(got["x_closed"][1::2], ref["x_closed"][1::2])          # car 1 does see car 0
    print("steps fleet %s plain %s" % (got["steps"].tolist(), ref["steps"].tolist()))
    solver.close()
    ps.close()


# ------------------------------------------------------------------------------------------------ 3. a parked car
def measured_pairs(x_closed, steps, V, n_sub=8):
    """obca_fleet_step itself as a measuring device on driven trajectories [B,S+1,3]: agent_clear_hist [B,S]"""
    B = len(steps)
    c = core.Case(B // V, V, 0, N=N, S=S, n_sub=n_sub)
    c["agent_clear_hist"][...] = np.inf
    c["u0"][...] = 0.0
    c["flags"][...] = RUN
    c["variant_out"][...] = 0
    c["xref_out"][...] = 0.0
    for k in range(int(steps.max())):
        at = lambda d: np.stack([x_closed[q, min(k + d, int(steps[q]))] for q in range(B)])
        c["x_prev"][...], c["x0"][...] = at(0), at(1)
        c["k"][...] = np.where(steps > k, k + 1, -1)
        c.dims["step"] = k
        c["agent_clear_hist"][...] = device_step(c, 1)["agent_clear_hist"]
    return c["agent_clear_hist"].copy()


def test_a_parked_car_is_an_obstacle(hosts):
    """worlds of two cars in the corridor: car 0 starts at its goal, ends at once and stands rotated on car 1's straight route.
    Plain pool loops drive car 1 through it (obca_fleet_step measures a negative distance on their trajectories); FleetLoop
    takes car 1 round it to its goal with agent_min_clear >= 0 -- this fails without the feature.  Every solve of the fleet
    loop is held to the host yardstick (host select, host solver), re-seeded from the device's state before every step, at
    the bound and in the idiom of tests/test_gpu_pool_loop.py."""
    pl_host, scene_host, _ = hosts
    G = 2
    w = fl.parked_world(G)
    ps, plain = make_plain(w, 2)
    ref = read_np(plain.run())
    d = measured_pairs(ref["x_closed"], ref["steps"], 2)
    print("plain: flags %s steps %s inter-car distance min %s" % (ref["flags"].tolist(), ref["steps"].tolist(), d.min(axis=1).tolist()))
    assert np.all(ref["flags"] == GOAL) and np.all(d[1::2].min(axis=1) < 0.0)
    ps.close()

    solver, lp = make_fleet(w, 2, margin=fl.MARGIN)
    B = 2 * G
    c, _ = fl.host_cases(w, 2, margin=fl.MARGIN)
    Ts = np.full(B, TS)
    worst = 0.0
    for step in range(S):
        torch.cuda.synchronize()
        for k, name in (("x0", "x0"), ("u0", "u0"), ("xref_out", "xref"), ("variant_out", "variant_out"), ("pool_A", "pool_A"),
                        ("pool_b", "pool_b"), ("pool_v", "pool_v")):
            c[k][...] = _np(getattr(lp, name))
        s, o, on = fl.host_step(scene_host, c, Ts)
        assert np.all(np.isin(o["status"][on], (0, 1))), (step, o["status"])          # the scenario's own condition
        lp.step()
        torch.cuda.synchronize()
        r, sel = lp._last
        assert np.array_equal(_np(sel)[on], s["sel"][on]) and np.array_equal(_np(r.status), o["status"]), step
        for k in ("xopt", "uopt", "ts_opt"):
            diff = float(np.max(np.abs(_np(getattr(r, k)) - o[k])[on])) if on.any() else 0.0
            worst = max(worst, diff)
            assert diff < TOL, (step, k, diff)
    got = read_np(lp)
    print("fleet: flags %s steps %s agent_min_clear %s; largest |device - host| of a single solve %.3e"
          % (got["flags"].tolist(), got["steps"].tolist(), got["agent_min_clear"].tolist(), worst))
    assert np.all(got["flags"] == GOAL) and np.all(got["steps"][1::2] > 0) and np.all(got["steps"][0::2] == 0)
    assert np.all(got["agent_min_clear"][1::2] >= 0.0) and np.all(np.isinf(got["agent_min_clear"][0::2]))
    # the measurement is the kernel's own on the driven trajectory, and the advance's view of the (standing) car agrees
    again = measured_pairs(got["x_closed"], got["steps"], 2)
    assert core.same_words(again, got["agent_clear"])
    solver.close()


# ------------------------------------------------------------------------------------------------ 4. two moving cars
@pytest.mark.parametrize("see", ("lower", "all"))
def test_two_cars_head_on(see):
    """head-on on one corridor line.  Under "lower" car 1 yields: car 0 drives the words it drives alone.  "all" is included
    because the host loop shows every solve of it feasible on this world (tests/test_fleet_loop_host.py; on routes that make
    the cars swap places it is not, and neither mode passes).  Both cars reach their goals with agent_clear >= 0 at every
    step.  With agent_clearance above the smallest distance of that run the colliding step stays in the history, both cars of
    the pair end COLLISION at that step and every later solve is masked."""
    w = fl.head_on_world(2)
    solver, lp = make_fleet(w, 2, see=see, margin=fl.MARGIN)
    free = read_np(lp.run())
    h = free["agent_clear"]
    print("%s: flags %s steps %s agent_min_clear %s" % (see, free["flags"].tolist(), free["steps"].tolist(), free["agent_min_clear"].tolist()))
    assert np.all(free["flags"] == GOAL) and np.all(h >= 0.0) and np.all(free["steps"] >= 10)
    n = int(free["steps"].min())
    assert core.same_words(h[0::2, :n], h[1::2, :n])                              # one word per pair
    assert np.all(np.isinf(h[np.arange(S)[None, :] >= free["steps"][:, None]]))
    first = 8                                                                      # both cars of every world still run there
    thr = float(0.5 * (h[:, first - 1].min() + h[:, first].max()))
    assert h[:, first - 1].min() > thr > h[:, first].max()
    lp2 = scene.FleetLoop(solver, 2, w["pool_A"], w["pool_b"], w["start"], w["goal"], w["path"], w["path_len"], TS, see=see,
                          margin=fl.MARGIN, agent_clearance=thr, max_steps=S, goal_tol2=fl.GOAL_TOL2)
    got = read_np(lp2.run())
    assert np.all(got["flags"] == COLLISION) and np.all(got["steps"] == first + 1)
    for k in HISTORY + ("agent_clear",):
        m = first + 2 if k == "x_closed" else first + 1
        assert core.same_words(got[k][:, :m], free[k][:, :m]), k
    assert np.all(np.isinf(got["agent_clear"][:, first + 1:])) and np.all(got["iters"][:, first + 1:] == 0)
    assert np.all(got["sel"][:, first + 1:] == -1) and np.all(np.isnan(got["x_closed"][:, first + 2:]))
    solver.close()


# ------------------------------------------------------------------------------------------------ 5. streams
def test_run_on_a_side_stream_gives_the_same_words():
    w = fl.parked_world(2)
    solver, lp = make_fleet(w, 2, margin=fl.MARGIN)
    ref = read_np(lp.run())
    ins = {k: torch.as_tensor(v, device="cuda") for k, v in w.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lp2 = scene.FleetLoop(solver, 2, ins["pool_A"], ins["pool_b"], ins["start"], ins["goal"], ins["path"], ins["path_len"], TS,
                              margin=fl.MARGIN, max_steps=S, goal_tol2=fl.GOAL_TOL2).run()
    del ins
    junk = [torch.full((4, KS + 2, 4, 2), 7.0, dtype=torch.float64, device="cuda") for _ in range(16)]
    torch.cuda.synchronize()
    del junk
    got = read_np(lp2)
    for k in ref:
        assert core.same_words(got[k], ref[k]), k
    assert np.all(ref["flags"] == GOAL)
    solver.close()


def test_fleet_loop_refuses_what_it_cannot_drive():
    w = fl.head_on_world(1)
    solver = BatchSolver(N, [4] * N_SEL, 2)
    args = (w["pool_A"], w["pool_b"], w["start"], w["goal"], w["path"], w["path_len"])
    with pytest.raises(ValueError):
        scene.FleetLoop(solver, 2, *args, TS, variant=4)                           # a free-time car has its own clock
    with pytest.raises(ValueError):
        scene.FleetLoop(solver, 2, *args, np.array([1.5, 1.0]))                    # two step lengths in one world
    with pytest.raises(ValueError):
        scene.FleetLoop(solver, 3, *args, TS)                                      # 2 rollouts are no worlds of 3
    with pytest.raises(ValueError):
        scene.FleetLoop(solver, 2, *args, TS, see="higher")
    solver.close()
    solver = BatchSolver(N, [4], 2)
    lp = scene.FleetLoop(solver, 2, None, None, *args[2:], TS, max_steps=2).run()  # Ks = 0: the cars alone, beyond the cap too
    lp.step()
    got = read_np(lp)
    assert lp.K == 2 and lp.Ks == 0 and np.all(got["flags"] == CAP) and np.all(np.isfinite(got["agent_clear"]))
    solver.close()
