"""The fleet closed loop on the host builds alone -- host select (tests/test_scene_core.py), host solver
(native_build.lpi_solve, variant 8), host pool-loop advance (tests/test_pool_loop_core.py) and host fleet step
(tests/test_fleet_core.py) -- as the yardstick of tests/test_gpu_fleet.py, and the recipe behind its scenario constants:
they are chosen here, on the CPU, so that every solve of the host loop is feasible until the rollouts end.

The corridor is tests/test_gpu_pool_loop.crossing_world's: two walls of 4 rows (y <= 1 and y >= 9 over x in [0, 39]), straight
routes at 0.6 m spacing driven at Ts = 1.5 s (0.4 m/s), N = 5, n_sel = 3 (the walls and the nearest car)."""
import functools

import numpy as np
import pytest

from tests import native_build
from tests import test_fleet_core as core
from tests import test_pool_loop_core as plc
from tests import test_scene_core as tsc
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.model_obstacle import obstacleModel

N, S, TS, N_SEL, KS = 5, 16, 1.5, 3, 2
SPACING, GOAL_TOL2 = 0.6, 1.0
RUN, GOAL, CAP, FAILED, COLLISION = core.RUN, core.GOAL, core.CAP, core.FAILED, core.COLLISION


@functools.lru_cache(maxsize=None)
def walls():
    """pool_A [2,4,2], pool_b [2,4]: the corridor's two walls"""
    polys = [[[39, 9], [0, 9], [0, 10], [39, 10], [39, 9]], [[0, 1], [39, 1], [39, 0], [0, 0], [0, 1]]]
    A, b = obstacleModel().obstacle_H_Represent(2, [5, 5], polys)
    return A.reshape(2, 4, 2), b[:, 0].reshape(2, 4)


def straight_route(x_first, y, points, direction=1.0, P=None):
    """[3,P]: ``points`` route points from (x_first, y) on along +x (direction 1, heading 0) or -x (direction -1, heading pi),
    SPACING apart, padded with the last point"""
    P = points if P is None else P
    i = np.minimum(np.arange(P), points - 1)
    path = np.zeros((3, P))
    path[0], path[1], path[2] = x_first + direction * SPACING * i, y, 0.0 if direction > 0 else np.pi
    return path


def fleet_world(cars, G=1, P=14):
    """G copies (world g shifted by 0.25 g m along x, so that the worlds differ) of one world of V = len(cars) cars in the
    corridor; a car is (route [3,P] or a pose for a car that stands at its goal, path_len).  Returns the dict ``make_loop``
    takes: static pool_A [B,2,4,2], pool_b [B,2,4], start [B,3], goal [B,2], path [B,3,P], path_len [B]"""
    V = len(cars)
    A, b = walls()
    w = dict(pool_A=np.tile(A, (G * V, 1, 1, 1)), pool_b=np.tile(b, (G * V, 1, 1)), start=np.zeros((G * V, 3)), goal=np.zeros((G * V, 2)),
             path=np.zeros((G * V, 3, P)), path_len=np.zeros(G * V, np.int32))
    for g in range(G):
        for a, (route, plen) in enumerate(cars):
            q = g * V + a
            route = np.asarray(route, float)
            path = np.repeat(route[:, None], P, axis=1) if route.ndim == 1 else route.copy()
            path[0] += 0.25 * g
            w["path"][q], w["path_len"][q] = path, plen
            w["start"][q], w["goal"][q] = path[:, 0], path[:2, plen - 1]
    return w


# ---- the scenarios of tests/test_gpu_fleet.py.  The constants were chosen with the host loop below; what it shows on them is
# asserted by the tests at the end of this file.
#   parked   car 0 stands at its goal (path_len 1), rotated by 1.25 rad, its upper corner 0.5 m inside the strip car 1's
#            footprint sweeps on its straight route at y = 5 (10 points from x = 4).  Tried: poses with the corner 0.25 .. 0.85 m
#            inside the strip at x = 6.5 .. 8.5 and routes of 14 points (no car reaches a goal 7.8 m away in 16 steps of
#            0.4 m/s).  With margin 0 the host loop passes at 0.025 m; MARGIN = 0.1 gives 0.149 m and is what the tests use.
#   head-on  two cars towards each other on the line y = 5, 13.5 m apart, each with a route of 10 points: they end 4 m apart,
#            nose to nose, and the second one brakes early because it sees the first one coming.  Starts 12 .. 16 m apart
#            were tried: below 16.5 m car 1 creeps and ends at the cap, and on routes that make the cars SWAP places (starts
#            9 m apart) the yielding car backs off and never passes -- under see="all" both solves go infeasible (status 2).
#            Passing oncoming traffic on one line is not something this loop does; DESIGN.md 5l says so.
PARKED_POSE = (7.5, 2.9, 1.25)
MARGIN = 0.1
ROUTE_POINTS, PATH_MAX = 10, 14


def parked_world(G=2):
    return fleet_world([(PARKED_POSE, 1), (straight_route(4.0, 5.0, ROUTE_POINTS, P=PATH_MAX), ROUTE_POINTS)], G=G, P=PATH_MAX)


def head_on_world(G=2):
    """two cars towards each other on the line y = 5: car 0 along +x, car 1 along -x"""
    return fleet_world([(straight_route(3.0, 5.0, ROUTE_POINTS, P=PATH_MAX), ROUTE_POINTS),
                        (straight_route(16.5, 5.0, ROUTE_POINTS, direction=-1.0, P=PATH_MAX), ROUTE_POINTS)], G=G, P=PATH_MAX)


# ---- the host loop
def host_step(scene_host, c, Ts):
    """one step's select and solve on the host builds, for the rollouts whose variant is not 0"""
    B = c.dims["B"]
    x0, u0, xref, variant = c["x0"].copy(), c["u0"].copy(), c["xref_out"].copy(), c["variant_out"].copy()
    s = tsc.host_select(scene_host, c["pool_A"], c["pool_b"], xref, N_SEL, pool_v=c["pool_v"], Ts=Ts, x0=x0, variant=variant, n_sub=1)
    o = dict(xopt=np.zeros((B, 3, N + 1)), uopt=np.zeros((B, 2, N)), ts_opt=np.zeros(B), status=np.full(B, -5, np.int32),
             iters=np.zeros(B, np.int32))
    on = (variant != 0) & (s["ok"] == 1)
    if on.any():
        r = native_build.lpi_solve(8, N, [4] * N_SEL, x0[on], u0[on], xref[on], s["A"][on], s["b"][on], Ts[on])
        for k in o:
            o[k][on] = r[k]
    return s, o, on


def host_cases(w, V, see="all", predict="velocity", margin=0.0, agent_clearance=core.NEVER, agent_n_sub=8, far=100.0):
    """(pool-loop case, fleet case) over ONE set of buffers: the pool with V spare agent slots appended"""
    B = len(w["start"])
    P = w["path"].shape[2]
    c = plc.Case(B, KS + V, 4, N, N_SEL, P, S, moving=True, variant=8, n_sub=8, goal_tol2=GOAL_TOL2)
    sA, sb = core.ref_spare_rows(far)
    c["pool_A"][:, :KS], c["pool_b"][:, :KS] = w["pool_A"], w["pool_b"]
    c["pool_A"][:, KS:], c["pool_b"][:, KS:] = sA, sb
    c["pool_v"][...] = 0.0
    for k in ("goal", "path", "path_len"):
        c[k][...] = w[k]
    c["x0"][...] = w["start"]
    f = core.Case(B // V, V, KS, N=N, S=S, n_sub=agent_n_sub, see={"all": core.SEE_ALL, "lower": core.SEE_LOWER}[see],
                  predict={"velocity": core.PREDICT_VELOCITY, "static": core.PREDICT_STATIC}[predict], clearance=agent_clearance,
                  margin=margin, far=far)
    for k in ("x0", "u0", "k", "flags", "pool_A", "pool_b", "pool_v", "xref_out", "variant_out"):
        f.a[k] = c.a[k]
    f["agent_clear_hist"][...] = np.inf
    return c, f


def host_fleet_loop(pl_host, scene_host, fleet_host, w, V, steps=S, **kw):
    """the whole loop on the host builds; returns (pool-loop case, fleet case, feasible_everywhere [B])"""
    c, f = host_cases(w, V, **kw)
    B = c.dims["B"]
    Ts = np.full(B, TS)
    plc.advance(pl_host, c, 0)
    f["x_prev"][...] = c["x0"]
    core.step_host(fleet_host, f, 0)
    ok = np.ones(B, bool)
    for step in range(steps):
        f["x_prev"][...] = c["x0"]
        s, o, on = host_step(scene_host, c, Ts)
        ok &= ~on | np.isin(o["status"], (0, 1))
        for k in ("xopt", "uopt", "ts_opt", "status", "iters"):
            c[k][...] = o[k]
        c["sel"][...] = s["sel"]
        plc.advance(pl_host, c, 1)
        f.dims["step"] = step
        core.step_host(fleet_host, f, 1)
    return c, f, ok


@pytest.fixture(scope="module")
def hosts():
    return plc.load_host(), tsc.load_host(), core.load_host()


def pair_history(fleet_host, x_closed, steps, i, j, n_sub=8, ego=core.EGO):
    """the distance of cars i < j of one world over every interval either drove, from the driven trajectories [B,S+1,3]"""
    e = np.array(ego, float)
    out = []
    for k in range(int(max(steps[i], steps[j]))):
        p = [np.ascontiguousarray(x_closed[q, min(k + d, int(steps[q]))]) for q in (i, j) for d in (0, 1)]
        out.append(fleet_host.fleet_pair_clear_host(*(v.ctypes.data for v in p), e.ctypes.data, n_sub))
    return np.array(out)


# ---- what the host loop shows on the scenarios
def test_parked_car_host_loop(hosts):
    """FleetLoop's recipe on the host: every solve feasible, car 1 passes the parked car at 0.149 m and reaches its goal in 14
    steps; the same two rollouts as worlds of their own (V = 1: plain pool loops) drive car 1 through car 0 (-0.5 m)"""
    w = parked_world(2)
    c, f, ok = host_fleet_loop(*hosts, w, 2, margin=MARGIN)
    print("fleet: flags %s steps %s agent_min %s" % (c["flags"].tolist(), c["k"].tolist(), f["agent_clear_hist"].min(axis=1).tolist()))
    assert ok.all() and list(c["flags"]) == [GOAL] * 4 and list(c["k"]) == [0, 14, 0, 14]
    assert np.all(f["agent_clear_hist"][[1, 3]].min(axis=1) > 0.1) and np.all(np.isinf(f["agent_clear_hist"][[0, 2]]))
    c, f, ok = host_fleet_loop(*hosts, w, 1)
    d = pair_history(hosts[2], c["x_closed"], c["k"], 0, 1)
    print("plain: flags %s steps %s pair min %.3f" % (c["flags"].tolist(), c["k"].tolist(), d.min()))
    assert ok.all() and list(c["flags"]) == [GOAL] * 4 and d.min() < -0.4 and np.all(np.isinf(f["agent_clear_hist"]))


@pytest.mark.parametrize("see", ("lower", "all"))
def test_head_on_host_loop(hosts, see):
    """both modes are feasible at every solve on this world and both cars reach their goals; under "lower" car 0 drives as if
    alone (12 steps) and car 1 takes 14, under "all" both take 13"""
    c, f, ok = host_fleet_loop(*hosts, head_on_world(1), 2, see=see, margin=MARGIN)
    h = f["agent_clear_hist"]
    print("%s: flags %s steps %s agent_min %s" % (see, c["flags"].tolist(), c["k"].tolist(), h.min(axis=1).tolist()))
    assert ok.all() and list(c["flags"]) == [GOAL, GOAL] and list(c["k"]) == ([12, 14] if see == "lower" else [13, 13])
    assert h.min() > 0.9
    n = int(min(c["k"]))
    assert core.same_words(h[0, :n], h[1, :n]) and np.all(np.diff(h[1, :n]) < 0)      # one word per pair, closing in
