"""GPU tier of the closed loop over scene pools: obca_pool_loop_advance against its serial definition
(csrc/obca_poolloop_core.h on the host, tests/test_pool_loop_core.py), ``scene.PoolLoop`` against the closed loop that exists
(``rollouts.DeviceRollouts``), against the host builds of the scene, solver and advance cores, against ``scene.pool_clearance``
as an independent audit, and ``scene.drive_maps`` against its hand composition.  B <= 16, N = 5, at most 12 steps.

Words.  Everything the advance kernel writes is a copy, a count or arithmetic that csrc/obca_poolloop_core.h keeps uncontracted,
except the clearance: that is scene::score_obstacle, which the library builds with contraction on and the device's own
sin / cos, exactly as obca_scene_select does -- so it equals obca_scene_select's words on the device (tests 4 and 5 below
compare those exactly), and the host's only where the arithmetic is exact.  Test 1 therefore runs on worlds in which it is
(headings 0, wall-like axis-parallel obstacles above and below the route, dyadic rows, velocities and step lengths; n_sub a
power of two) and compares EVERY output word for word; one more case with rotated rectangles around the route compares
clear_hist at TOL = 1e-9 m, the bound tests/test_gpu_scene.py sets for the same measurement, and the rest word for word."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import native_build
from tests import test_pool_loop_core as core
from tests import test_scene_core as scene_core
from tests.descriptor_case import TOL, _np, check_struct_mirror, device_descriptor_call
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib, scenarios, scene
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.model_obstacle import obstacleModel, rectangle_vertices
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.openloop import route_search
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.rollouts import DeviceRollouts, PackedWorlds
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams

pytestmark = pytest.mark.gpu

N, S, TS = 5, 12, 0.1
RUN, GOAL, CAP, FAILED, COLLISION = core.RUN, core.GOAL, core.CAP, core.FAILED, core.COLLISION
HISTORY = ("x_closed", "u_closed", "T_closed", "status", "iters", "clear", "sel")


@pytest.fixture(scope="module")
def host():
    return core.load_host()


@pytest.fixture(scope="module")
def scene_host():
    return scene_core.load_host()


def same(a, b):
    return core.same_words(_np(a) if isinstance(a, torch.Tensor) else a, _np(b) if isinstance(b, torch.Tensor) else b)


# ------------------------------------------------------------------------------------------------ 1. kernel against host core
def device_advance(case, solved, rc=0, null=(), **over):
    """obca_pool_loop_advance itself on the buffers of ``case`` uploaded between sentinels (``device_descriptor_call``)"""
    return device_descriptor_call(case, _lib.load().obca_pool_loop_advance, (solved,), (), core.INT, rc=rc, null=null, **over)


def both(host, case, solved, clear_tol=None):
    """the call on the device and on the host from the same buffers; the host's result stays in ``case``"""
    dev = device_advance(case, solved)
    core.advance(host, case, solved)
    for name in case.a:
        if name == "clear_hist" and clear_tol is not None:
            a, b = dev[name], case.a[name]
            fin = np.isfinite(b)                                  # +inf: the fill of a step not measured
            assert np.array_equal(np.isinf(a), np.isinf(b)) and np.all(np.abs(a[fin] - b[fin]) < clear_tol)
            case.a[name][...] = a                                 # both sides go on from the device's words
            continue
        assert core.same_words(dev[name], case.a[name]), (name, solved)


# where the car of a route of plen points starts: next to this route point.  63 -> the last lane's only point, 64 -> a point
# of lane 0's first pass that is not the route's first, 65 -> point 64, the first that a lane meets in its SECOND pass of the
# strided search, 130 -> point 100, a second-pass point in the middle of the wavefront
START_POINT = {1: 0, 2: 0, 63: 62, 64: 32, 65: 64, 130: 100}


def exact_world(case, rng, shift=0):
    """worlds on which host and device measure the same words (module docstring): rollout b follows a straight route of
    PATH_LENS[(b + shift) % 6] points at height 5, heading 0, and starts 0.25 m behind point START_POINT[length] of it; the
    goal is the last point for the routes of 1 and 2 points (a start at the goal where the car's lateral offset allows) and
    1000 m away otherwise; obstacle i is a wall 512 m long and 1 m thick (E = 4) or a half-plane (E = 1) above or below the
    route, 2.5 m and more from it; velocities multiples of 1/8 m/s"""
    dm = case.dims
    B, K, E, P = dm["B"], dm["K"], dm["E"], dm["path_max"]
    nx, ny = (0.0, 1.0, 0.0, -1.0), (1.0, 0.0, -1.0, 0.0)       # rows: top, right, bottom, left
    for b in range(B):
        for i in range(K):
            up = (i + b) % 2 == 0
            cy = 5.0 + (1 if up else -1) * (3.0 + 0.25 * i + 0.125 * b)
            if E == 4:
                h = (0.5, 256.0, 0.5, 256.0)
                for r in range(4):
                    case["pool_A"][b, i, r] = (nx[r], ny[r])
                    case["pool_b"][b, i, r] = nx[r] * 100.0 + ny[r] * cy + h[r]
            else:                                                 # E = 1: the half-plane beyond cy
                case["pool_A"][b, i, 0] = (0.0, -1.0 if up else 1.0)
                case["pool_b"][b, i, 0] = -cy if up else cy
        case["pool_v"][b] = rng.integers(-2, 3, (K, 2)) / 8.0
        plen = core.PATH_LENS[(b + shift) % len(core.PATH_LENS)]
        case["path"][b] = core.straight_path(P, plen)
        case["path_len"][b] = plen
        case["goal"][b] = case["path"][b, :2, plen - 1] if plen <= 2 else (1000.0, 5.0)
        case["x0"][b] = (1.5 * START_POINT[plen] - 0.25, 5.0 + 0.125 * (b % 4), 0.0)
    return case


def mixed_solve(case, step, fail_status=None, fail_nan=None):
    """scripted solves: the window as the plan, dyadic inputs and step lengths; rollout fail_status = (index, step) gets
    status 2 at that step, rollout fail_nan = (index, step) a NaN knot"""
    core.script_solve(case, ts=0.5)
    B = case.dims["B"]
    case["uopt"][...] = 0.125
    case["ts_opt"][...] = 0.5 + 0.25 * (np.arange(B) % 3)
    if fail_status is not None and step == fail_status[1]:
        case["status"][fail_status[0]] = 2
    if fail_nan is not None and step == fail_nan[1]:
        case["xopt"][fail_nan[0], 0, 1] = np.nan


# the whole product: B across a block's four wavefronts, K, E, N.  Which route lengths a B holds: SHIFT below
KERNEL_CASES = [(B, K, E, n) for B in (1, 4, 5, 9) for K in (1, 3, 64) for E in (1, 4) for n in (1, 5)]
SHIFT = {1: 4, 4: 2, 5: 1, 9: 0}          # B = 1: 65; B = 4: 63, 64, 65, 130; B = 5: 2, 63, 64, 65, 130; B = 9: all six, then 1, 2, 63


@pytest.mark.parametrize("moving", (False, True), ids=("static", "moving"))
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "B%d_K%d_E%d_N%d" % c)
def test_kernel_equals_the_host_core(host, case, moving):
    """a start (solved = 0), then three steps (solved = 1): every buffer word for word, sentinels intact.  Every B runs its
    routes of 63, 64, 65 and 130 points (B = 1: 65) through all four calls as RUN rollouts; B = 9 runs all six lengths and
    mixes in a start at the goal (rollout 0), a failing status at step 0 (6), a NaN knot at step 1 (7) and a bad path_len
    (8); in B = 5 rollout 0 reaches its goal at the first step"""
    B, K, E, n = case
    rng = np.random.default_rng(1000 * B + 10 * K + E + n)
    c = exact_world(core.Case(B, K, E, n, min(K, 3), 130, 4, moving=moving, n_sub=4), rng, SHIFT[B])
    fail_status, fail_nan = ((6, 0), (7, 1)) if B == 9 else (None, None)
    if B == 9:
        c["path_len"][8] = 131                                    # FAILED at the start
        c["goal"][6:] = (1000.0, 5.0)                             # 6 and 7 are to fail, not to arrive
    both(host, c, 0)
    long_routes = np.flatnonzero(c["path_len"] <= 130)
    long_routes = long_routes[c["path_len"][long_routes] >= 63]
    assert np.all(c["flags"][long_routes] == RUN) and len(long_routes) >= min(B, 4)
    for b in long_routes:                                         # the window starts where the car stands, lane-pass and all
        at = START_POINT[int(c["path_len"][b])]
        assert c["xref_out"][b, 0, 0] == c["path"][b, 0, at], b
    for step in range(3):
        mixed_solve(c, step, fail_status, fail_nan)
        both(host, c, 1)
    flags = c["flags"]
    keep = long_routes[long_routes < 6] if B == 9 else long_routes
    assert np.all(flags[keep] == RUN) and np.all(c["k"][keep] == 3) and np.isfinite(c["clear_hist"][keep, :3]).all()
    if B == 9:
        assert sorted(int(v) for v in c["path_len"][:6]) == list(core.PATH_LENS)
        assert flags[0] == GOAL and c["k"][0] == 0                 # a one-point route whose point the car stands next to
        assert [int(v) for v in flags[[6, 7, 8]]] == [FAILED] * 3 and list(c["k"][[6, 7, 8]]) == [0, 1, 0]


def test_window_reduction_on_the_device(host):
    """the lane combine of the window search, which the serial host loop does not have: ties within a lane's pass, between a
    first-pass and a second-pass point 64 apart (the same lane), between two second-pass points, a minimum deep in the second
    pass, nothing found, and a NaN point -- every buffer word for word after a start and after a step"""
    rng = np.random.default_rng(8)
    P = 130
    c = core.fill_world(core.Case(8, 2, 4, N, 1, P, 4), rng, far_pool=True)
    c["goal"][...] = (-500.0, -500.0)
    path = c["path"]
    path[0] = core.straight_path(P, P, spacing=2.0)               # 0: equidistant from points 3 and 4
    c["x0"][0] = (7.0, 5.0, 0.0)
    path[1, :2, 40] = path[1, :2, 2]                              # 1: the route comes back to point 2 at point 40
    c["x0"][1, :2] = path[1, :2, 2]
    c["x0"][2] = (-400.0, 5.0, 0.0)                               # 2: every point farther than sqrt(1e5) m
    path[3, 0, 10] = np.nan                                       # 3: a NaN point, the car next to it
    c["x0"][3, :2] = (15.1, 5.0)
    path[4, :2, 66] = path[4, :2, 2]                              # 4: a tie 64 points apart: lane 2's first and second pass
    c["x0"][4, :2] = path[4, :2, 2] + (0.0, 0.25)
    path[5, :2, 120] = path[5, :2, 70]                            # 5: a tie between two second-pass points of different lanes
    c["x0"][5, :2] = path[5, :2, 70] + (0.0, 0.25)
    c["x0"][6, :2] = path[6, :2, 100] + (0.3, 0.1)                # 6: the minimum at point 100
    path[7, :2, 3] = path[7, :2, 127]                             # 7: a tie between a first-pass point and the route's end
    c["x0"][7, :2] = path[7, :2, 127] + (0.0, -0.25)
    both(host, c, 0)
    assert np.all(c["flags"] == RUN)
    for i, i0 in ((0, 3), (1, 2), (2, 0), (4, 2), (5, 70), (6, 100), (7, 3)):
        assert core.same_words(c["xref_out"][i][:, :2], path[i][:, i0:i0 + 2]), i
    core.script_solve(c, rng, ts=0.7)
    both(host, c, 1, clear_tol=TOL)
    assert np.all(c["k"] == 1)


def test_kernel_on_rotated_rectangles_around_the_route(host):
    """the measurement where the arithmetic is not exact: rotated rectangles beside and on the route, n_sub = 16, moving --
    clear_hist at TOL, every other buffer word for word"""
    rng = np.random.default_rng(5)
    c = core.fill_world(core.Case(9, 7, 4, N, 3, 30, 4, moving=True, n_sub=16), rng)
    both(host, c, 0)
    for _ in range(3):
        core.script_solve(c, rng, ts=0.7)
        both(host, c, 1, clear_tol=TOL)
    assert np.all(c["k"] == 3) and np.isfinite(c["clear_hist"][:, :3]).all()


def test_refused_calls_launch_nothing(host):
    rng = np.random.default_rng(6)
    c = exact_world(core.Case(5, 3, 4, N, 2, 130, 4), rng)
    both(host, c, 0)
    mixed_solve(c, 0)
    for solved in (0, 1):
        for over in core.REFUSED:
            device_advance(c, solved, rc=core.E_INVAL, **over)
        for name in ("pool_A", "path_len", "x0", "flags", "clear_hist", "sel_hist", "xref_out", "variant_out"):
            device_advance(c, solved, rc=core.E_INVAL, null=(name,))
        device_advance(c, 2, rc=core.E_INVAL)
    for name in core.SOLVE:
        device_advance(c, 1, rc=core.E_INVAL, null=(name,))
    assert _lib.load().obca_pool_loop_advance(None, 0, 0, None) == core.E_INVAL
    d = c.descriptor()
    assert _lib.load().obca_pool_loop_advance(ctypes.byref(d), 0, -1, None) == core.E_INVAL
    check_struct_mirror(None, _lib.load().obca_pool_loop_init, _lib.ObcaPoolLoop)


# ------------------------------------------------------------------------------------------------ worlds for the loop
ROUTE_POINTS, GOAL_POINT, GOAL_TOL2 = 12, 7, 1.0   # the route goes on beyond the goal, so the car arrives at speed; a car that
                                                   # advances about 1 m per step has a knot within 1 m of the goal


@functools.lru_cache(maxsize=None)
def loop_world(seed, n_distract=0):
    """``scenarios.make_instance(seed, three_boxes=True)`` -- the corridor's two walls and one box, 4 rows each -- as a closed-loop
    world: the ROUTE_POINTS points of its lattice route that start 5 m before the box (the car starts on the first with the
    route's heading, point GOAL_POINT is the goal), and ``n_distract`` unit squares (generator ``default_rng(seed + 777)``: centre x
    from 3 m behind the start to 6 m beyond the goal, y in [2, 8]; redrawn while closer than 0.6 m to the footprint at a route
    point or 0.2 m to the box).  Returns pool_A [K,4,2], pool_b [K,4], start [3], goal [2], path [3,ROUTE_POINTS]"""
    q = scenarios.make_instance(seed, N, three_boxes=True)
    path, (cx, cy, l, w) = q["path"], q["box"]
    j0 = int(np.clip(np.floor(cx - l / 2) - 3 - 5, 0, path.shape[1] - ROUTE_POINTS))
    sub = path[:, j0:j0 + ROUTE_POINTS].copy()
    K = 3 + n_distract
    pool_A, pool_b = np.zeros((K, 4, 2)), np.zeros((K, 4))
    pool_A[:3], pool_b[:3] = q["A"].reshape(3, 4, 2), q["b"].reshape(3, 4)
    rng, om = np.random.default_rng(seed + 777), obstacleModel()
    own = np.array(rectangle_vertices(cx, cy, 0.0, l, w)[:4])
    cars = [scenarios._car_corners(sub[:, j]) for j in range(ROUTE_POINTS)]
    for k in range(3, K):
        while True:
            rect = rectangle_vertices(rng.uniform(sub[0, 0] - 3.0, sub[0, -1] + 6.0), rng.uniform(2.0, 8.0), 0.0, 1.0, 1.0)
            sq = np.array(rect[:4])
            if min(scenarios._poly_distance(c, sq) for c in cars) >= 0.6 and scenarios._poly_distance(own, sq) >= 0.2:
                break
        A, b = om.obstacle_H_Represent(1, [5], [rect])
        pool_A[k], pool_b[k] = A, b[:, 0]
    return dict(pool_A=pool_A, pool_b=pool_b, start=sub[:, 0].copy(), goal=sub[:2, GOAL_POINT].copy(), path=sub)


def loop_worlds(seeds, n_distract=0):
    ws = [loop_world(s, n_distract) for s in seeds]               # (cached: np.stack copies)
    out = {k: np.stack([w[k] for w in ws]) for k in ws[0]}
    out["path_len"] = np.full(len(ws), ROUTE_POINTS, np.int32)
    return out


def make_loop(w, n_sel, Ts=TS, **kw):
    B = len(w["start"])
    solver = BatchSolver(N, [4] * n_sel, B)
    kw.setdefault("max_steps", S)
    kw.setdefault("goal_tol2", GOAL_TOL2)
    lp = scene.PoolLoop(solver, w["pool_A"], w["pool_b"], w["start"], w["goal"], w["path"], w["path_len"], Ts,
                        pool_v=w.get("pool_v"), **kw)
    return solver, lp


def read_np(lp):
    out = lp.read()
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ 2. anchor
ANCHOR_SEEDS = list(range(8))


def test_anchor_to_device_rollouts():
    """static worlds whose three obstacles all have 4 rows, K = n_sel = 3: the selection is every obstacle in order, so every
    solve of PoolLoop (variant 4, rounds = 0, Ts = Ts0) reads the words DeviceRollouts' solve reads, and the two closed loops
    must agree word for word"""
    w = loop_worlds(ANCHOR_SEEDS)
    B = len(ANCHOR_SEEDS)
    pw = PackedWorlds()
    pw.m_static, pw.n_dyn, pw.sense_dis, pw.xL, pw.xU = [4, 4, 4], 0, 10.0, scenarios.XL, scenarios.XU
    pw.start, pw.goal, pw.path, pw.path_len = w["start"], w["goal"], w["path"], w["path_len"]
    pw.static_A, pw.static_b, pw.dyn = w["pool_A"].reshape(B, 12, 2), w["pool_b"].reshape(B, 12), np.zeros((B, 0, 13))
    params = SolverParams(xL=pw.xL, xU=pw.xU)
    dr = DeviceRollouts(pw, N=N, params=params, Ts0=TS, max_steps=S)
    dr.set_mode("lockstep")
    dr.reset()
    dr.run()
    ref = {k: _np(v) for k, v in dr.read().items()}
    solver, lp = make_loop(w, 3, variant=4, params=params, n_sub=0, goal_tol2=0.1)
    lp.run()
    got = read_np(lp)
    print("steps %s flags %s (DeviceRollouts: %s %s)" % (got["steps"].tolist(), got["flags"].tolist(), ref["steps"].tolist(), ref["flags"].tolist()))
    assert np.array_equal(got["steps"], ref["steps"]) and np.array_equal(got["flags"], ref["flags"])
    for i in range(B):
        k = int(ref["steps"][i])
        assert core.same_words(got["x_closed"][i, :k + 1], ref["x_closed"][i, :k + 1]), i
        assert core.same_words(got["u_closed"][i, :k], ref["u_closed"][i, :k]) and core.same_words(got["T_closed"][i, :k], ref["T_closed"][i, :k]), i
        n = min(k + 1, S) if ref["flags"][i] == FAILED else k     # a failed step is in status and iters only
        assert np.array_equal(got["status"][i, :n], ref["status"][i, :n]) and np.array_equal(got["iters"][i, :n], ref["iters"][i, :n]), i
        assert np.all(got["sel"][i, :n] == [0, 1, 2])
    assert ref["steps"].max() > 3
    dr.close()
    solver.close()


# ------------------------------------------------------------------------------------------------ 3. a pool no handle fits
# seeds of ``loop_world(seed, 13)``: the first 8 of 0, 1, 2, ... on which every solve of the host loop (host select, host
# solver, host advance; host_loop below) is feasible until the rollout ends.  Left out: 2, 6, 8, 9, 11, 12, 13, 14 -- their routes
# run towards smaller y, where the free-time problem's signed time bound is infeasible at the first step (scenarios.py)
POOL_SEEDS = [0, 1, 3, 4, 5, 7, 10, 15]
K_POOL, N_SEL = 16, 3


def host_step(scene_host, w, x0, u0, xref, variant, pool_b):
    """one step's select and solve on the host builds, for the rollouts whose variant is not 0"""
    B = len(x0)
    s = scene_core.host_select(scene_host, w["pool_A"], pool_b, xref, N_SEL, x0=x0, variant=variant, n_sub=1)
    o = dict(xopt=np.zeros((B, 3, N + 1)), uopt=np.zeros((B, 2, N)), ts_opt=np.zeros(B), status=np.full(B, -5, np.int32),
             iters=np.zeros(B, np.int32))
    on = (variant != 0) & (s["ok"] == 1)
    if on.any():
        r = native_build.lpi_solve(4, N, [4] * N_SEL, x0[on], u0[on], xref[on], s["A"][on], s["b"][on], TS)
        for k in o:
            o[k][on] = r[k]
    return s, o, on


def host_loop(host, scene_host, w, steps=S):
    """the whole loop on the host builds; returns (case, feasible_everywhere [B])"""
    B = len(w["start"])
    c = core.Case(B, K_POOL, 4, N, N_SEL, ROUTE_POINTS, S, n_sub=8, goal_tol2=GOAL_TOL2)
    for k in ("pool_A", "pool_b", "goal", "path", "path_len"):
        c[k][...] = w[k]
    c["x0"][...] = w["start"]
    core.advance(host, c, 0)
    ok = np.ones(B, bool)
    for _ in range(steps):
        s, o, on = host_step(scene_host, w, c["x0"].copy(), c["u0"].copy(), c["xref_out"].copy(), c["variant_out"].copy(), c["pool_b"].copy())
        ok &= ~on | np.isin(o["status"], (0, 1))
        for k in ("xopt", "uopt", "ts_opt", "status", "iters"):
            c[k][...] = o[k]
        c["sel"][...] = s["sel"]
        core.advance(host, c, 1)
    return c, ok


def test_pool_seeds_are_the_feasible_ones(host, scene_host):
    """the recipe behind POOL_SEEDS, on the host builds alone: of the seeds 0 .. 15 the whole host loop is feasible on exactly
    the listed eight, and on those every rollout reaches the goal"""
    c, ok = host_loop(host, scene_host, loop_worlds(list(range(16)), K_POOL - 3))
    assert [s for s in range(16) if ok[s]] == POOL_SEEDS
    assert np.all(c["flags"][POOL_SEEDS] == GOAL) and np.all(c["flags"][~ok] == FAILED)


def test_sixteen_obstacles_three_selected_against_the_host_yardstick(host, scene_host):
    """K = 16, n_sel = 3, static, rounds = 0, step by step: the yardstick -- host select, host solver (native_build.lpi_solve),
    host advance -- is re-seeded from the device's state before every step, so that every comparison is of one step alone.
    The solve at TOL, the selection, the flags, the step counts and variant_out exactly."""
    w = loop_worlds(POOL_SEEDS, K_POOL - 3)
    B = len(POOL_SEEDS)
    with pytest.raises((RuntimeError, IndexError, ValueError)):
        BatchSolver(N, [4] * K_POOL, B)
    solver, lp = make_loop(w, N_SEL, variant=4, n_sub=8)
    c = core.Case(B, K_POOL, 4, N, N_SEL, ROUTE_POINTS, S, n_sub=8, goal_tol2=GOAL_TOL2)
    for k in ("pool_A", "goal", "path", "path_len"):
        c[k][...] = w[k]
    worst = 0.0
    for step in range(S):
        torch.cuda.synchronize()
        st = {k: _np(getattr(lp, k)).copy() for k in ("x0", "u0", "xref", "variant_out", "pool_b", "k", "flags")}
        hist = {k: _np(v).copy() for k, v in lp.hist.items()}
        s, o, on = host_step(scene_host, w, st["x0"], st["u0"], st["xref"], st["variant_out"], st["pool_b"])
        assert np.all(np.isin(o["status"][on], (0, 1))), (step, o["status"])     # the seeds' own condition
        lp.step()
        torch.cuda.synchronize()
        r, sel = lp._last
        assert np.array_equal(_np(sel)[on], s["sel"][on]) and np.array_equal(_np(r.status), o["status"]), step
        for k in ("xopt", "uopt", "ts_opt"):
            diff = np.max(np.abs(_np(getattr(r, k)) - o[k])[on]) if on.any() else 0.0
            worst = max(worst, diff)
            assert diff < TOL, (step, k, diff)
        # the advance on the host from the device's state and the device's solve: flags, counts and variant_out exactly
        for k, name in (("x0", "x0"), ("u0", "u0"), ("pool_b", "pool_b"), ("k", "k"), ("flags", "flags"), ("xref_out", "xref"),
                        ("variant_out", "variant_out")):
            c[k][...] = st[name]
        for k, name in (("x_closed", "x_closed"), ("u_closed", "u_closed"), ("T_closed", "T_closed"), ("status_hist", "status"),
                        ("iters_hist", "iters"), ("clear_hist", "clear"), ("sel_hist", "sel")):
            c[k][...] = hist[name]
        for k in ("xopt", "uopt", "ts_opt", "status", "iters"):
            c[k][...] = _np(getattr(r, k))
        c["sel"][...] = _np(sel)
        core.advance(host, c, 1)
        assert np.array_equal(c["flags"], _np(lp.flags)) and np.array_equal(c["k"], _np(lp.k)), step
        assert np.array_equal(c["variant_out"], _np(lp.variant_out)) and core.same_words(c["xref_out"], _np(lp.xref)), step
        fin = np.isfinite(c["clear_hist"])
        assert core.same_words(c["x0"], _np(lp.x0)) and np.all(np.abs(c["clear_hist"][fin] - _np(lp.hist["clear"])[fin]) < TOL)
    got = read_np(lp)
    print("largest |device - host| of a single solve %.3e; steps %s flags %s" % (worst, got["steps"].tolist(), got["flags"].tolist()))
    assert not (got["flags"] == FAILED).any() and (got["flags"] == GOAL).any()
    solver.close()


# ------------------------------------------------------------------------------------------------ 4. independent audit
def plan_of(x_closed):
    """x_closed [B,S+1,3] read as plans [B,3,S+1]"""
    return torch.as_tensor(x_closed).permute(0, 2, 1).contiguous()


def test_min_clear_is_pool_clearance_of_the_driven_trajectory():
    w = loop_worlds(POOL_SEEDS, K_POOL - 3)
    solver, lp = make_loop(w, N_SEL, variant=4, n_sub=8)
    lp.run()
    got = lp.read()
    _, audit = scene.pool_clearance(plan_of(got["x_closed"]).cuda(), w["pool_A"], w["pool_b"], variant=4, n_sub=8)
    torch.cuda.synchronize()
    mc, audit, flags = _np(got["min_clear"]), _np(audit), _np(got["flags"])
    print("min_clear %s flags %s" % (np.round(mc, 4).tolist(), flags.tolist()))
    assert core.same_words(mc, audit)
    assert (flags == GOAL).any() and np.all(mc[flags == GOAL] >= 0.0)
    solver.close()


# ------------------------------------------------------------------------------------------------ 5. moving pool
def crossing_world(B):
    """a corridor (two walls of 4 rows) with one 2 x 2 box crossing the straight route at 0.25 .. 0.4 m/s, variant 8"""
    om = obstacleModel()
    polys = [[[39, 9], [0, 9], [0, 10], [39, 10], [39, 9]], [[0, 1], [39, 1], [39, 0], [0, 0], [0, 1]]]
    pool_A, pool_b, pool_v = np.zeros((B, 3, 4, 2)), np.zeros((B, 3, 4)), np.zeros((B, 3, 2))
    path = np.zeros((B, 3, ROUTE_POINTS))
    for i in range(B):
        box = rectangle_vertices(12.0 + 0.5 * i, 1.5 if i % 2 == 0 else 8.5, 0.0, 2.0, 2.0)
        A, b = om.obstacle_H_Represent(3, [5, 5, 5], polys + [box])
        pool_A[i], pool_b[i] = A.reshape(3, 4, 2), b[:, 0].reshape(3, 4)
        pool_v[i, 2] = (0.0, (0.25 + 0.05 * (i % 4)) * (1 if i % 2 == 0 else -1))
        path[i, 0], path[i, 1] = 4.0 + 0.6 * np.arange(ROUTE_POINTS), 5.0
    return dict(pool_A=pool_A, pool_b=pool_b, pool_v=pool_v, start=path[:, :, 0].copy(), goal=path[:, :2, -1].copy(), path=path,
                path_len=np.full(B, ROUTE_POINTS, np.int32))


def test_moving_pool_accumulates_and_measures_the_interval():
    B, n_sub = 6, 8
    w = crossing_world(B)
    solver, lp = make_loop(w, 3, Ts=1.5, n_sub=n_sub)      # 0.6 m between route points at 0.4 m/s
    assert lp.variant == 8
    lp.run()
    got = read_np(lp)
    print("steps %s flags %s min_clear %s" % (got["steps"].tolist(), got["flags"].tolist(), np.round(got["min_clear"], 3).tolist()))
    assert got["steps"].max() >= 3
    rows = [w["pool_b"].copy()]                                   # the pool before every step, numpy's accumulation
    for k in range(S):
        nxt = rows[-1].copy()
        for i in range(B):
            if k < got["steps"][i]:
                nxt[i] = core.ref_move(w["pool_A"][i], rows[-1][i], w["pool_v"][i], got["T_closed"][i, k])
        rows.append(nxt)
    assert core.same_words(got["pool_b"], rows[-1])
    for k in range(int(got["steps"].max())):
        live = np.flatnonzero(got["steps"] > k)
        x = torch.as_tensor(got["x_closed"][live, k:k + 2]).permute(0, 2, 1).contiguous().cuda()
        _, c = scene.pool_clearance(x, w["pool_A"][live], rows[k][live], pool_v=w["pool_v"][live], Ts=got["T_closed"][live, k],
                                    variant=8, n_sub=n_sub)
        assert core.same_words(_np(c), got["clear"][live, k]), k
    assert np.all(np.isinf(got["clear"][np.arange(S)[None, :] >= got["steps"][:, None]]))
    solver.close()


# ------------------------------------------------------------------------------------------------ 6. collision stop
def test_collision_stop_cuts_the_unstopped_history():
    w = loop_worlds(POOL_SEEDS, K_POOL - 3)
    solver, lp = make_loop(w, N_SEL, variant=4, n_sub=8)
    free = read_np(lp.run())
    thr = float(np.median(free["min_clear"]))
    lp2 = scene.PoolLoop(solver, w["pool_A"], w["pool_b"], w["start"], w["goal"], w["path"], w["path_len"], TS, variant=4, n_sub=8,
                         max_steps=S, goal_tol2=GOAL_TOL2, clearance=thr)
    got = read_np(lp2.run())
    below = free["clear"] < thr
    stopped = 0
    for i in range(len(POOL_SEEDS)):
        if not below[i].any():
            for k in HISTORY + ("steps", "flags"):
                assert core.same_words(got[k][i], free[k][i]), (i, k)
            continue
        first = int(np.argmax(below[i]))
        stopped += 1
        assert got["flags"][i] == COLLISION and got["steps"][i] == first + 1
        for k in HISTORY:
            n = first + 2 if k == "x_closed" else first + 1
            assert core.same_words(got[k][i, :n], free[k][i, :n]), (i, k)
        assert np.all(np.isinf(got["clear"][i, first + 1:])) and np.all(got["T_closed"][i, first + 1:] == 0.0)
        assert np.all(np.isnan(got["x_closed"][i, first + 2:])) and np.all(got["sel"][i, first + 1:] == -1)
    print("threshold %.4f stops %d of %d" % (thr, stopped, len(POOL_SEEDS)))
    assert stopped >= 1
    solver.close()


# ------------------------------------------------------------------------------------------------ 7. drive_maps
from tests.test_gpu_grid_pool import GOAL_CELL, GOAL_POSE, START_CELL, START_POSE, world  # noqa: E402

MAP_SEEDS = [0, 1, 2, 3, 4, 5]


def test_drive_maps_is_its_hand_composition_and_masks_what_it_cannot_drive():
    grids = np.stack([world(s) for s in MAP_SEEDS])
    blocked = world(MAP_SEEDS[0])
    blocked[1:10, 10:12] = 1
    dense = (np.random.default_rng(18).random((11, 40)) < 0.5).astype(np.uint8)
    dense[START_CELL], dense[GOAL_CELL] = 0, 0
    grids8 = np.concatenate([grids, blocked[None], dense[None]])
    K = 16
    solver = BatchSolver(N, [4] * N_SEL, len(grids8))
    kw = dict(variant=4, max_steps=S, n_sub=8)

    def run(g):
        n = len(g)
        cells = lambda c: np.tile(np.array(c, np.int32), (n, 1))
        lp, info = scene.drive_maps(solver, g, cells(START_CELL), cells(GOAL_CELL), np.tile(START_POSE, (n, 1)), np.tile(GOAL_POSE, (n, 1)),
                                    TS, K, pad=0.5, dilation=1, **kw)
        return read_np(lp), {k: _np(v) for k, v in info.items() if k != "pool"}
    got, info = run(grids8)
    print("steps %s flags %s source %s pool_ok %s" % (got["steps"].tolist(), got["flags"].tolist(), info["source"].tolist(), info["pool_ok"].tolist()))
    # by hand
    n = len(grids8)
    cells = lambda c: np.tile(np.array(c, np.int32), (n, 1))
    g = torch.as_tensor(grids8, device="cuda")
    pool = scene.grid_pool(g, K, pad=0.5, far=100.0)
    path, plen, src = route_search(g, cells(START_CELL), cells(GOAL_CELL), dilation=1)
    plen = torch.where((pool["ok"] != 0) & (plen >= 1), plen, 0).to(torch.int32)
    lp = scene.PoolLoop(solver, pool["pool_A"], pool["pool_b"], np.tile(START_POSE, (n, 1)), np.tile(GOAL_POSE, (n, 1)), path, plen, TS,
                        **kw).run()
    hand = read_np(lp)
    for k in hand:
        assert core.same_words(got[k], hand[k]), k
    assert info["source"][6] == 0 and info["pool_ok"][6] == 1 and info["pool_ok"][7] == 0
    for i in (6, 7):
        assert got["flags"][i] == FAILED and got["steps"][i] == 0 and info["path_len"][i] == 0
        assert np.all(got["status"][i] == 0) and np.all(got["sel"][i] == -1) and np.all(np.isnan(got["x_closed"][i, 1:]))
    assert np.all(info["source"][:6] != 0) and np.all(info["pool_ok"][:6] == 1) and (got["steps"][:6] > 0).sum() >= 3
    # the masked worlds do not disturb the others: the six alone give the same words
    alone, _ = run(grids)
    for k in alone:
        assert core.same_words(alone[k], got[k][:6]), k
    solver.close()


# ------------------------------------------------------------------------------------------------ 8. run, reset, streams, rounds
def test_run_is_steps_and_reset_reproduces():
    w = loop_worlds(POOL_SEEDS, K_POOL - 3)
    solver, lp = make_loop(w, N_SEL, variant=4, n_sub=8)
    whole = read_np(lp.run(7))
    lp.reset()
    fresh = read_np(lp)
    assert np.all(fresh["steps"] == 0) and np.all(np.isnan(fresh["x_closed"][:, 1:])) and same(fresh["pool_b"], w["pool_b"])
    for _ in range(7):
        lp.step()
    stepped = read_np(lp)
    for k in whole:
        assert core.same_words(whole[k], stepped[k]), k
    assert lp.steps_enqueued == 7 and whole["steps"].max() == 7
    solver.close()


def test_run_on_a_side_stream_with_its_inputs_dropped():
    w = loop_worlds(POOL_SEEDS, K_POOL - 3)
    solver, lp = make_loop(w, N_SEL, variant=4, n_sub=8)
    ref = read_np(lp.run())
    ins = {k: torch.as_tensor(v, device="cuda") for k, v in w.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lp2 = scene.PoolLoop(solver, ins["pool_A"], ins["pool_b"], ins["start"], ins["goal"], ins["path"], ins["path_len"], TS,
                             variant=4, n_sub=8, max_steps=S, goal_tol2=GOAL_TOL2).run()
    del ins
    junk = [torch.full((len(POOL_SEEDS), K_POOL, 4, 2), 7.0, dtype=torch.float64, device="cuda") for _ in range(16)]
    torch.cuda.synchronize()
    del junk
    got = read_np(lp2)
    for k in ref:
        assert core.same_words(got[k], ref[k]), k
    solver.close()


def test_one_round_is_the_hand_composition_with_solve_scene():
    w = loop_worlds(POOL_SEEDS, K_POOL - 3)
    solver, lp = make_loop(w, N_SEL, variant=4, n_sub=8, rounds=1)
    lp.run(4)
    got = read_np(lp)
    _, hand = make_loop(w, N_SEL, variant=4, n_sub=8, rounds=1)
    for _ in range(4):
        r, info = scene.solve_scene(hand.solver, hand.variant_out, hand.x0, hand.u0, hand.xref, hand.pool_A, hand.pool_b, hand.Ts,
                                    term=hand.term, params=SolverParams(), rounds=1, n_sub=8)
        d = hand._desc
        for name, t in (("status", r.status), ("iters", r.iters), ("ts_opt", r.ts_opt), ("xopt", r.xopt), ("uopt", r.uopt),
                        ("sel", info["sel"])):
            setattr(d, name, t.data_ptr())
        hand._advance(1)
        torch.cuda.synchronize()
    ref = read_np(hand)
    for k in ref:
        assert core.same_words(got[k], ref[k]), k
    assert got["steps"].max() == 4
    solver.close()
    hand.solver.close()
