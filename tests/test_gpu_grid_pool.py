"""GPU tier of the grid-to-pool cover (obca_grid_pool through the C ABI, scene.grid_pool, scene.solve_maps).

1. The kernel against the host build of the same core (tests/test_grid_pool_core.py pins that one to a numpy restatement of
   the serial definition): rect, count and ok exactly, pool_A and pool_b bit for bit, at every shape where the kernel takes
   another path (a word boundary, a chunk of 64 rows), every pattern, different maps in one launch, sentinels around every
   output.
2. The round trip on the device: planner.rasterise_batch of the pad = 0 boxes gives the grid back.
3. Refused calls launch nothing.
4. grid_pool on a side stream with its inputs dropped right after the call.
5. Map to plan: scene.solve_maps against the same recipe on the host (host cover, Python A* on model_map.dilate_map's grid,
   the host builds of the route, scene and solver cores)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import native_build
from tests import test_grid_pool_core as core
from tests import test_route_core as route_core
from tests import test_scene_core as scene_core
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib, planner, scene
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.a_star import a_star
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.model_map import dilate_map
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams

pytestmark = pytest.mark.gpu
TOL = 1e-9                        # tests/test_gpu_scene.py: TOL
PAD = 32                          # sentinel words on either side of every output
E_INVAL = -22


@pytest.fixture(scope="module")
def host():
    return core.load_host()


def _np(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _guarded(B, K):
    """every output in the middle of a buffer of sentinels: name -> (buffer, view of the output, fill)"""
    out = {}
    for name, (shape, dt, fill) in core.out_shapes(B, K).items():
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), fill, dtype=torch.float64 if dt == np.float64 else torch.int32, device="cuda")
        out[name] = (buf, buf[PAD:PAD + n].view(*shape), fill)
    return out


def device_pool(grids, K, res=1.0, pad=0.5, far=100.0, rc=0, null=(), over=None, shift_A=0):
    """obca_grid_pool itself on guarded outputs: numpy in, numpy out.  A refused call (rc != 0) must leave every buffer as it
    was, an accepted one the sentinels.  ``shift_A``: pool_A handed over that many bytes further on"""
    g = torch.as_tensor(np.ascontiguousarray(grids, np.uint8), device="cuda")
    B, rows, cols = g.shape
    o = _guarded(B, K)
    a = {k: _ptr(v[1]) for k, v in o.items()}
    a["grid"] = _ptr(g)
    if shift_A:
        a["pool_A"] = ctypes.c_void_p(o["pool_A"][1].data_ptr() + shift_A)
    for k in null:
        a[k] = None
    s = dict(B=B, rows=rows, cols=cols, K=K)
    s.update(over or {})
    got = _lib.load().obca_grid_pool(a["grid"], s["B"], s["rows"], s["cols"], s["K"], res, pad, far, a["pool_A"], a["pool_b"], a["rect"],
                                     a["count"], a["ok"], torch.cuda.current_device(), _lib.stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    assert got == rc
    for name, (buf, view, fill) in o.items():
        if rc != 0:
            assert (buf == fill).all(), name
        else:
            assert (buf[:PAD] == fill).all() and (buf[-PAD:] == fill).all(), name
    return {k: _np(v[1]) for k, v in o.items()}


def assert_same(dev, ref):
    for k in ("rect", "count", "ok"):
        assert np.array_equal(dev[k], ref[k]), k
    for k in ("pool_A", "pool_b"):
        assert np.array_equal(core.words(dev[k]), core.words(ref[k])), k


# ------------------------------------------------------------------------------------------------ 1. kernel = host core
@pytest.mark.parametrize("shape", core.GPU_SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_host_core(host, shape):
    """every pattern of tests/test_grid_pool_core.py (its four additions included: the run over columns 60..70, the rectangle
    100 rows tall, the column that splits a later run, the run to the last column) as the maps of one launch: B = 1 (the
    checkerboard), B = 5 and B = 67 (the patterns in turn, random maps of other seeds after the first round), K = 1, 3 and 64;
    resolution 0.3 with pad 0.1 once, where a fused c res - pad would be another word"""
    rows, cols = shape
    pats = list(patterns_in_turn(rows, cols, 67))
    for lo, B, K, res, pad in ((2, 1, 64, 1.0, 0.5), (4, 5, 3, 1.0, 0.0), (0, 67, 64, 0.3, 0.1), (0, 67, 1, 1.0, 0.5), (9, 5, 64, 1.0, 0.5)):
        grids = np.stack(pats[lo:lo + B])
        ref = core.host_pool(host, grids, K, res=res, pad=pad)
        dev = device_pool(grids, K, res=res, pad=pad)
        assert_same(dev, ref)
        assert not np.isnan(dev["pool_A"]).any() and not np.isnan(dev["pool_b"]).any()


def patterns_in_turn(rows, cols, n):
    """n maps: the patterns of the shape, again and again with other seeds for the random ones"""
    out, seed = [], 0
    while len(out) < n:
        out += list(core.patterns(rows, cols, seed).values())
        seed += 1
    return out[:n]


def test_rect_may_be_null(host):
    grids = np.stack(list(core.patterns(11, 40).values()))
    ref = core.host_pool(host, grids, 8)
    dev = device_pool(grids, 8, null=("rect",))
    for k in ("pool_A", "pool_b", "count", "ok"):
        assert np.array_equal(dev[k], ref[k]), k
    assert np.all(dev["rect"] == core.FILL_I)


# ------------------------------------------------------------------------------------------------ 2. round trip
# seeds of np.random.default_rng(seed).random((11, 40)) < 0.3.  A random map of this density has 62 to 101 rectangles (median
# 82 over seeds 0 .. 3999), so K = 64 covers few of them: the first 13 seeds are the first of 0, 1, 2, ... whose cover has at
# most 64 (found with the host core), the last 3 are ordinary ones that overflow.  3 of 16 excluded, at most a quarter.
ROUND_TRIP_SEEDS = [213, 838, 2001, 8582, 13358, 16183, 18628, 19841, 20137, 23925, 34735, 41956, 42443, 0, 1, 2]
ROUND_TRIP_OVERFLOW = 3


def test_round_trip_on_the_device(host):
    """the pad = 0 boxes of the cover, downloaded as polygons, through planner.rasterise_batch at resolution 1: the input grid"""
    grids = np.stack([(np.random.default_rng(s).random((11, 40)) < 0.3).astype(np.uint8) for s in ROUND_TRIP_SEEDS])
    B = len(grids)
    href = core.host_pool(host, grids, 64, pad=0.0)
    excluded = int((href["ok"] == 0).sum())
    assert excluded == ROUND_TRIP_OVERFLOW and 4 * excluded <= B
    pool = scene.grid_pool(grids, 64, resolution=1.0, pad=0.0)
    torch.cuda.synchronize()
    ok, count, b = _np(pool["ok"]), _np(pool["count"]), _np(pool["pool_b"])
    assert np.array_equal(ok, href["ok"]) and np.array_equal(count, href["count"])
    print("round trip: %d of %d maps excluded (count %s)" % (excluded, B, count.tolist()))
    keep = np.flatnonzero(ok == 1)
    polys = [[[[-b[i, k, 3], -b[i, k, 2]], [b[i, k, 1], b[i, k, 0]]] for k in range(count[i])] for i in keep]
    back = planner.rasterise_batch(polys, (40, 11), resolution=1.0)
    torch.cuda.synchronize()
    assert np.array_equal(_np(back), grids[keep])


# ------------------------------------------------------------------------------------------------ 3. refusals
REFUSED = [dict(over=dict(K=65)), dict(over=dict(rows=4097, cols=1)), dict(pad=-0.5), dict(far=float("inf")), dict(far=float("nan")),
           dict(null=("grid",)), dict(null=("pool_b",)), dict(null=("count",)), dict(shift_A=8), dict(over=dict(B=0)), dict(res=0.0)]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: repr(c).replace(" ", ""))
def test_refused_calls_launch_nothing(case):
    """OBCA_E_INVAL, and every output buffer -- guard bands and the middle -- as it was"""
    grids = core.patterns(4, 9)["checkerboard"][None].repeat(2, 0)
    device_pool(grids, 6, rc=E_INVAL, **case)


def test_refused_calls_raise_from_python():
    g = core.patterns(4, 9)["checkerboard"][None]
    for kw in (dict(K=65), dict(K=0), dict(K=4, pad=-1.0), dict(K=4, far=float("nan")), dict(K=4, resolution=0.0)):
        with pytest.raises(RuntimeError, match="code -22"):
            scene.grid_pool(g, **kw)
    with pytest.raises(RuntimeError, match="code -22"):
        scene.grid_pool(np.zeros((1, 4097, 1), np.uint8), 4)
    with pytest.raises(ValueError):
        scene.grid_pool(g[0], 4)


# ------------------------------------------------------------------------------------------------ 4. side stream
def test_grid_pool_on_a_side_stream_with_its_inputs_dropped(host):
    """the launch is asynchronous: grid_pool ties the grid to its result and records it on the stream, so a caller may drop it
    right after the call, on a stream that is not the default one"""
    rows, cols, K = 130, 70, 64
    grids = np.stack(patterns_in_turn(rows, cols, 257))
    ref = core.host_pool(host, grids, K)
    g = torch.as_tensor(grids, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = scene.grid_pool(g, K)
    del g
    junk = [torch.full((257, rows, cols), 1, dtype=torch.uint8, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    del junk
    assert_same({k: _np(v) for k, v in got.items()}, ref)


# ------------------------------------------------------------------------------------------------ 5. map to plan
N_PLAN, TS, K_PLAN, N_SEL, N_SUB, ROUNDS = 10, 0.1, 16, 4, 16, 2
START_CELL, GOAL_CELL, START_POSE, GOAL_POSE = (5, 3), (5, 23), (3.0, 5.0, 0.0), (23.0, 5.0, 0.0)
# seeds of ``world``: the first 16 of 0, 1, 2, ... on which the host yardstick below is feasible (it is not on seed 10)
WORLD_SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16]


def world(seed):
    """11 x 40, rows 0 and 10 occupied, two boxes of height 1..2 and width 1..3 cells, top row in [1, 10 - h], left column
    in [7, 20 - w]"""
    rng = np.random.default_rng(seed)
    g = np.zeros((11, 40), np.uint8)
    g[0] = g[10] = 1
    for _ in range(2):
        h, w = int(rng.integers(1, 3)), int(rng.integers(1, 4))
        r, c = int(rng.integers(1, 10 - h + 1)), int(rng.integers(7, 20 - w + 1))
        g[r:r + h, c:c + w] = 1
    return g


def _host_route(grid, start_cell, goal_cell):
    """the Python mirror's route [3,L] on one grid, or None (tests/test_gpu_route.py: _host_route)"""
    pl = a_star(grid, tuple(start_cell), tuple(goal_cell))
    chain = pl.solve(grid, tuple(start_cell), tuple(goal_cell))
    if chain is False or len(chain) < 2:
        return None
    return np.asarray(pl.create_reference_path(pl.rebuild_path(chain)), float).T


def host_references(grids, dilation=1):
    """route_references' recipe on the host: the dilated route where there is one, else the plain one; (xref, source)"""
    B = len(grids)
    routes, source = [], []
    for g in grids:
        r = _host_route(dilate_map(g, dilation), START_CELL, GOAL_CELL)
        src = 2
        if r is None:
            r, src = _host_route(g, START_CELL, GOAL_CELL), 1
        routes.append(r)
        source.append(src if r is not None else 0)
    P = max([r.shape[1] for r in routes if r is not None] + [2])
    path, plen = route_core.pack([r if r is not None else np.zeros((3, 1)) for r in routes], P)
    plen = np.where([r is None for r in routes], -1, plen).astype(np.int32)
    start, goal = np.tile(START_POSE, (B, 1)), np.tile(GOAL_POSE, (B, 1))
    o = route_core.host_resample(route_core.load_host(), path, plen, N_PLAN, start, goal)
    return o["xref"], np.array(source, np.int32)


def host_solve_maps(grids):
    """scene.solve_maps' recipe on the host for worlds that have a pool and a route: host cover (pad 0.5, far 100), host
    references, then solve_scene's loop -- select from the reference and x0, solve (native_build.lpi_solve, obca_mpc4), measure
    the plan against the whole pool, re-select, re-solve where the selection changed, hold the clearer plan.  Returns
    (feasible [B], xopt [B,3,N+1])"""
    B, m = len(grids), [4] * N_SEL
    pool = core.host_pool(core.load_host(), grids, K_PLAN, pad=0.5, far=100.0)
    xref, source = host_references(grids)
    assert np.all(pool["ok"] == 1) and np.all(source != 0)
    sh = scene_core.load_host()
    pA, pb = pool["pool_A"].copy(), pool["pool_b"].copy()
    start, u0, var = np.tile(START_POSE, (B, 1)), np.zeros((B, 2)), np.full(B, 4, np.int32)
    kw = dict(n_sub=N_SUB)

    def solve(which, A, b):
        """lpi_solve on the instances ``which``; the others skipped (status -5, plan of zeros)"""
        x, st = np.zeros((B, 3, N_PLAN + 1)), np.full(B, -5, np.int32)
        if which.any():
            o = native_build.lpi_solve(4, N_PLAN, m, start[which], u0[which], xref[which], A[which], b[which], TS)
            x[which], st[which] = o["xopt"], o["status"]
        return x, st

    s0 = scene_core.host_select(sh, pA, pb, xref, N_SEL, x0=start, variant=var, **kw)
    score, sel = s0["score"].copy(), s0["sel"].copy()
    held_x, held_st = solve(np.ones(B, bool), s0["A"], s0["b"])
    t = scene_core.host_select(sh, pA, pb, held_x, N_SEL, variant=var, status=held_st, state=(score, sel), **kw)
    score, sel, min_clear, v = t["score"].copy(), t["sel"].copy(), t["min_clear"].copy(), t["variant_out"].copy()
    for _ in range(ROUNDS):
        cur_x, cur_st = solve(v != 0, t["A"], t["b"])
        t = scene_core.host_select(sh, pA, pb, cur_x, N_SEL, variant=v, status=cur_st, state=(score, sel), **kw)
        score, sel = t["score"].copy(), t["sel"].copy()
        with np.errstate(invalid="ignore"):
            better = t["min_clear"] > min_clear
        held_x[better], held_st[better], min_clear[better] = cur_x[better], cur_st[better], t["min_clear"][better]
        v = t["variant_out"].copy()
    return np.isin(held_st, (0, 1)), held_x


def test_map_to_plan():
    """16 worlds (WORLD_SEEDS), a 17th whose corridor a full-height box blocks and an 18th of density 0.5 that overflows
    K = 16.  N = 10, Ts = 0.1, obca_mpc4, n_sel = 4, K = 16, pad = 0.5, dilation = 1.  The test prints what it observes."""
    grids = np.stack([world(s) for s in WORLD_SEEDS])
    yfeas, _ = host_solve_maps(grids)
    print("host yardstick feasible on %d of %d" % (yfeas.sum(), len(grids)))
    assert yfeas.all()                                           # the seeds' own condition
    blocked = world(WORLD_SEEDS[0])
    blocked[1:10, 10:12] = 1
    dense = (np.random.default_rng(18).random((11, 40)) < 0.5).astype(np.uint8)
    dense[START_CELL], dense[GOAL_CELL] = 0, 0
    grids18 = np.concatenate([grids, blocked[None], dense[None]])
    B = len(grids18)
    solver = BatchSolver(N_PLAN, [4] * N_SEL, B)

    def run(g):
        n = len(g)
        cells = lambda c: np.tile(np.array(c, np.int32), (n, 1))
        res, info = scene.solve_maps(solver, g, cells(START_CELL), cells(GOAL_CELL), np.tile(START_POSE, (n, 1)), np.tile(GOAL_POSE, (n, 1)),
                                     TS, K_PLAN, pad=0.5, dilation=1, variant=4, rounds=ROUNDS, n_sub=N_SUB)
        torch.cuda.synchronize()
        return res, info
    res, info = run(grids18)
    feas, status = _np(res.feas), _np(res.status)
    source, pool_ok, count = _np(info["source"]), _np(info["pool_ok"]), _np(info["pool"]["count"])
    print("solve_maps feasible %s, source %s, pool_ok %s, count %s, rounds used %s" %
          (feas.astype(int).tolist(), source.tolist(), pool_ok.tolist(), count.tolist(), _np(info["rounds_used"]).tolist()))
    assert np.all(feas[:16][yfeas])                              # (a)
    pA, pb = info["pool"]["pool_A"], info["pool"]["pool_b"]
    _, knots = scene.pool_clearance(res.xopt, pA, pb, variant=4, n_sub=1)
    knots = _np(knots)
    print("smallest knot clearance against the whole pool %.9f" % knots[feas].min())
    assert np.all(knots[feas] >= SolverParams().dmin - 1e-6)     # (b)
    _, fresh = scene.pool_clearance(res.xopt, pA, pb, variant=4, n_sub=N_SUB)
    mc, fresh = _np(info["min_clear"]), _np(fresh)
    print("largest |min_clear - pool_clearance| %.3e" % np.max(np.abs(mc - fresh)[feas]))
    assert not np.isnan(mc[feas]).any() and np.all(np.abs(mc - fresh)[feas] < TOL)       # (c)
    # (d) the blocked corridor: no route, masked
    assert source[16] == 0 and pool_ok[16] == 1 and status[16] == _lib.STATUS_SKIPPED and not feas[16] and np.isnan(mc[16])
    assert np.all(source[:16] != 0) and np.all(pool_ok[:16] == 1)
    # (e) the dense map: the pool overflows, reported and masked
    assert pool_ok[17] == 0 and count[17] > K_PLAN and status[17] == _lib.STATUS_SKIPPED and not feas[17]
    assert _np(info["rounds_used"])[16:].tolist() == [0, 0]
    # ... and neither disturbs the others: the 16 worlds alone give the same words
    res16, info16 = run(grids)
    for k in ("xopt", "uopt", "ts_opt", "status", "iters"):
        assert np.array_equal(_np(getattr(res16, k)), _np(getattr(res, k))[:16], equal_nan=True), k
    assert np.array_equal(_np(info16["min_clear"]), mc[:16], equal_nan=True)
    assert np.array_equal(_np(info16["xref"]), _np(info["xref"])[:16])
    solver.close()
