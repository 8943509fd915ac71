"""Scene pools: a world holds up to 64 obstacles per instance, a solve sees the few its plan comes near.

``select`` (obca_scene_select, arithmetic in csrc/obca_scene_core.h) scores every obstacle of a pool by its smallest signed
distance to a set of poses, takes the ``n_sel`` nearest and gathers their rows for ``BatchSolver.solve``; called again with the
state it returned and the plans solved against that selection, it keeps a running minimum per obstacle and says which
instances' selections changed.  ``pool_clearance`` is the same measurement as an audit of plans against whole pools -- the
one that is not bound to OBCA_MAX_OBST obstacles.  ``solve_scene`` is the loop: select from the reference, solve, measure
the plans against the whole pool, re-select, solve again where the selection changed.  No solver kernel is involved beyond
being called with other rows.

``grid_pool`` (obca_grid_pool, arithmetic in csrc/obca_gridpool_core.h) is the producer of pools on the device: it covers
every occupancy grid of a batch with disjoint axis-parallel rectangles, one pool obstacle each.  ``solve_maps`` composes it
with ``openloop.route_references`` and ``solve_scene``: B maps and B start/goal pairs in, B plans out, each measured against
its whole map.
"""
import ctypes

from . import _lib
from .solver import DEFAULT_EGO, SolverParams


def _dev_of(device, *tensors):
    import torch
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def select(pool_A, pool_b, x, n_sel, pool_v=None, Ts=None, x0=None, variant=None, status=None, n_sub=1, state=None,
           ego=DEFAULT_EGO, device=None):
    """pool_A [B,K,E,2], pool_b [B,K,E] (K <= 64 obstacles of E rows each), pool_v [B,K,2] m/s or None, Ts [B] or a float
    (needed with pool_v); x [B,3,N+1] the poses to measure (a reference window, or plans), x0 [B,3] or None one more pose
    against stage 0's rows; variant [B], an int or None (4: every sample against stage 0's rows), status [B] or None.

    ``state=None``: scores are written from the samples and every usable instance counts as changed.  ``state`` = the dict a
    previous call returned: its ``score`` and ``sel`` are updated IN PLACE to the running minimum and the new selection, and
    only instances with variant != 0 and status 0 / 1 are measured.

    Returns a dict of device tensors on the current stream, no host synchronisation: A [B,N+1,n_sel E,2] and b [B,N+1,n_sel E]
    (rows for a handle with m = [E] * n_sel), sel [B,n_sel] int32 ascending pool indices, variant_out [B] (variant where the
    selection changed, else 0), ok [B] (0: unusable pool or poses, filled rows a = (1, 0), b = -1e6), score [B,K] (NaN where
    never written) and min_clear [B] (this call's smallest distance over the whole pool, NaN where not measured)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("scene.select needs a ROCm GPU; there is no CPU fallback on the product path")
    dev = _dev_of(device, x, pool_A)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=dev).contiguous()
    pool_A, pool_b, x = t(pool_A), t(pool_b), t(x)
    if pool_A.dim() != 4 or pool_b.dim() != 3 or x.dim() != 3:
        raise ValueError("expected pool_A [B,K,E,2], pool_b [B,K,E], x [B,3,N+1]")
    B, K, E = (int(v) for v in pool_b.shape)
    N1, n_sel = int(x.shape[2]), int(n_sel)
    if tuple(pool_A.shape) != (B, K, E, 2) or tuple(x.shape) != (B, 3, N1):
        raise ValueError("expected pool_A [B,K,E,2], pool_b [B,K,E], x [B,3,N+1], got %s, %s, %s" %
                         (tuple(pool_A.shape), tuple(pool_b.shape), tuple(x.shape)))

    def opt(a, shape, dt=torch.float64):
        if a is None:
            return None
        a = torch.as_tensor(a, dtype=dt, device=dev)
        a = a.expand(shape).contiguous() if a.dim() == 0 else a.contiguous()
        if tuple(a.shape) != shape:
            raise ValueError("expected shape %s, got %s" % (shape, tuple(a.shape)))
        return a
    pool_v, Ts, x0 = opt(pool_v, (B, K, 2)), opt(Ts, (B,)), opt(x0, (B, 3))
    variant, status = opt(variant, (B,), torch.int32), opt(status, (B,), torch.int32)
    if state is None:
        score = torch.full((B, K), float("nan"), dtype=torch.float64, device=dev)
        sel = torch.zeros(B, max(n_sel, 0), dtype=torch.int32, device=dev)
    else:
        score, sel = state["score"], state["sel"]
        for a, shape, dt in ((score, (B, K), torch.float64), (sel, (B, n_sel), torch.int32)):
            if not (isinstance(a, torch.Tensor) and a.device == dev and a.dtype == dt and a.is_contiguous() and
                    tuple(a.shape) == shape):
                raise ValueError("state: expected contiguous device tensors score [B,K] float64 and sel [B,n_sel] int32")
    rows = max(n_sel, 0) * E
    out = {"A": torch.empty(B, N1, rows, 2, dtype=torch.float64, device=dev),
           "b": torch.empty(B, N1, rows, dtype=torch.float64, device=dev),
           "sel": sel, "score": score,
           "variant_out": torch.empty(B, dtype=torch.int32, device=dev),
           "ok": torch.empty(B, dtype=torch.int32, device=dev),
           "min_clear": torch.empty(B, dtype=torch.float64, device=dev)}
    ego_c = (ctypes.c_double * 4)(*[float(v) for v in ego])
    p = _lib.ptr
    _lib.check(_lib.load().obca_scene_select(ego_c, B, K, E, N1 - 1, n_sel, int(n_sub), 0 if state is None else 1, p(pool_A),
                                             p(pool_b), p(pool_v), p(Ts), p(x), p(x0), p(variant), p(status), p(score), p(sel),
                                             p(out["A"]), p(out["b"]), p(out["variant_out"]), p(out["ok"]), p(out["min_clear"]),
                                             _lib.device_index(dev), _lib.stream_ptr(dev)))
    # the launch is asynchronous: the tensors it reads are tied to the result and to the stream (see openloop.route_reference)
    out["A"]._obca_keep = (pool_A, pool_b, pool_v, Ts, x, x0, variant, status)
    for a in out["A"]._obca_keep:
        if a is not None:
            a.record_stream(torch.cuda.current_stream(dev))
    return out


def pool_clearance(x, pool_A, pool_b, pool_v=None, Ts=None, variant=None, n_sub=1, ego=DEFAULT_EGO, device=None):
    """Plans x [B,3,N+1] against whole pools (``select``'s pool arguments): returns device tensors (per_obstacle [B,K],
    min_clear [B]), the smallest signed distance of every plan to every obstacle of its pool over the knots and, with
    n_sub > 1, obca_plan_sweep's samples between them, and its minimum over the pool.  NaN for an unusable instance."""
    s = select(pool_A, pool_b, x, 1, pool_v=pool_v, Ts=Ts, variant=variant, n_sub=n_sub, ego=ego, device=device)
    return s["score"], s["min_clear"]


def solve_scene(solver, variant, x0, u0, xref, pool_A, pool_b, Ts, pool_v=None, term=None, params=None, rounds=2, n_sub=16,
                target=0.0, ego=DEFAULT_EGO):
    """``solver.solve`` against the ``n_sel = len(solver.m)`` obstacles of each instance's pool that matter.

    Round 0 selects from the reference window ``xref`` and the pose ``x0`` and solves every instance.  Every later round
    measures the last plans against the WHOLE pool (n_sub + 1 samples per interval), re-selects on the running minimum of
    every obstacle's distance, and solves only the instances whose selection changed.  One plan per instance is held: round
    0's, replaced by a later one only if that is feasible and its clearance against the whole pool is larger.  The last
    solve is measured too.  ``solver`` must have m == [E] * n_sel.

    Runs on the current stream without host synchronisation.  Returns (result, info): the held ``BatchResult`` (``iters``
    summed over the rounds; with rounds = 0 exactly ``solver.solve``'s words on the selected rows) and a dict of device
    tensors: clear [B] bool (the held plan measures >= target against the whole pool), min_clear [B] and min_clear_first [B]
    (the held plan's and round 0's; NaN where there is no feasible plan), rounds_used [B] (re-solves of the instance),
    sel [B,n_sel], A_used [B,N+1,M,2] and b_used [B,N+1,M] (the selection and rows the held plan was solved with)."""
    import torch
    params = params or SolverParams()
    dev, N, M, m = solver.device, solver.N, solver.M, solver.m
    pool_A = torch.as_tensor(pool_A, dtype=torch.float64, device=dev).contiguous()
    pool_b = torch.as_tensor(pool_b, dtype=torch.float64, device=dev).contiguous()
    if pool_A.dim() != 4 or pool_b.dim() != 3 or tuple(pool_A.shape) != tuple(pool_b.shape) + (2,):
        raise ValueError("expected pool_A [B,K,E,2], pool_b [B,K,E]")
    B, K, E = (int(v) for v in pool_b.shape)
    n_sel = len(m)
    if m != [E] * n_sel or n_sel > K:
        raise ValueError("solver.m = %s does not fit a pool of %d obstacles of %d rows: expected [%d] * n_sel, n_sel <= %d" %
                         (m, K, E, E, K))
    if isinstance(variant, int):
        variant = torch.full((B,), variant, dtype=torch.int32, device=dev)
    on_dev = lambda t, shape, dt=torch.float64: solver._dev(t, shape, dt)
    variant = on_dev(variant, (B,), torch.int32)
    x0, u0, xref = on_dev(x0, (B, 3)), on_dev(u0, (B, 2)), on_dev(xref, (B, 3, N + 1))
    Ts = on_dev(torch.as_tensor(Ts, dtype=torch.float64).expand(B) if torch.as_tensor(Ts).dim() == 0 else Ts, (B,))
    term = on_dev(torch.zeros(B, 3) if term is None else term, (B, 3))
    if pool_v is not None:
        pool_v = on_dev(pool_v, (B, K, 2))
    cp = params.to_c() if isinstance(params, SolverParams) else params
    kw = dict(pool_v=pool_v, Ts=Ts, n_sub=n_sub, ego=ego, device=dev)

    state = select(pool_A, pool_b, xref, n_sel, x0=x0, variant=variant, **kw)
    A_held, b_held, sel_held = state["A"], state["b"], state["sel"].clone()
    held = solver.solve(variant, x0, u0, xref, A_held, b_held, Ts, term, cp)
    t = select(pool_A, pool_b, held.xopt, n_sel, variant=variant, status=held.status, state=state, **kw)
    min_clear = t["min_clear"]
    first = min_clear.clone()
    rounds_used = torch.zeros(B, dtype=torch.int32, device=dev)
    iters = held.iters.clone()
    cur, var = None, t["variant_out"]
    for _ in range(int(rounds)):
        A_cur, b_cur, sel_cur = t["A"], t["b"], state["sel"].clone()
        if cur is None:
            cur = solver.solve(var, x0, u0, xref, A_cur, b_cur, Ts, term, cp)
        else:
            solver.solve(var, x0, u0, xref, A_cur, b_cur, Ts, term, cp, out=cur)
        iters += cur.iters                                       # a masked instance reports 0
        rounds_used += (var != 0).to(torch.int32)
        t = select(pool_A, pool_b, cur.xopt, n_sel, variant=var, status=cur.status, state=state, **kw)
        better = t["min_clear"] > min_clear                      # NaN (masked, infeasible) compares false
        for name in ("xopt", "uopt", "ts_opt", "status", "info"):
            h, c = getattr(held, name), getattr(cur, name)
            if h is not None:
                h.copy_(torch.where(better.reshape((B,) + (1,) * (h.dim() - 1)), c, h))
        min_clear = torch.where(better, t["min_clear"], min_clear)
        A_held = torch.where(better[:, None, None, None], A_cur, A_held)
        b_held = torch.where(better[:, None, None], b_cur, b_held)
        sel_held = torch.where(better[:, None], sel_cur, sel_held)
        var = t["variant_out"]
    held.iters.copy_(iters)
    return held, {"clear": min_clear >= float(target), "min_clear": min_clear, "min_clear_first": first,
                  "rounds_used": rounds_used, "sel": sel_held, "A_used": A_held, "b_used": b_held}


def grid_pool(grids, K, resolution=1.0, pad=None, far=100.0, device=None):
    """Occupancy grids -> scene pools (obca_grid_pool): grids [B,rows,cols] (non-zero = occupied; a device tensor, e.g.
    ``planner.rasterise_batch``'s, stays on the device), K <= 64 slots per pool.  Every grid is covered greedily (right, then
    down, in row-major order) by disjoint rectangles of cells; rectangle (r0, c0, r1, c1) becomes the box
    [c0 res - pad, c1 res + pad] x [r0 res - pad, r1 res + pad] as 4 rows.  pad=None means resolution / 2 (a cell is a square
    centred on its lattice point, neighbouring rectangles touch); pad=0 is the reference's convention (a cell is a lattice
    point: ``planner.rasterise_batch`` of the boxes gives the grid back).  Spare slots hold the unit square
    [-far-1, -far]^2: far enough never to be near a plan, near enough for a solve that selects it (1e6 is not).

    Returns a dict of device tensors on the current stream, no host synchronisation: pool_A [B,K,4,2], pool_b [B,K,4]
    (``select``'s pool arguments), rect [B,K,4] int32 ((-1,-1,-1,-1) for a spare slot), count [B] int32 (the true number of
    rectangles, also beyond K) and ok [B] int32 (0: count > K, the first K rectangles are written, the map is not covered)."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("scene.grid_pool needs a ROCm GPU; there is no CPU fallback on the product path")
    dev = _dev_of(device, grids)
    if isinstance(grids, torch.Tensor):
        g = grids.to(device=dev, dtype=torch.uint8).contiguous()
    else:
        g = torch.as_tensor(np.ascontiguousarray(grids), device=dev).to(torch.uint8).contiguous()
    if g.dim() != 3:
        raise ValueError("expected grids [B,rows,cols], got %s" % (tuple(g.shape),))
    B, rows, cols = (int(v) for v in g.shape)
    K, resolution = int(K), float(resolution)
    pad = resolution / 2 if pad is None else float(pad)
    k = max(K, 0)
    out = {"pool_A": torch.empty(B, k, 4, 2, dtype=torch.float64, device=dev),
           "pool_b": torch.empty(B, k, 4, dtype=torch.float64, device=dev),
           "rect": torch.empty(B, k, 4, dtype=torch.int32, device=dev),
           "count": torch.empty(B, dtype=torch.int32, device=dev),
           "ok": torch.empty(B, dtype=torch.int32, device=dev)}
    p = _lib.ptr
    _lib.check(_lib.load().obca_grid_pool(p(g), B, rows, cols, K, resolution, pad, float(far), p(out["pool_A"]), p(out["pool_b"]),
                                          p(out["rect"]), p(out["count"]), p(out["ok"]), _lib.device_index(dev),
                                          _lib.stream_ptr(dev)))
    out["pool_A"]._obca_keep = (g,)                          # the launch is asynchronous: see planner.dilate_batch
    g.record_stream(torch.cuda.current_stream(dev))
    return out


def solve_maps(solver, grids, start_cells, goal_cells, start, goal, Ts, K, pad=None, far=100.0, dilation=1, variant=4, u0=None,
               term=None, params=None, rounds=2, n_sub=16, target=0.0, ego=DEFAULT_EGO):
    """B occupancy grids and B start/goal pairs -> B plans, each measured against its whole map, on the current stream without
    host synchronisation: ``grid_pool(grids, K, pad=pad, far=far)`` gives the pools, ``openloop.route_references(grids,
    start_cells, goal_cells, solver.N, start=start, goal=goal, dilation=dilation)`` the references, ``solve_scene(solver,
    variant, x0=start, ...)`` the plans.  grids [B,rows,cols], start_cells / goal_cells [B,2] as (row, col), start / goal
    [B,3] poses, Ts [B] or a float, u0 [B,2] (None: zeros); ``solver`` must have m == [4] * n_sel, n_sel <= K.

    Resolution 1 only, and no ``resolution`` argument: the planner's routes are in cells, so a cell is a metre here.

    An instance whose pool is incomplete (grid_pool's ok == 0) or that has no route (route_references' source == 0) is
    masked -- variant 0, made on the device with ``torch.where`` -- and reported, never raised on.  Returns (result, info)
    exactly as ``solve_scene`` does; ``info`` also carries ``pool`` (grid_pool's dict), ``xref`` [B,3,N+1], ``pool_ok`` [B]
    and ``source`` [B] (2 = the dilated route, 1 = the plain route, 0 = none)."""
    import torch
    from .openloop import route_references
    dev = solver.device
    if not isinstance(grids, torch.Tensor):                  # one upload for the cover and both searches
        import numpy as np
        grids = torch.as_tensor(np.ascontiguousarray(grids), device=dev)
    pool = grid_pool(grids, K, resolution=1.0, pad=pad, far=far, device=dev)
    xref, _, source = route_references(grids, start_cells, goal_cells, solver.N, start=start, goal=goal, dilation=dilation,
                                       device=dev)
    B = int(source.shape[0])
    if isinstance(variant, int):
        variant = torch.full((B,), variant, dtype=torch.int32, device=dev)
    variant = solver._dev(variant, (B,), torch.int32)
    variant = torch.where((pool["ok"] != 0) & (source != 0), variant, 0).to(torch.int32)
    if u0 is None:
        u0 = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    result, info = solve_scene(solver, variant, start, u0, xref, pool["pool_A"], pool["pool_b"], Ts, term=term, params=params,
                               rounds=rounds, n_sub=n_sub, target=target, ego=ego)
    info.update(pool=pool, xref=xref, pool_ok=pool["ok"], source=source)
    return result, info
