"""Clearance repair of batched plans: solve, measure between the knots, grow the obstacles where the plan comes too close,
solve those instances again -- a few rounds, all on the device.

``solve_clear`` wraps ``BatchSolver.solve``.  The measuring and the row update are ``audit.plan_tighten``
(obca_plan_tighten, geometry and reasoning in csrc/obca_audit_core.h); no solver kernel is involved in the repair beyond
being called again with other rows.  A module of its own because ``audit`` imports from ``solver``.
"""
from .audit import plan_tighten
from .solver import DEFAULT_EGO, SolverParams


def solve_clear(solver, variant, x0, u0, xref, A, b, Ts, term=None, params=None, ego=DEFAULT_EGO, rounds=4, n_sub=16,
                target=0.0, gain=1.0, grow_max=2.0, certified=False):
    """``solver.solve(variant, x0, u0, xref, A, b, Ts, term, params)`` followed by up to ``rounds`` repair rounds.

    Round 0 solves every instance with the caller's rows.  Every later round solves only the instances whose last plan was
    feasible and came closer than ``target`` to an obstacle somewhere between two knots (n_sub + 1 samples per interval;
    certified: the certified bound instead), with that obstacle grown at the two stages next to the interval by ``gain``
    times the shortfall, at most ``grow_max`` metres in all; A is never changed.  One plan per instance is held: round 0's,
    replaced by a later one only if that is feasible and its clearance against the ORIGINAL rows is larger.  An instance
    ends when its plan measures >= target, its re-solve is infeasible, its growth is capped or the rounds are spent.

    Runs on the current stream without host synchronisation.  Returns (result, info): the held ``BatchResult`` (``iters``
    summed over the rounds; with rounds = 0 exactly ``solver.solve``'s words) and a dict of device tensors:
    clear [B] bool (the held plan measures >= target), min_clear [B] and min_clear_first [B] (the held plan's and round
    0's clearance against the original rows; NaN where there is no feasible plan or it is not finite), rounds_used [B]
    (re-solves of the instance), grow [B,N+1,n_obs] and b_used [B,N+1,M] (the growth and the rows the held plan was solved
    with)."""
    import torch
    params = params or SolverParams()
    dev, N, M, m = solver.device, solver.N, solver.M, solver.m
    x0 = torch.as_tensor(x0, dtype=torch.float64, device=dev)
    B = x0.shape[0]
    if isinstance(variant, int):
        variant = torch.full((B,), variant, dtype=torch.int32, device=dev)
    on_dev = lambda t, shape, dt=torch.float64: solver._dev(t, shape, dt)
    variant = on_dev(variant, (B,), torch.int32)
    x0, u0, xref = on_dev(x0, (B, 3)), on_dev(u0, (B, 2)), on_dev(xref, (B, 3, N + 1))
    A, b, Ts = on_dev(A, (B, N + 1, M, 2)), on_dev(b, (B, N + 1, M)), on_dev(Ts, (B,))
    term = on_dev(torch.zeros(B, 3) if term is None else term, (B, 3))
    cp = params.to_c() if isinstance(params, SolverParams) else params

    held = solver.solve(variant, x0, u0, xref, A, b, Ts, term, cp)
    grow = torch.zeros(B, N + 1, len(m), dtype=torch.float64, device=dev)
    kw = dict(n_sub=n_sub, certified=certified, target=target, gain=gain, grow_max=grow_max, ego=ego)
    t = plan_tighten(held.xopt, A, b, m, variant, held.status, grow=grow, **kw)
    min_clear = t["min_clear"]
    first = min_clear.clone()
    grow_held, b_held = torch.zeros_like(grow), b.clone()
    rounds_used = torch.zeros(B, dtype=torch.int32, device=dev)
    iters = held.iters.clone()
    cur, var, b_cur, b_next = None, t["variant_out"], t["b_out"], torch.empty_like(b)
    for _ in range(int(rounds)):
        if cur is None:
            cur = solver.solve(var, x0, u0, xref, A, b_cur, Ts, term, cp)
        else:
            solver.solve(var, x0, u0, xref, A, b_cur, Ts, term, cp, out=cur)
        iters += cur.iters                                       # a masked instance reports 0
        rounds_used += (var != 0).to(torch.int32)
        grow_cur = grow.clone()
        t = plan_tighten(cur.xopt, A, b, m, var, cur.status, grow=grow, b_out=b_next, **kw)
        better = t["min_clear"] > min_clear                      # NaN (masked, infeasible, not finite) compares false
        for name in ("xopt", "uopt", "ts_opt", "status", "info"):
            h, c = getattr(held, name), getattr(cur, name)
            if h is not None:
                h.copy_(torch.where(better.reshape((B,) + (1,) * (h.dim() - 1)), c, h))
        min_clear = torch.where(better, t["min_clear"], min_clear)
        grow_held = torch.where(better[:, None, None], grow_cur, grow_held)
        b_held = torch.where(better[:, None, None], b_cur, b_held)
        var, b_cur, b_next = t["variant_out"], b_next, b_cur
    held.iters.copy_(iters)
    return held, {"clear": min_clear >= float(target), "min_clear": min_clear, "min_clear_first": first,
                  "rounds_used": rounds_used, "grow": grow_held, "b_used": b_held}
