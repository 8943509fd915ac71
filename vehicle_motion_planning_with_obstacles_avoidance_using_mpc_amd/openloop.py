"""Batched two-stage open-loop planner on the device -- the reference's ``simulation.run`` entry (src/simulation.py:20-62:
``closedLoop.mpc_openLoop_freeTime`` then ``mpc_openLoop_fixTime``) for B worlds at once, with no host round trip between
the stages.

Stage 1 is a free-time ``obca_mpc4`` plan from a start/goal-only reference, or from a route: ``route_references`` dilates
the occupancy grids, runs the batched A* and resamples each route to the N_free + 1 knots stage 1 tracks (obca_grid_dilate_batch
and obca_route_resample, csrc/obca_route.hip on csrc/obca_route_core.h), and ``plan(..., xref_free=...)`` takes the result.  ``refine`` (obca_plan_refine, csrc/obca_refine.hip
on csrc/obca_refine_core.h) resamples it to ``ratio x N_free`` knots, recomputes the yaws and rescales the step -- the
reference's ``update_path(allAviable=1)``.  Stage 2 is ``obca_mpc6`` against the moving boxes predicted at the new step
(``solver.moving_rows``) with the setting's terminal set; ``obca_mpc8`` answers where ``obca_mpc6`` fails.  The per-instance
mirror ``closed_loop.closedLoop`` stays the readable restatement of the reference; tests compare the two.

Everything runs on the current stream without host synchronisation, the way ``clear.solve_clear`` does: which instances
stage 2 solves, and which of them ``obca_mpc8`` answers, is decided by variant masks built on the device.
"""
import copy

import numpy as np

from . import _lib
from .solver import BatchResult, BatchSolver, SolverParams, moving_rows


def refine(x, ts, ratio, status=None, variant_ok=6, device=None):
    """Stage 1's plans -> stage 2's inputs (obca_plan_refine): x [B,3,N+1], ts [B] and status [B] (None: all feasible) are
    ``BatchSolver.solve``'s xopt, ts_opt and status.  Returns device tensors (xref [B,3,ratio N+1], ts_out [B],
    variant_out [B] int32): the plan resampled to ratio x N intervals with recomputed yaws, ``N ts / (ratio N)``, and
    ``variant_ok`` (4, 6 or 8) -- or, for an instance without a usable plan (status not 0 / 1, a knot or ts not finite,
    ts <= 0), knot 0 at every point (zeros where it is not finite), ts / ratio (0 where not finite) and variant 0, which
    ``BatchSolver.solve`` skips.  On the current stream, no host synchronisation."""
    import torch
    _lib.require_gpu("refine")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _lib.load()
    x = torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
    if x.dim() != 3 or x.shape[1] != 3 or x.shape[2] < 2:
        raise ValueError("expected x [B,3,N+1], got %s" % (tuple(x.shape),))
    B, N, ratio = int(x.shape[0]), int(x.shape[2]) - 1, int(ratio)
    ts = torch.as_tensor(ts, dtype=torch.float64, device=dev).contiguous()
    if tuple(ts.shape) != (B,):
        raise ValueError("expected ts [B], got %s" % (tuple(ts.shape),))
    if status is not None:
        status = torch.as_tensor(status, dtype=torch.int32, device=dev).contiguous()
        if tuple(status.shape) != (B,):
            raise ValueError("expected status [B], got %s" % (tuple(status.shape),))
    xref = torch.empty(B, 3, max(ratio, 0) * N + 1, dtype=torch.float64, device=dev)
    ts_out = torch.empty(B, dtype=torch.float64, device=dev)
    variant_out = torch.empty(B, dtype=torch.int32, device=dev)
    ptr = _lib.ptr
    _lib.launch(lib.obca_plan_refine, B, N, ratio, ptr(x), ptr(ts), ptr(status), int(variant_ok), ptr(xref), ptr(ts_out),
                ptr(variant_out), dev=dev)
    return xref, ts_out, variant_out


def route_reference(path, path_len, N, start=None, goal=None, device=None):
    """Routes -> references of a horizon-N solve (obca_route_resample): path [B,3,path_max] and path_len [B] are
    ``planner.plan_batch``'s outputs, negative codes included; start / goal [B,3] (either may be None) pin the poses of knot 0
    and knot N.  Returns device tensors (xref [B,3,N+1], ok [B] int32): N + 1 knots equally spaced along the route's arc
    length with ``create_reference_path``'s yaws and ok = 1 -- or, for an instance without a usable route (path_len < 2, a
    point not finite, zero length), ok = 0 and the start/goal-only reference where both pins are given, else point 0 of the
    path at every knot (zeros where it is not finite).  On the current stream, no host synchronisation."""
    import torch
    _lib.require_gpu("route_reference")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _lib.load()
    path = torch.as_tensor(path, dtype=torch.float64, device=dev).contiguous()
    if path.dim() != 3 or path.shape[1] != 3:
        raise ValueError("expected path [B,3,path_max], got %s" % (tuple(path.shape),))
    B, P, N = int(path.shape[0]), int(path.shape[2]), int(N)
    path_len = torch.as_tensor(path_len, dtype=torch.int32, device=dev).contiguous()
    if tuple(path_len.shape) != (B,):
        raise ValueError("expected path_len [B], got %s" % (tuple(path_len.shape),))
    pins = []
    for name, v in (("start", start), ("goal", goal)):
        if v is not None:
            v = torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous()
            if tuple(v.shape) != (B, 3):
                raise ValueError("expected %s [B,3], got %s" % (name, tuple(v.shape)))
        pins.append(v)
    xref = torch.empty(B, 3, max(N, 0) + 1, dtype=torch.float64, device=dev)
    ok = torch.empty(B, dtype=torch.int32, device=dev)
    ptr = _lib.ptr
    _lib.launch(lib.obca_route_resample, B, P, N, ptr(path), ptr(path_len), ptr(pins[0]), ptr(pins[1]), ptr(xref), ptr(ok), dev=dev)
    # the launch is asynchronous: the tensors it reads are tied to the result and to the stream (see _lib.keep_alive)
    _lib.keep_alive(xref, (path, path_len, pins[0], pins[1]), dev)
    return xref, ok


def route_search(grids, start_cells, goal_cells, dilation=0, path_max=None, device=None):
    """The search of ``route_references`` alone: the route on ``planner.dilate_batch``'s grid where that search found one
    (path_len >= 2), the route on the plain grid otherwise, chosen by ``torch.where`` on the device.  Returns device tensors
    (path [B,3,path_max], path_len [B] int32 -- ``planner.plan_batch``'s, negative codes included -- and src [B] int32: 2 = the
    dilated search's answer, 1 = the plain one's)."""
    import torch
    from .planner import dilate_batch, plan_batch
    if not isinstance(grids, torch.Tensor):                  # one upload for both searches
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        grids = torch.as_tensor(np.ascontiguousarray(grids), device=dev)
    path, plen = plan_batch(grids, start_cells, goal_cells, path_max=path_max, device=device)
    src = torch.ones_like(plen)
    if int(dilation) > 0:
        path_d, plen_d = plan_batch(dilate_batch(grids, dilation, device=device), start_cells, goal_cells, path_max=path_max,
                                    device=device)
        use_d = plen_d >= 2
        path, plen = torch.where(use_d[:, None, None], path_d, path), torch.where(use_d, plen_d, plen)
        src = torch.where(use_d, 2, 1).to(torch.int32)
    return path, plen, src


def route_references(grids, start_cells, goal_cells, N, start=None, goal=None, dilation=0, path_max=None, device=None):
    """Map -> dilated map -> route -> reference for B worlds on the current stream, no host round trip: grids [B,rows,cols]
    (non-zero = occupied), start_cells / goal_cells [B,2] as (row, col) -- ``planner.plan_batch``'s arguments --, start /
    goal [B,3] the poses ``route_reference`` pins.  With dilation > 0 the search runs on ``planner.dilate_batch``'s grid AND on
    the plain one; an instance takes the dilated route where that search found one (path_len >= 2) and the plain route
    otherwise, chosen by ``torch.where`` on the device (``route_search``).  Returns (xref [B,3,N+1], ok [B] int32, source [B]
    int32): 2 = the dilated route, 1 = the plain route, 0 = neither (``route_reference``'s fill)."""
    import torch
    path, plen, src = route_search(grids, start_cells, goal_cells, dilation=dilation, path_max=path_max, device=device)
    xref, ok = route_reference(path, plen, N, start, goal, device=device)
    return xref, ok, torch.where(ok == 1, src, 0).to(torch.int32)


class TwoStagePlan:
    """What ``TwoStagePlanner.plan`` returns (device tensors): ``free`` / ``fix`` -- the ``BatchResult`` of stage 1 and of
    stage 2 (``iters`` summed over the obca_mpc6 and the obca_mpc8 launch; status OBCA_STATUS_SKIPPED and zero outputs where
    stage 1 had no plan); stage 2's inputs ``xref_fix`` [B,3,N_fix+1], ``ts_fix`` [B], ``A_fix`` [B,N_fix+1,M,2], ``b_fix``
    [B,N_fix+1,M], ``term`` [B,3]; ``variant_fix`` [B]: 6 or 8 for the variant that answered, 0 where stage 1 had no plan;
    ``feas`` [B] bool: stage 2 has a feasible plan."""
    __slots__ = ("free", "fix", "xref_fix", "ts_fix", "A_fix", "b_fix", "term", "variant_fix", "feas")


def _zero_result(B, N, dev):
    """outputs a masked launch may leave untouched: zeros, not uninitialised memory"""
    import torch
    r = BatchResult()
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
    r.xopt, r.uopt, r.ts_opt, r.info = z(B, 3, N + 1), z(B, 2, N), z(B), z(B, 4)
    r.status, r.iters = torch.full((B,), _lib.STATUS_SKIPPED, dtype=torch.int32, device=dev), z(B, dt=torch.int32)
    return r


class TwoStagePlanner:
    """Two solver handles for one world shape: (N_free, m_static) for stage 1 and (ratio N_free, m_static + [4] * n_box) for
    stage 2, at most ``max_batch`` worlds per call."""

    def __init__(self, N_free, ratio, m_static, n_box, max_batch, device=None):
        self.N_free, self.ratio, self.N_fix = int(N_free), int(ratio), int(ratio) * int(N_free)
        self.m_static, self.n_box = [int(v) for v in m_static], int(n_box)
        if self.ratio < 1 or self.N_free < 1:
            raise ValueError("N_free >= 1 and ratio >= 1, got %d and %d" % (self.N_free, self.ratio))
        self.free_solver = BatchSolver(self.N_free, self.m_static, max_batch, device=device)
        try:
            self.fix_solver = BatchSolver(self.N_fix, self.m_static + [4] * self.n_box, max_batch, device=device)
        except Exception:
            self.free_solver.close()
            raise
        self.device = self.free_solver.device

    def close(self):
        for s in (getattr(self, "free_solver", None), getattr(self, "fix_solver", None)):
            if s is not None:
                s.close()

    def plan(self, start, goal, static_A, static_b, boxes, term, Ts=0.1, u0=None, params=None, half_window=0.0, margin=0.0,
             xref_free=None):
        """start [B,3], goal [B,3], static_A [B,Ms,2], static_b [B,Ms], boxes [B,n_box,13] (``solver.moving_rows``' tuple),
        term [B,3] (the terminal set as ``BatchSolver.solve`` takes it), Ts: stage 1's nominal step, u0 [B,2] (None: zeros),
        params: ``SolverParams`` for both stages -- stage 1 runs them with start_order "x0" unless another order is set (its
        reference is start and goal only, no trajectory a solve could start from), stage 2's obca_mpc6 with the first start of
        the ladder only, because obca_mpc8 follows a failure.  half_window / margin: ``solver.moving_rows``' swept, inflated
        boxes for stage 2.  xref_free [B,3,N_free+1] (None: the start/goal-only reference): the reference stage 1 tracks, e.g.
        ``route_references``'; with it stage 1 keeps the caller's start_order -- there is a trajectory to start from.
        Returns a ``TwoStagePlan``."""
        import torch
        dev, Nf, N2 = self.device, self.N_free, self.N_fix
        params = params or SolverParams()
        t = lambda a, shape, dt=torch.float64: self.free_solver._dev(a, shape, dt)
        start = torch.as_tensor(start, dtype=torch.float64, device=dev)
        B, Ms = int(start.shape[0]), sum(self.m_static)
        start, goal, term = t(start, (B, 3)), t(goal, (B, 3)), t(term, (B, 3))
        static_A, static_b, boxes = t(static_A, (B, Ms, 2)), t(static_b, (B, Ms)), t(boxes, (B, self.n_box, 13))
        u0 = t(torch.zeros(B, 2) if u0 is None else u0, (B, 2))
        Ts = torch.as_tensor(Ts, dtype=torch.float64, device=dev)
        Ts = t(Ts.expand(B) if Ts.dim() == 0 else Ts, (B,))

        # stage 1: obca_mpc4, reference = the start pose, then the goal pose N_free times; the static rows at every stage
        # (or the caller's reference, under the caller's start order)
        A1 = static_A[:, None].expand(B, Nf + 1, Ms, 2)
        b1 = static_b[:, None].expand(B, Nf + 1, Ms)
        p1 = copy.copy(params)
        if xref_free is None:
            xref = torch.cat([start[:, :, None], goal[:, :, None].expand(B, 3, Nf)], 2)
            if p1.start_order == _lib.START_DEFAULT:
                p1.start_order = _lib.START_X0_FIRST
        else:
            xref = t(xref_free, (B, 3, Nf + 1))
        free = self.free_solver.solve(4, start, u0, xref, A1, b1, Ts, None, p1)

        # refinement and stage 2's rows, from stage 1's outputs where they lie
        xref_fix, ts_fix, var6 = refine(free.xopt, free.ts_opt, self.ratio, free.status, 6, device=dev)
        A_fix, b_fix = moving_rows(static_A, static_b, boxes, ts_fix, N2, half_window, margin, device=dev)

        # stage 2: obca_mpc6 with the first start only, then obca_mpc8 (whole ladder) for the instances it did not answer
        p6 = copy.copy(params)
        p6.single_start = True
        r6 = self.fix_solver.solve(var6, start, u0, xref_fix, A_fix, b_fix, ts_fix, term, p6, out=_zero_result(B, N2, dev))
        solved6 = (r6.status == _lib.STATUS_OK) | (r6.status == _lib.STATUS_ACCEPTABLE)
        var8 = torch.where((var6 != 0) & ~solved6, 8, 0).to(torch.int32)
        r8 = self.fix_solver.solve(var8, start, u0, xref_fix, A_fix, b_fix, ts_fix, term, params, out=_zero_result(B, N2, dev))
        use8 = var8 != 0
        fix = BatchResult()
        for name in ("xopt", "uopt", "ts_opt", "status", "info"):
            a8, a6 = getattr(r8, name), getattr(r6, name)
            setattr(fix, name, torch.where(use8.reshape((B,) + (1,) * (a6.dim() - 1)), a8, a6))
        fix.status = torch.where(var6 == 0, _lib.STATUS_SKIPPED, fix.status).to(torch.int32)
        fix.iters = r6.iters + r8.iters                              # a masked instance reports 0

        out = TwoStagePlan()
        out.free, out.fix = free, fix
        out.xref_fix, out.ts_fix, out.A_fix, out.b_fix, out.term = xref_fix, ts_fix, A_fix, b_fix, term
        out.variant_fix = torch.where(use8, 8, var6).to(torch.int32)
        out.feas = fix.feas & (var6 != 0)
        return out


class PlanArguments:
    """``from_settings``' result: ``m_static`` and ``n_box`` for the planner's constructor, ``kwargs()`` for ``plan``."""
    __slots__ = ("m_static", "n_box", "start", "goal", "static_A", "static_b", "boxes", "term", "params")

    def kwargs(self):
        return {k: getattr(self, k) for k in self.__slots__[2:]}


def from_settings(settings):
    """B ``problemSetting`` objects of one shape -> the arguments of ``TwoStagePlanner`` (numpy arrays): rows and boxes from
    ``rollouts.pack_worlds``, goal = goalPose[:3], term = (ts[0,0], ts[1,0], ts[1,1]) of the setting's terminal set (the
    packing of ``solver.pack_reference_call``), the setting's position box xL / xU in the ``SolverParams``."""
    from .rollouts import pack_worlds
    settings = list(settings)
    w = pack_worlds(settings)
    a = PlanArguments()
    a.m_static, a.n_box = list(w.m_static), int(w.n_dyn)
    a.start, a.static_A, a.static_b, a.boxes = w.start, w.static_A, w.static_b, w.dyn
    a.goal = np.array([np.asarray(s.goalPose[:3], float) for s in settings])
    ts = [np.asarray(s.terminal_set, float) for s in settings]
    a.term = np.array([(v[0, 0], v[1, 0], v[1, 1]) for v in ts])
    a.params = SolverParams(xL=w.xL, xU=w.xU)
    return a


def route_arguments(settings):
    """B ``problemSetting`` objects of one map shape -> (grids [B,rows,cols] uint8, start_cells [B,2], goal_cells [B,2]) for
    ``route_references``, read from a setting the way ``rollouts.device_reference_paths`` reads them: ``org_gridMap`` and
    (row, col) = (pose_y, pose_x) of ``startPose`` / ``goalPose``."""
    settings = list(settings)
    grids = np.stack([np.asarray(s.org_gridMap) for s in settings]).astype(np.uint8)
    cells = lambda name: np.array([(getattr(s, name)[1], getattr(s, name)[0]) for s in settings]).astype(np.int32)
    return grids, cells("startPose"), cells("goalPose")
