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

``PoolLoop`` is the receding-horizon version: B rollouts, each in a world that is a pool (static, or translating at constant
velocities), driven by select -> solve -> obca_pool_loop_advance per step.  The advance call (arithmetic and serial definition
in csrc/obca_poolloop_core.h) records the step, measures the applied interval against the WHOLE pool, moves the pool by the
applied step length, advances the state, sets the flags and writes the next reference window from the route.  ``drive_maps``
composes ``grid_pool``, ``openloop.route_search`` and ``PoolLoop``: B maps and B start/goal pairs in, B driven trajectories
out.  ``FleetLoop`` puts V of those rollouts into one world: after every step obca_fleet_step (csrc/obca_fleet_core.h) writes
the other cars of the world into the last V pool slots of each car and measures what the cars did to each other; with predict="plan" obca_fleet_tracks
(csrc/obca_fleet_tracks_core.h) then turns the plans just applied into rows per stage, which the next ``select`` reads through
obca_scene_select_staged.  ``TrackLoop`` gives a world obstacles that follow timed tracks -- recorded or scripted road users
that turn, brake, stop or set off later: after every step obca_pool_tracks (csrc/obca_pool_tracks_core.h) writes the last Kt pool
slots from the tracks' poses now, their rows at the stage times of the next solve for obca_scene_select_staged, and measures what
the car kept from the tracks themselves.  ``solve_tracks`` is ``solve_scene`` among such obstacles, for whole plans: ``track_rows``
gives the stage rows of an open-loop solve, ``plan_track_clearance`` (obca_plan_tracks, csrc/obca_plan_tracks_core.h) measures a
batch of plans against the tracks themselves -- the track's own rectangle at its own pose at every sample's time, which rows
interpolated between two stage times cannot show -- and folds that into the running minimum the staged ``select`` re-ranks on.
Not here: the reference's 4 -> 6 -> 8 dispatch, its lidar gate and its fixed-time reference preparation
(``rollouts.DeviceRollouts`` has those, for at most 8 static obstacles).
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
           ego=DEFAULT_EGO, device=None, stage_A=None, stage_b=None, stage_ok=None, stage_group=1):
    """pool_A [B,K,E,2], pool_b [B,K,E] (K <= 64 obstacles of E rows each), pool_v [B,K,2] m/s or None, Ts [B] or a float
    (needed with pool_v); x [B,3,N+1] the poses to measure (a reference window, or plans), x0 [B,3] or None one more pose
    against stage 0's rows; variant [B], an int or None (4: every sample against stage 0's rows), status [B] or None.

    ``state=None``: scores are written from the samples and every usable instance counts as changed.  ``state`` = the dict a
    previous call returned: its ``score`` and ``sel`` are updated IN PLACE to the running minimum and the new selection, and
    only instances with variant != 0 and status 0 / 1 are measured.

    ``stage_A`` [B/stage_group,Kt,N+1,E,2], ``stage_b`` [B/stage_group,Kt,N+1,E] and ``stage_ok`` [B,Kt] int32 (given together, or
    not at all) make it obca_scene_select_staged: pool slot K - Kt + t of instance b has the rows stage_A / stage_b[b //
    stage_group, t, kk] at stage kk where stage_ok[b,t] != 0 (a track, e.g. one of ``fleet_tracks``), in place of its pool rows moved by
    pool_v.  Without them obca_scene_select is called.

    Returns a dict of device tensors on the current stream, no host synchronisation: A [B,N+1,n_sel E,2] and b [B,N+1,n_sel E]
    (rows for a handle with m = [E] * n_sel), sel [B,n_sel] int32 ascending pool indices, variant_out [B] (variant where the
    selection changed, else 0), ok [B] (0: unusable pool or poses, filled rows a = (1, 0), b = -1e6), score [B,K] (NaN where
    never written) and min_clear [B] (this call's smallest distance over the whole pool, NaN where not measured)."""
    import torch
    _lib.require_gpu("scene.select")
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
    staged = (stage_A, stage_b, stage_ok)
    if all(a is None for a in staged):
        _lib.launch(_lib.load().obca_scene_select, ego_c, B, K, E, N1 - 1, n_sel, int(n_sub), 0 if state is None else 1, p(pool_A),
                    p(pool_b), p(pool_v), p(Ts), p(x), p(x0), p(variant), p(status), p(score), p(sel), p(out["A"]), p(out["b"]),
                    p(out["variant_out"]), p(out["ok"]), p(out["min_clear"]), dev=dev)
        staged = ()
    else:
        if any(a is None for a in staged):
            raise ValueError("stage_A, stage_b and stage_ok are given together")
        stage_ok = torch.as_tensor(stage_ok, dtype=torch.int32, device=dev).contiguous()
        group = int(stage_group)
        if stage_ok.dim() != 2 or stage_ok.shape[0] != B or group < 1 or B % group != 0:
            raise ValueError("expected stage_ok [B,Kt] and a stage_group that divides B = %d" % B)
        Kt = int(stage_ok.shape[1])
        stage_A, stage_b = opt(stage_A, (B // group, Kt, N1, E, 2)), opt(stage_b, (B // group, Kt, N1, E))
        staged = (stage_A, stage_b, stage_ok)
        _lib.launch(_lib.load().obca_scene_select_staged, ego_c, B, K, E, N1 - 1, n_sel, int(n_sub), 0 if state is None else 1,
                    p(pool_A), p(pool_b), p(pool_v), p(Ts), p(x), p(x0), p(variant), p(status), Kt, group, p(stage_A), p(stage_b),
                    p(stage_ok), p(score), p(sel), p(out["A"]), p(out["b"]), p(out["variant_out"]), p(out["ok"]), p(out["min_clear"]),
                    dev=dev)
    # the launch is asynchronous: the tensors it reads are tied to the result and to the stream (see _lib.keep_alive)
    _lib.keep_alive(out["A"], (pool_A, pool_b, pool_v, Ts, x, x0, variant, status) + staged, dev)
    return out


def _fleet_tracks_desc(G, V, N, see, margin, far, ego, **members):
    """the descriptor of obca_fleet_tracks: ``fleet_tracks``' and ``FleetLoop``'s"""
    return _lib.ObcaFleetTracks().set(G=G, V=V, N=N, see=_lib.FLEET_SEE[see], margin=float(margin), far=float(far), ego=ego, **members)


def fleet_tracks(x0, flags, k, xopt, status, V, step, see="all", margin=0.0, far=100.0, ego=DEFAULT_EGO, out=None, device=None):
    """obca_fleet_tracks: the plans just applied as rows per stage.  x0 [B,3], flags [B], k [B] as they are after obca_fleet_step
    of loop step ``step``, xopt [B,3,N+1] and status [B] the solve that was applied; B = G V.  Returns a dict of device tensors
    on the current stream, no host synchronisation: track_A [G,V,N+1,4,2], track_b [G,V,N+1,4] and track_ok [B,V] int32 --
    ``select``'s stage_A, stage_b and stage_ok with stage_group = V for pools whose last V slots are the cars.  ``out``: a dict
    of such tensors to write into."""
    import torch
    _lib.require_gpu("scene.fleet_tracks")
    if see not in _lib.FLEET_SEE:
        raise ValueError("see is one of %s" % sorted(_lib.FLEET_SEE))
    dev = _dev_of(device, xopt, x0)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=dev).contiguous()
    x0, xopt, flags, k, status = t(x0), t(xopt), t(flags, torch.int32), t(k, torch.int32), t(status, torch.int32)
    V = int(V)
    if xopt.dim() != 3 or xopt.shape[1] != 3 or V < 1 or xopt.shape[0] % V != 0:
        raise ValueError("expected xopt [B,3,N+1] with B a multiple of V")
    B, N1 = int(xopt.shape[0]), int(xopt.shape[2])
    for a, shape in ((x0, (B, 3)), (flags, (B,)), (k, (B,)), (status, (B,))):
        if tuple(a.shape) != shape:
            raise ValueError("expected shape %s, got %s" % (shape, tuple(a.shape)))
    G = B // V
    if out is None:
        out = {"track_A": torch.empty(G, V, N1, 4, 2, dtype=torch.float64, device=dev),
               "track_b": torch.empty(G, V, N1, 4, dtype=torch.float64, device=dev),
               "track_ok": torch.empty(B, V, dtype=torch.int32, device=dev)}
    d = _fleet_tracks_desc(G, V, N1 - 1, see, margin, far, ego, step=int(step), x0=x0, flags=flags, k=k, xopt=xopt, status=status,
                           track_A=out["track_A"], track_b=out["track_b"], track_ok=out["track_ok"])
    _lib.launch(_lib.load().obca_fleet_tracks, ctypes.byref(d), dev=dev)
    _lib.keep_alive(out["track_A"], (x0, flags, k, xopt, status), dev)     # the launch is asynchronous: see ``select``
    return out


def check_tracks(tracks, track_t, track_len, track_size):
    """host arrays of tracks (``pool_tracks``' first four arguments) checked by obca_pool_tracks' own rules; raises ValueError for
    the first track that is not usable.  A length of 0 (a spare on request) passes."""
    import numpy as np
    x, t, ln, size = np.asarray(tracks, float), np.asarray(track_t, float), np.asarray(track_len), np.asarray(track_size, float)
    L = x.shape[2]
    for bt in range(x.shape[0]):
        for j in range(x.shape[1]):
            n = int(ln[bt, j])
            if n == 0:
                continue
            why = None
            if not 1 <= n <= L:
                why = "length %d outside 1 .. %d" % (n, L)
            elif not (np.all(np.isfinite(x[bt, j, :n])) and np.all(np.isfinite(t[bt, j, :n]))):
                why = "a pose word or a time that is not finite"
            elif not np.all(np.diff(t[bt, j, :n]) > 0.0):
                why = "times that do not increase strictly"
            elif not (np.all(np.isfinite(size[bt, j])) and size[bt, j, 0] + size[bt, j, 2] > 0.0 and size[bt, j, 1] + size[bt, j, 3] > 0.0):
                why = "a size that is no rectangle"
            if why:
                raise ValueError("track %d of block %d is not usable: %s" % (j, bt, why))


def _pool_tracks_desc(B, K, Kt, N, L, group, max_steps, n_sub, predict, clearance, margin, far, ego, **members):
    """the descriptor of obca_pool_tracks: ``pool_tracks``' and ``TrackLoop``'s"""
    return _lib.ObcaPoolTracks().set(B=B, K=K, Kt=Kt, N=N, L=L, group=group, max_steps=max_steps, n_sub=int(n_sub),
                                     predict=_lib.TRACK_PREDICT[predict], clearance=NEVER_STOP if clearance is None else float(clearance),
                                     margin=float(margin), far=float(far), ego=ego, **members)


def pool_tracks(tracks, track_t, track_len, track_size, Ts, k, x0, pool_A, pool_b, pool_v, N, group=1, t0=None, predict="track",
                margin=0.0, far=100.0, measure=False, step=0, x_prev=None, flags=None, max_steps=1, n_sub=8, clearance=None,
                ego=DEFAULT_EGO, out=None, device=None):
    """obca_pool_tracks: timed tracks as the rows of the last Kt pool slots, now and at the N + 1 stage times of the next solve.
    tracks [Bt,Kt,L,3] poses (x, y, heading; unwrapped), track_t [Bt,Kt,L], track_len [Bt,Kt] int32, track_size [Bt,Kt,4] in
    ego's convention; rollout b of B = Bt * group reads block b // group.  Ts [B] or a float, k [B] int32 and x0 [B,3] the
    loop's state, t0 [B] or None; pool_A [B,K,4,2], pool_b [B,K,4], pool_v [B,K,2] contiguous float64 DEVICE tensors, whose
    slots K - Kt .. K - 1 are written IN PLACE.  measure=True also measures the interval x_prev -> x0 of every rollout with
    k == step + 1 against the tracks themselves (n_sub + 1 samples) and may end it: flags [B] int32 is updated in place
    (clearance=None: measured, never stopped).

    Returns a dict of device tensors on the current stream, no host synchronisation: stage_A [B,Kt,N+1,4,2], stage_b
    [B,Kt,N+1,4] and stage_ok [B,Kt] int32 -- ``select``'s arguments of those names with stage_group = 1 -- track_state [B,Kt]
    int32 (1 usable, 0 a length of 0, -1 not usable: a spare), track_clear_hist [B,max_steps] (word ``step`` written where
    measured), flags, xref_out [B,3,N+1] and variant_out [B] (written for a rollout that measure ended).  ``out``: a dict of
    such tensors to write into."""
    import torch
    _lib.require_gpu("scene.pool_tracks")
    if predict not in _lib.TRACK_PREDICT:
        raise ValueError("predict is one of %s" % sorted(_lib.TRACK_PREDICT))
    dev = _dev_of(device, pool_A, tracks, x0)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=dev).contiguous()
    tracks, track_t, track_len, track_size = t(tracks), t(track_t), t(track_len, torch.int32), t(track_size)
    if tracks.dim() != 4 or tracks.shape[3] != 3:
        raise ValueError("expected tracks [Bt,Kt,L,3], got %s" % (tuple(tracks.shape),))
    Bt, Kt, L = (int(v) for v in tracks.shape[:3])
    group, N = int(group), int(N)
    B = Bt * group
    x0, k = t(x0), t(k, torch.int32)
    Ts = torch.as_tensor(Ts, dtype=torch.float64, device=dev)
    Ts = (Ts.expand(B) if Ts.dim() == 0 else Ts).contiguous()
    t0 = None if t0 is None else t(t0)
    x_prev = x0 if x_prev is None else t(x_prev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev) if flags is None else flags
    for a in (pool_A, pool_b, pool_v, flags):
        if not (isinstance(a, torch.Tensor) and a.device == dev and a.is_contiguous()):
            raise ValueError("pool_A, pool_b, pool_v and flags are written in place: contiguous tensors on %s" % dev)
    if pool_A.dtype != torch.float64 or pool_b.dtype != torch.float64 or pool_v.dtype != torch.float64 or flags.dtype != torch.int32:
        raise ValueError("expected float64 pools and int32 flags")
    K = int(pool_b.shape[1]) if pool_b.dim() == 3 else -1
    for a, shape in ((track_t, (Bt, Kt, L)), (track_len, (Bt, Kt)), (track_size, (Bt, Kt, 4)), (Ts, (B,)), (k, (B,)), (x0, (B, 3)),
                     (x_prev, (B, 3)), (flags, (B,)), (pool_A, (B, K, 4, 2)), (pool_b, (B, K, 4)), (pool_v, (B, K, 2))) + \
            (() if t0 is None else ((t0, (B,)),)):
        if tuple(a.shape) != shape:
            raise ValueError("expected shape %s, got %s" % (shape, tuple(a.shape)))
    S = int(max_steps)
    if out is None:
        out = {"stage_A": torch.empty(B, Kt, N + 1, 4, 2, dtype=torch.float64, device=dev),
               "stage_b": torch.empty(B, Kt, N + 1, 4, dtype=torch.float64, device=dev),
               "stage_ok": torch.empty(B, Kt, dtype=torch.int32, device=dev),
               "track_state": torch.empty(B, Kt, dtype=torch.int32, device=dev),
               "track_clear_hist": torch.full((B, max(S, 1)), float("inf"), dtype=torch.float64, device=dev),
               "xref_out": torch.zeros(B, 3, N + 1, dtype=torch.float64, device=dev),
               "variant_out": torch.zeros(B, dtype=torch.int32, device=dev)}
    out["flags"] = flags
    ins = dict(track_x=tracks, track_t=track_t, track_len=track_len, track_size=track_size, t0=t0, Ts=Ts, x_prev=x_prev, x0=x0, k=k)
    d = _pool_tracks_desc(B, K, Kt, N, L, group, S, n_sub, predict, clearance, margin, far, ego, step=int(step), flags=flags,
                          pool_A=pool_A, pool_b=pool_b, pool_v=pool_v, **ins,
                          **{n: out[n] for n in ("stage_A", "stage_b", "stage_ok", "track_state", "track_clear_hist", "xref_out", "variant_out")})
    _lib.launch(_lib.load().obca_pool_tracks, ctypes.byref(d), 1 if measure else 0, dev=dev)
    _lib.keep_alive(out["stage_A"], ins.values(), dev)                    # the launch is asynchronous: see ``select``
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
    _lib.require_gpu("scene.grid_pool")
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
    _lib.launch(_lib.load().obca_grid_pool, p(g), B, rows, cols, K, resolution, pad, float(far), p(out["pool_A"]), p(out["pool_b"]),
                p(out["rect"]), p(out["count"]), p(out["ok"]), dev=dev)
    _lib.keep_alive(out["pool_A"], (g,), dev)                # the launch is asynchronous: see planner.dilate_batch
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


NEVER_STOP = -1e300          # obca_pool_loop.clearance must be finite: below every distance a double can hold


def _with_spare_slots(solver, B, pool_A, pool_b, pool_v, n, far, what):
    """the static part of every rollout's pool -- pool_A [B,Ks,4,2], pool_b [B,Ks,4] and optionally pool_v [B,Ks,2], or None for
    Ks = 0 -- with n spare slots (``grid_pool``'s spare at ``far``) appended, which a loop's step call rewrites at every reset
    and after every step.  Returns (full_A, full_b, full_v, Ks); ``what`` names the n slots in the error message."""
    import torch
    dev = solver.device
    f64 = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)
    if pool_A is None or pool_b is None:
        if pool_A is not None or pool_b is not None or pool_v is not None:
            raise ValueError("pool_A and pool_b are given together; without them there is no pool_v")
        sA, sb = torch.zeros(B, 0, 4, 2, dtype=torch.float64, device=dev), torch.zeros(B, 0, 4, dtype=torch.float64, device=dev)
    else:
        sA, sb = f64(pool_A), f64(pool_b)
    if sA.dim() != 4 or sb.dim() != 3 or tuple(sA.shape) != tuple(sb.shape) + (2,) or sb.shape[0] != B or sb.shape[2] != 4:
        raise ValueError("expected pool_A [B,Ks,4,2], pool_b [B,Ks,4] with B = %d" % B)
    Ks = int(sb.shape[1])
    if Ks + n > 64:
        raise ValueError("Ks + %s = %d slots: a pool holds 64 at the most" % (what, Ks + n))
    sv = torch.zeros(B, Ks, 2, dtype=torch.float64, device=dev) if pool_v is None else solver._dev(pool_v, (B, Ks, 2))
    spare_A = f64([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]])
    spare_b = f64([-far, -far, far + 1.0, far + 1.0])
    full_A = torch.cat([sA, spare_A.expand(B, n, 4, 2)], dim=1).contiguous()
    full_b = torch.cat([sb, spare_b.expand(B, n, 4)], dim=1).contiguous()
    full_v = torch.cat([sv, torch.zeros(B, n, 2, dtype=torch.float64, device=dev)], dim=1).contiguous()
    return full_A, full_b, full_v, Ks


class _OnDevice:
    """what ``_with_spare_slots`` asks of a solver, for a caller that has none: a device and ``BatchSolver._dev``'s check"""

    def __init__(self, device):
        self.device = device

    def _dev(self, t, shape, dtype=None):
        import torch
        t = torch.as_tensor(t, dtype=dtype or torch.float64, device=self.device).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(t.shape)))
        return t


def _tracks_on_device(tracks, track_t, track_len, track_size, ego, dev):
    """tracks [Bt,Kt,L,3], track_t [Bt,Kt,L], track_len [Bt,Kt] and track_size [Bt,Kt,4] (None: ``ego``'s) as contiguous device
    tensors.  Tracks given as host arrays go through ``check_tracks`` and an unusable one raises; device tensors are taken at
    their word."""
    import numpy as np
    import torch
    on_host = lambda a: not (isinstance(a, torch.Tensor) and a.is_cuda)
    shape = tuple(np.shape(tracks) if on_host(tracks) else tracks.shape)
    if len(shape) != 4 or shape[3] != 3 or shape[1] < 1 or shape[2] < 1:
        raise ValueError("expected tracks [Bt,Kt,L,3], got %s" % (shape,))
    Bt, Kt, L = shape[:3]
    if track_size is None:
        track_size = np.tile(np.asarray(ego, float), (Bt, Kt, 1))
    for a, want in ((track_t, (Bt, Kt, L)), (track_len, (Bt, Kt)), (track_size, (Bt, Kt, 4))):
        got = tuple(np.shape(a) if on_host(a) else a.shape)
        if got != want:
            raise ValueError("expected shape %s next to tracks %s, got %s" % (want, shape, got))
    if all(on_host(a) for a in (tracks, track_t, track_len, track_size)):
        check_tracks(tracks, track_t, track_len, track_size)
    f64 = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous()
    return f64(tracks), f64(track_t), torch.as_tensor(track_len, dtype=torch.int32, device=dev).contiguous(), f64(track_size)


def plan_track_clearance(x, tracks, track_t, track_len, dt, track_size=None, t0=None, x0=None, variant=None, status=None, group=1,
                         n_sub=16, score=None, ego=DEFAULT_EGO, device=None):
    """obca_plan_tracks: plans x [B,3,N+1] measured against timed tracks themselves -- at every sample the track's own rectangle at
    the track's pose at the sample's time, across knots and turning, where ``select``'s staged score rests on rows interpolated
    between two stage times.  tracks [Bt,Kt,L,3], track_t [Bt,Kt,L], track_len [Bt,Kt], track_size [Bt,Kt,4] (None: ``ego``'s) as
    ``TrackLoop`` takes them, plan b of B = Bt * group reading block b // group; host arrays are checked (``check_tracks``) and an
    unusable track raises, device tensors are taken at their word (track_state -1).  dt [B] or a float is the time between two
    knots of a plan (a plan of obca_mpc4: Ts * ts_opt), t0 [B], a float or None the time of knot 0: knot kk is at t0 + kk dt,
    the word ``pool_tracks`` forms for stage kk with k = 0 and Ts = dt.  x0 [B,3] or None is one more pose at knot 0's time.
    The samples are ``select``'s: n_sub + 1 per interval.  variant [B] / status [B], each or None: only plans with variant != 0
    and status 0 / 1 are measured.

    ``score``: a contiguous float64 device tensor [B,K], K >= Kt -- ``select``'s state["score"] for pools whose last Kt slots are
    the tracks -- whose slots K - Kt .. K - 1 are folded IN PLACE to min(score, track_clear) for every measured plan and usable
    track: the running minimum the next staged ``select(..., state=state)`` re-ranks on.

    Returns a dict of device tensors on the current stream, no host synchronisation: track_clear [B,Kt] (the smallest distance to
    every track; +inf for a slot that is no usable track), track_min [B] (their minimum), both NaN for a plan that was not
    measured, has no finite pose or met a distance that is no number, and track_state [B,Kt] int32 (1 usable, 0 a length of 0,
    -1 not usable)."""
    import torch
    _lib.require_gpu("scene.plan_track_clearance")
    dev = _dev_of(device, x, tracks)
    tracks, track_t, track_len, track_size = _tracks_on_device(tracks, track_t, track_len, track_size, ego, dev)
    Bt, Kt, L = (int(v) for v in tracks.shape[:3])
    x = torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
    group = int(group)
    if x.dim() != 3 or x.shape[1] != 3 or group < 1 or int(x.shape[0]) != Bt * group:
        raise ValueError("expected x [B,3,N+1] with B = %d track blocks * group = %d, got %s" % (Bt, group, tuple(x.shape)))
    B, N1 = int(x.shape[0]), int(x.shape[2])

    def opt(a, shape, dt_=torch.float64):
        if a is None:
            return None
        a = torch.as_tensor(a, dtype=dt_, device=dev)
        a = a.expand(shape).contiguous() if a.dim() == 0 else a.contiguous()
        if tuple(a.shape) != shape:
            raise ValueError("expected shape %s, got %s" % (shape, tuple(a.shape)))
        return a
    dt, t0, x0 = opt(dt, (B,)), opt(t0, (B,)), opt(x0, (B, 3))
    variant, status = opt(variant, (B,), torch.int32), opt(status, (B,), torch.int32)
    K = Kt
    if score is not None:
        if not (isinstance(score, torch.Tensor) and score.device == dev and score.dtype == torch.float64 and score.is_contiguous() and
                score.dim() == 2 and score.shape[0] == B and score.shape[1] >= Kt):
            raise ValueError("score is folded in place: a contiguous float64 tensor [B,K] on %s with K >= Kt = %d" % (dev, Kt))
        K = int(score.shape[1])
    out = {"track_clear": torch.empty(B, Kt, dtype=torch.float64, device=dev),
           "track_min": torch.empty(B, dtype=torch.float64, device=dev),
           "track_state": torch.empty(B, Kt, dtype=torch.int32, device=dev)}
    ins = dict(track_x=tracks, track_t=track_t, track_len=track_len, track_size=track_size, t0=t0, dt=dt, x=x, x0=x0, variant=variant,
               status=status)
    d = _lib.ObcaPlanTracks().set(B=B, K=K, Kt=Kt, N=N1 - 1, L=L, group=group, n_sub=int(n_sub), ego=ego, score=score, **ins, **out)
    _lib.launch(_lib.load().obca_plan_tracks, ctypes.byref(d), dev=dev)
    _lib.keep_alive(out["track_clear"], tuple(ins.values()) + (score,), dev)       # the launch is asynchronous: see ``select``
    return out


def track_rows(tracks, track_t, track_len, Ts, N, pool_A=None, pool_b=None, pool_v=None, track_size=None, group=1, t0=None, margin=0.0,
               far=100.0, solver=None):
    """Timed tracks as the rows of an open-loop solve: ``pool_tracks`` with k = 0, measure=False and predict="track".  The
    caller's static pool -- pool_A [B,Ks,4,2], pool_b [B,Ks,4] and optionally pool_v [B,Ks,2], or None for Ks = 0 -- gets Kt
    slots appended, slot Ks + j being track j of block b // group at t0 (its rows grown by ``margin``, its chord velocity), and
    every track gets its rows at the N + 1 stage times t0 + kk Ts.  Tracks as ``plan_track_clearance`` takes them; ``solver``
    only names the device (None: the current one).

    Returns a dict of device tensors on the current stream, no host synchronisation: pool_A [B,K,4,2], pool_b [B,K,4] and pool_v
    [B,K,2] with K = Ks + Kt, stage_A [B,Kt,N+1,4,2], stage_b [B,Kt,N+1,4] and stage_ok [B,Kt] (``select``'s arguments of those
    names with stage_group = 1), track_state [B,Kt] (a track that is not usable is a spare at ``far``) and Ks."""
    import torch
    _lib.require_gpu("scene.track_rows")
    dev = solver.device if solver is not None else _dev_of(None, pool_A, tracks)
    ego = DEFAULT_EGO
    tracks, track_t, track_len, track_size = _tracks_on_device(tracks, track_t, track_len, track_size, ego, dev)
    Bt, Kt = int(tracks.shape[0]), int(tracks.shape[1])
    group = int(group)
    if group < 1:
        raise ValueError("group = %d: at least 1" % group)
    B = Bt * group
    full_A, full_b, full_v, Ks = _with_spare_slots(solver if solver is not None else _OnDevice(dev), B, pool_A, pool_b, pool_v, Kt,
                                                   float(far), "Kt")
    zeros = torch.zeros(B, 3, dtype=torch.float64, device=dev)
    out = pool_tracks(tracks, track_t, track_len, track_size, Ts, torch.zeros(B, dtype=torch.int32, device=dev), zeros, full_A, full_b,
                      full_v, int(N), group=group, t0=t0, predict="track", margin=margin, far=far, measure=False, device=dev)
    return {"pool_A": full_A, "pool_b": full_b, "pool_v": full_v, "stage_A": out["stage_A"], "stage_b": out["stage_b"],
            "stage_ok": out["stage_ok"], "track_state": out["track_state"], "Ks": Ks}


def solve_tracks(solver, variant, x0, u0, xref, pool_A, pool_b, Ts, tracks, track_t, track_len, track_size=None, group=1, t0=None,
                 margin=0.0, far=100.0, pool_v=None, term=None, params=None, rounds=2, n_sub=16, target=0.0, ego=DEFAULT_EGO):
    """``solve_scene`` among obstacles on timed tracks: the caller's static pool (pool_A [B,Ks,4,2], pool_b [B,Ks,4], pool_v
    [B,Ks,2] or None; None and None for Ks = 0) and Kt tracks (as ``plan_track_clearance`` takes them; a track's rectangle is
    grown by ``margin`` in the rows and measured without it), ``solver`` with m == [4] * n_sel, n_sel <= Ks + Kt.  Variants 6
    and 8 only: the tracks' clock needs a fixed step, stage kk being at t0 + kk Ts; obca_mpc4 reads stage 0's rows at every
    stage and is refused (a device tensor is taken at its word but for that: an instance whose word is 4 is masked).

    Round 0 is ``track_rows`` and the staged ``select`` on ``xref`` and ``x0``, then the solve.  Every solve is measured in
    three parts: ``plan_track_clearance`` on the plans with dt = Ts, which folds the distances to the TRACKS THEMSELVES into the
    running minimum of the tracked slots; the staged ``select`` with that state, which does the static slots and the
    re-ranking; and ``pool_clearance`` of the plans against the caller's Ks slots alone.  The figure that decides which plan is
    held and what ``clear`` says is min(static minimum, track_min), NaN where either is -- not the staged select's min_clear,
    which rests on rows interpolated between two stage times for the tracked slots.  The rest is ``solve_scene``'s: every later
    round solves only the instances whose selection changed, a later plan is held only if it is feasible and its figure larger.

    Runs on the current stream without host synchronisation.  Returns (result, info) as ``solve_scene`` does -- clear,
    min_clear, min_clear_first (round 0's true figure), rounds_used, sel (pool indices, Ks + j being track j), A_used, b_used --
    and track_min_clear [B], track_clear [B,Kt] and track_state [B,Kt] of the held plan."""
    import numpy as np
    import torch
    params = params or SolverParams()
    dev, N, m = solver.device, solver.N, solver.m
    n_sel = len(m)
    x0 = torch.as_tensor(x0, dtype=torch.float64, device=dev).contiguous()
    if x0.dim() != 2 or x0.shape[1] != 3:
        raise ValueError("expected x0 [B,3], got %s" % (tuple(x0.shape),))
    B = int(x0.shape[0])
    if isinstance(variant, torch.Tensor) and variant.is_cuda:
        variant = torch.where(variant.to(torch.int32) == 4, 0, variant.to(torch.int32)).to(torch.int32)
    else:
        v = np.asarray(variant.cpu() if isinstance(variant, torch.Tensor) else variant)
        if not np.all(np.isin(v, (0, 6, 8))):
            raise ValueError("variant %s: among tracks the solve is obca_mpc6 (6) or obca_mpc8 (8); obca_mpc4 reads stage 0's rows "
                             "at every stage" % (v.tolist(),))
        variant = torch.as_tensor(np.broadcast_to(v, (B,)).astype(np.int32), device=dev)
    on_dev = lambda t, shape, dt=torch.float64: solver._dev(t, shape, dt)
    variant = on_dev(variant, (B,), torch.int32)
    u0, xref = on_dev(u0, (B, 2)), on_dev(xref, (B, 3, N + 1))
    Ts = on_dev(torch.as_tensor(Ts, dtype=torch.float64).expand(B) if torch.as_tensor(Ts).dim() == 0 else Ts, (B,))
    if t0 is not None:
        t0 = on_dev(torch.as_tensor(t0, dtype=torch.float64).expand(B) if torch.as_tensor(t0).dim() == 0 else t0, (B,))
    term = on_dev(torch.zeros(B, 3) if term is None else term, (B, 3))
    tracks, track_t, track_len, track_size = _tracks_on_device(tracks, track_t, track_len, track_size, ego, dev)
    Kt, group = int(tracks.shape[1]), int(group)
    if group < 1 or int(tracks.shape[0]) * group != B:
        raise ValueError("B = %d instances are not %d track blocks of group = %d" % (B, int(tracks.shape[0]), group))
    rows = track_rows(tracks, track_t, track_len, Ts, N, pool_A, pool_b, pool_v, track_size=track_size, group=group, t0=t0,
                      margin=margin, far=far, solver=solver)
    full_A, full_b, full_v, Ks = rows["pool_A"], rows["pool_b"], rows["pool_v"], rows["Ks"]
    K = Ks + Kt
    if m != [4] * n_sel or n_sel > K:
        raise ValueError("solver.m = %s does not fit a pool of %d obstacles of 4 rows: expected [4] * n_sel, n_sel <= %d" % (m, K, K))
    cp = params.to_c() if isinstance(params, SolverParams) else params
    kw = dict(pool_v=full_v, Ts=Ts, n_sub=n_sub, ego=ego, device=dev, stage_A=rows["stage_A"], stage_b=rows["stage_b"],
              stage_ok=rows["stage_ok"], stage_group=1)
    static = (full_A[:, :Ks].contiguous(), full_b[:, :Ks].contiguous(), full_v[:, :Ks].contiguous()) if Ks > 0 else None

    state = select(full_A, full_b, xref, n_sel, x0=x0, variant=variant, **kw)

    def measure(r, var):
        """the three parts of a measurement of solve ``r``: (the staged select's dict, the tracks' dict, the true figure)"""
        tr = plan_track_clearance(r.xopt, tracks, track_t, track_len, Ts, track_size=track_size, t0=t0, variant=var, status=r.status,
                                  group=group, n_sub=n_sub, score=state["score"], ego=ego, device=dev)
        t = select(full_A, full_b, r.xopt, n_sel, variant=var, status=r.status, state=state, **kw)
        mc = tr["track_min"]
        if static is not None:
            _, smin = pool_clearance(r.xopt, static[0], static[1], pool_v=static[2], Ts=Ts, variant=var, n_sub=n_sub, ego=ego,
                                     device=dev)
            mc = torch.where(torch.isnan(smin) | torch.isnan(mc), float("nan"), torch.minimum(smin, mc))
        return t, tr, mc

    A_held, b_held, sel_held = state["A"], state["b"], state["sel"].clone()
    held = solver.solve(variant, x0, u0, xref, A_held, b_held, Ts, term, cp)
    t, tr, min_clear = measure(held, variant)
    first = min_clear.clone()
    track_min, track_clear = tr["track_min"], tr["track_clear"]
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
        t, tr, mc = measure(cur, var)
        better = mc > min_clear                                  # NaN (masked, infeasible) compares false
        for name in ("xopt", "uopt", "ts_opt", "status", "info"):
            h, c = getattr(held, name), getattr(cur, name)
            if h is not None:
                h.copy_(torch.where(better.reshape((B,) + (1,) * (h.dim() - 1)), c, h))
        min_clear = torch.where(better, mc, min_clear)
        track_min = torch.where(better, tr["track_min"], track_min)
        track_clear = torch.where(better[:, None], tr["track_clear"], track_clear)
        A_held = torch.where(better[:, None, None, None], A_cur, A_held)
        b_held = torch.where(better[:, None, None], b_cur, b_held)
        sel_held = torch.where(better[:, None], sel_cur, sel_held)
        var = t["variant_out"]
    held.iters.copy_(iters)
    return held, {"clear": min_clear >= float(target), "min_clear": min_clear, "min_clear_first": first,
                  "rounds_used": rounds_used, "sel": sel_held, "A_used": A_held, "b_used": b_held,
                  "track_min_clear": track_min, "track_clear": track_clear, "track_state": rows["track_state"]}


class PoolLoop:
    """B closed-loop rollouts over scene pools on one GPU, the counterpart of ``rollouts.DeviceRollouts`` for worlds of up to 64
    obstacles: ``reset()`` starts them, ``step()`` enqueues one receding-horizon step of every running rollout, ``run()`` all of
    them, ``read()`` returns state and history.  Everything runs on the current stream without host synchronisation.

    pool_A [B,K,E,2], pool_b [B,K,E] (the pool at the start; the loop moves its own copy), pool_v [B,K,2] or None; start [B,3],
    goal [B,2] (or [B,3] poses); path [B,3,path_max] and path_len [B] the routes to follow (``planner.plan_batch``'s outputs; a
    path_len outside 1 .. path_max starts the rollout FAILED); ``solver`` a ``BatchSolver`` with m == [E] * n_sel.
    variant: 4 (free time; default without pool_v) or 8 (fixed time; default with pool_v); 6 is refused, there is no terminal
    set here.  Ts [B] or a float is constant over the rollout: for variant 4 the reference's base step (the applied duration
    is the solve's ts_opt), for 8 the step itself -- choose it to fit the route's spacing.
    One step: ``select`` (n_sub = select_n_sub) of the pool as it is now around the window and the pose, the solve
    (rounds = 0: ``solver.solve`` on the selected rows; rounds >= 1: ``solve_scene``, whose held plan is applied), then
    obca_pool_loop_advance: the applied interval is measured against the whole pool at n_sub + 1 samples (n_sub = 0: not
    measured) and a rollout whose interval comes closer than ``clearance`` ends with flag "collision" (clearance=None:
    measured, never stopped -- the C call wants a finite threshold and gets -1e300).  A rollout whose pool or poses ``select``
    cannot use is masked and ends FAILED with status -5."""

    def __init__(self, solver, pool_A, pool_b, start, goal, path, path_len, Ts, pool_v=None, variant=None, params=None,
                 max_steps=30, rounds=0, select_n_sub=1, n_sub=8, clearance=None, goal_tol2=0.1, ego=DEFAULT_EGO):
        import torch
        _lib.require_gpu("scene.PoolLoop")
        self.torch, self.lib, self.solver = torch, _lib.load(), solver
        dev = self.device = solver.device
        f64 = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous()
        self.pool_A, self.pool_b0 = f64(pool_A), f64(pool_b)
        if self.pool_A.dim() != 4 or self.pool_b0.dim() != 3 or tuple(self.pool_A.shape) != tuple(self.pool_b0.shape) + (2,):
            raise ValueError("expected pool_A [B,K,E,2], pool_b [B,K,E]")
        B, K, E = (int(v) for v in self.pool_b0.shape)
        self.B, self.K, self.E, self.N, self.n_sel = B, K, E, solver.N, len(solver.m)
        if solver.m != [E] * self.n_sel or self.n_sel > K or self.n_sel < 1:
            raise ValueError("solver.m = %s does not fit a pool of %d obstacles of %d rows: expected [%d] * n_sel, n_sel <= %d" %
                             (solver.m, K, E, E, K))
        self.pool_v = None if pool_v is None else solver._dev(pool_v, (B, K, 2))
        self.variant = int((4 if pool_v is None else 8) if variant is None else variant)
        if self.variant not in (4, 8):
            raise ValueError("variant %d: the closed loop over pools runs obca_mpc4 (4) or obca_mpc8 (8); there is no terminal set "
                             "for 6" % self.variant)
        self.start = solver._dev(start, (B, 3))
        goal = f64(goal)
        if goal.dim() != 2 or goal.shape[0] != B or goal.shape[1] not in (2, 3):
            raise ValueError("expected goal [B,2] or [B,3], got %s" % (tuple(goal.shape),))
        self.goal = goal[:, :2].contiguous()
        self.path = f64(path)
        if self.path.dim() != 3 or self.path.shape[0] != B or self.path.shape[1] != 3 or self.path.shape[2] < 1:
            raise ValueError("expected path [B,3,path_max], got %s" % (tuple(self.path.shape),))
        self.path_len = solver._dev(path_len, (B,), torch.int32)
        Ts = torch.as_tensor(Ts, dtype=torch.float64, device=dev)
        self.Ts = solver._dev(Ts.expand(B) if Ts.dim() == 0 else Ts, (B,))
        self.params = params or SolverParams()
        self._cparams = self.params.to_c() if isinstance(self.params, SolverParams) else self.params
        self.max_steps, self.rounds, self.select_n_sub, self.n_sub = int(max_steps), int(rounds), int(select_n_sub), int(n_sub)
        self.clearance = NEVER_STOP if clearance is None else float(clearance)
        self.goal_tol2, self.ego = float(goal_tol2), tuple(float(v) for v in ego)
        S, N, n_sel = self.max_steps, self.N, self.n_sel
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        i = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
        self.x0, self.u0, self.pool_b, self.k, self.flags = f(B, 3), f(B, 2), f(B, K, E), i(B), i(B)
        self.hist = {"x_closed": f(B, S + 1, 3), "u_closed": f(B, S, 2), "T_closed": f(B, S), "status": i(B, S), "iters": i(B, S),
                     "clear": f(B, S), "sel": i(B, S, n_sel)}
        self.xref, self.variant_out = f(B, 3, N + 1), i(B)
        self.term = f(B, 3)
        self._held = None                                    # the solve's outputs, allocated by the first solve
        self._last = (None, None)                            # (result, selection) of the last step
        self._desc = _lib.ObcaPoolLoop().set(
            B=B, K=K, E=E, N=N, n_sel=n_sel, path_max=int(self.path.shape[2]), max_steps=S, variant=self.variant, n_sub=self.n_sub,
            clearance=self.clearance, goal_tol2=self.goal_tol2, ego=self.ego, pool_A=self.pool_A, pool_v=self.pool_v, goal=self.goal,
            path=self.path, path_len=self.path_len, x0=self.x0, u0=self.u0, pool_b=self.pool_b, k=self.k, flags=self.flags,
            x_closed=self.hist["x_closed"], u_closed=self.hist["u_closed"], T_closed=self.hist["T_closed"],
            status_hist=self.hist["status"], iters_hist=self.hist["iters"], clear_hist=self.hist["clear"], sel_hist=self.hist["sel"],
            xref_out=self.xref, variant_out=self.variant_out)
        self.x_prev = None                                   # a loop with an after-step hook: made by the first reset
        self.steps_enqueued = 0
        self.reset()

    # ---- what a loop with a step call of its own between two solves overrides (``FleetLoop``, ``TrackLoop``)
    def _staged(self):
        """the stage_* keyword arguments of ``select``, or {} for obca_scene_select"""
        return {}

    def _after_reset(self):
        """called at the end of ``reset()``, x_prev = x0; the first time, it also makes the loop's own buffers and descriptor"""

    def _after_step(self, measure, step):
        """called after obca_pool_loop_advance of every step: (1, the step's index), or (0, 0) beyond the cap, where nobody steps"""

    def _hooked(self):
        return type(self)._after_step is not PoolLoop._after_step

    def _tensors(self):
        own = [self.pool_A, self.pool_b0, self.pool_v, self.start, self.goal, self.path, self.path_len, self.Ts, self.x0, self.u0,
               self.pool_b, self.k, self.flags, self.xref, self.variant_out, self.term, self.x_prev] + list(self.hist.values())
        r, sel = self._last                                  # the last solve's outputs: the descriptor still points at them
        if r is not None:
            own += [r.xopt, r.uopt, r.ts_opt, r.status, r.iters, r.info, sel]
        return [t for t in own if t is not None]

    def _on_stream(self):
        """the launches are asynchronous: every tensor they touch is recorded on the stream they run on (see ``select``)"""
        _lib.keep_alive(self, self._tensors(), self.device)

    def _advance(self, solved):
        _lib.launch(self.lib.obca_pool_loop_advance, ctypes.byref(self._desc), int(solved), dev=self.device)

    def reset(self):
        self._on_stream()
        self.x0.copy_(self.start)
        self.pool_b.copy_(self.pool_b0)
        self._advance(0)
        self.steps_enqueued = 0
        if self._hooked():
            first = self.x_prev is None                      # the reset the constructor ends with
            if first:
                self.x_prev = self.torch.zeros(self.B, 3, dtype=self.torch.float64, device=self.device)
            self.x_prev.copy_(self.x0)
            self._after_reset()
            if first:
                self._on_stream()

    def _select(self):
        return select(self.pool_A, self.pool_b, self.xref, self.n_sel, pool_v=self.pool_v, Ts=self.Ts, x0=self.x0,
                      variant=self.variant_out, n_sub=self.select_n_sub, ego=self.ego, device=self.device, **self._staged())

    def _step(self):
        torch, solver, d = self.torch, self.solver, self._desc
        if self._hooked():
            self.x_prev.copy_(self.x0)
        if self.rounds == 0:
            s = self._select()
            var = torch.where(s["ok"] != 0, self.variant_out, 0).to(torch.int32)
            self._held = solver.solve(var, self.x0, self.u0, self.xref, s["A"], s["b"], self.Ts, self.term, self._cparams,
                                      out=self._held)
            r, sel = self._held, s["sel"]
        else:
            r, info = solve_scene(solver, self.variant_out, self.x0, self.u0, self.xref, self.pool_A, self.pool_b, self.Ts,
                                  pool_v=self.pool_v, term=self.term, params=self._cparams, rounds=self.rounds,
                                  n_sub=max(self.n_sub, 1), ego=self.ego)
            sel = info["sel"]
        self._last = (r, sel)                                # alive until the next step replaces them
        d.set(status=r.status, iters=r.iters, ts_opt=r.ts_opt, xopt=r.xopt, uopt=r.uopt, sel=sel)
        self._advance(1)
        self.steps_enqueued += 1
        if self.steps_enqueued <= self.max_steps:
            self._after_step(1, self.steps_enqueued - 1)
        else:                                                # beyond the cap nobody steps
            self._after_step(0, 0)

    def step(self):
        self._on_stream()
        self._step()

    def run(self, n_steps=None):
        self._on_stream()
        for _ in range(self.max_steps if n_steps is None else int(n_steps)):
            self._step()
        return self

    def read(self):
        """copies, as device tensors on the current stream: x_closed [B,S+1,3] (NaN beyond the driven knots), u_closed [B,S,2],
        T_closed [B,S], status / iters [B,S], clear [B,S] (+inf where no interval was measured), sel [B,S,n_sel] (-1 where no
        step was solved), steps [B], flags [B], pool_b [B,K,E] (the pool now), x0 [B,3], min_clear [B] (the smallest measured
        interval)"""
        out = {k: v.clone() for k, v in self.hist.items()}
        out.update(steps=self.k.clone(), flags=self.flags.clone(), pool_b=self.pool_b.clone(), x0=self.x0.clone(),
                   min_clear=self.hist["clear"].min(dim=1).values)
        return out


class FleetLoop(PoolLoop):
    """G worlds of V cars each: ``PoolLoop`` whose rollouts share worlds.  Rollout b = g V + a is car a of world g (B = G V, a
    multiple of V); the caller gives the static part of every pool -- pool_A [B,Ks,4,2], pool_b [B,Ks,4] and optionally pool_v
    [B,Ks,2], or None for Ks = 0 -- and the loop appends V agent slots, slot Ks + j being "car j of my world": the rectangle of
    that car where it stands (grown by ``margin``), translating with its last applied speed along its heading
    (predict="velocity") or standing (predict="static"); a car that has ended is parked where it stands and stays an obstacle.
    see="all": every other car is an obstacle; see="lower": only the cars of lower index are (prioritised planning: car 0
    yields to nobody).  A spare slot (the car itself, a car not seen, a car without a pose) is ``grid_pool``'s spare at ``far``.
    predict="plan": a car that has just applied a feasible plan is predicted by that plan -- after obca_fleet_step,
    obca_fleet_tracks turns every such plan into rows per stage (knot kk + 1 is stage kk of the next solve, the last stage
    extrapolated) and the next ``select`` is obca_scene_select_staged, which reads those rows for the agent slots in place of
    the translating rectangle.  The pool slots themselves, and with them obca_pool_loop_advance's ``clear``, stay the velocity
    prediction, which is also the fallback for a car without a usable plan (ended, masked, infeasible, or the first step).
    Plans of cars of lower index are commitments under see="lower"; under see="all" every car plans against plans that are
    being revised against it, which can be worse than velocities.  rounds >= 1 is refused with "plan":
    ``solve_scene`` is not staged.

    The fleet's time is synchronous: variant 8 only, and Ts must be one value per world -- checked here when Ts is a float or a
    host array; a device tensor is taken at its word (checking it would cost a host synchronisation).
    One step: x_prev = x0, ``PoolLoop``'s step unchanged (select, solve, obca_pool_loop_advance: its ``clear`` measures a car
    against the PREDICTION of the others), then obca_fleet_step (arithmetic and serial definition in csrc/obca_fleet_core.h):
    the smallest distance of every car that stepped to every other car of its world over the interval both actually drove
    (agent_n_sub + 1 samples; 0: not measured), a car closer than ``agent_clearance`` ends with flag "collision"
    (None: measured, never stopped), and the agent slots are rewritten from the poses, inputs and flags as they are now.
    ``read()`` adds agent_clear [B,S] (+inf where nothing was measured) and agent_min_clear [B].

        solver = BatchSolver(5, [4] * 3, B)                       # two corridor walls and the nearest other car
        loop = FleetLoop(solver, 2, walls_A, walls_b, start, goal, path, path_len, Ts=1.5, see="lower").run()
        out = loop.read()                                         # out["flags"], out["agent_min_clear"], out["x_closed"], ...
    """

    def __init__(self, solver, V, pool_A, pool_b, start, goal, path, path_len, Ts, pool_v=None, see="all", predict="velocity",
                 margin=0.0, far=100.0, agent_clearance=None, agent_n_sub=8, **kw):
        import numpy as np
        import torch
        _lib.require_gpu("scene.FleetLoop")
        V = self.V = int(V)
        if see not in _lib.FLEET_SEE or (predict not in _lib.FLEET_PREDICT and predict != "plan"):
            raise ValueError("see is one of %s and predict one of %s" % (sorted(_lib.FLEET_SEE), sorted(_lib.FLEET_PREDICT) + ["plan"]))
        if predict == "plan" and int(kw.get("rounds", 0)) >= 1:
            raise ValueError('predict="plan" needs rounds = 0: solve_scene is not staged')
        if kw.get("variant") not in (None, 8):
            raise ValueError("variant %r: a fleet's time is synchronous, the loop runs obca_mpc8 (8) only" % (kw["variant"],))
        kw["variant"] = 8
        start = torch.as_tensor(start, dtype=torch.float64, device=solver.device)
        B = int(start.shape[0])
        if V < 1 or V > 16 or B % V != 0:
            raise ValueError("B = %d rollouts are no whole number of worlds of V = %d cars (1 <= V <= 16)" % (B, V))
        self.G = B // V
        # the agent slots start as spares; obca_fleet_step writes them at every reset and after every step
        full_A, full_b, full_v, self.Ks = _with_spare_slots(solver, B, pool_A, pool_b, pool_v, V, float(far), "V")
        if not isinstance(Ts, torch.Tensor) or not Ts.is_cuda:
            t = np.asarray(Ts.cpu() if isinstance(Ts, torch.Tensor) else Ts, dtype=float)
            if t.ndim != 0 and (t.shape != (B,) or not np.all(t.reshape(self.G, V) == t.reshape(self.G, V)[:, :1])):
                raise ValueError("Ts must be one value per world: [B] with the same word for the V cars of a world, or a float")
        self.see, self.predict, self.margin, self.far = see, predict, float(margin), float(far)
        self.agent_clearance = NEVER_STOP if agent_clearance is None else float(agent_clearance)
        self.agent_n_sub = int(agent_n_sub)
        self._fdesc = None                                   # made by the first reset, which PoolLoop's constructor ends with
        super().__init__(solver, full_A, full_b, start, goal, path, path_len, Ts, pool_v=full_v, **kw)

    def _make_fleet(self):
        torch = self.torch
        self.agent_clear = torch.zeros(self.B, self.max_steps, dtype=torch.float64, device=self.device)
        # "plan" is the loop's word: the C call writes the velocity prediction, the tracks replace it where there is a plan
        self._fdesc = _lib.ObcaFleet().set(
            G=self.G, V=self.V, Ks=self.Ks, N=self.N, max_steps=self.max_steps, n_sub=self.agent_n_sub, see=_lib.FLEET_SEE[self.see],
            predict=_lib.FLEET_PREDICT["velocity" if self.predict == "plan" else self.predict], clearance=self.agent_clearance,
            margin=self.margin, far=self.far, ego=self.ego, x_prev=self.x_prev, x0=self.x0, u0=self.u0, k=self.k, flags=self.flags,
            pool_A=self.pool_A, pool_b=self.pool_b, pool_v=self.pool_v, agent_clear_hist=self.agent_clear, xref_out=self.xref,
            variant_out=self.variant_out)
        if self.predict == "plan":
            G, V, N1 = self.G, self.V, self.N + 1
            self.track_A = torch.zeros(G, V, N1, 4, 2, dtype=torch.float64, device=self.device)
            self.track_b = torch.zeros(G, V, N1, 4, dtype=torch.float64, device=self.device)
            self.track_ok = torch.zeros(self.B, V, dtype=torch.int32, device=self.device)
            self._tdesc = _fleet_tracks_desc(G, V, self.N, self.see, self.margin, self.far, self.ego, x0=self.x0, flags=self.flags,
                                             k=self.k, track_A=self.track_A, track_b=self.track_b, track_ok=self.track_ok)

    def _tensors(self):
        own = super()._tensors()
        if self._fdesc is not None:
            own.append(self.agent_clear)
            if self.predict == "plan":
                own += [self.track_A, self.track_b, self.track_ok]
        return own

    def _staged(self):
        plan = self.predict == "plan"
        return dict(stage_A=self.track_A, stage_b=self.track_b, stage_ok=self.track_ok, stage_group=self.V) if plan else {}

    def _fleet_step(self, measure, step):
        self._fdesc.set(step=int(step))
        _lib.launch(self.lib.obca_fleet_step, ctypes.byref(self._fdesc), int(measure), dev=self.device)

    def _after_reset(self):
        if self._fdesc is None:
            self._make_fleet()
        self.agent_clear.fill_(float("inf"))
        self._fleet_step(0, 0)
        if self.predict == "plan":
            self.track_ok.zero_()                            # no plan yet: the first select is the velocity loop's

    def _tracks(self, step):
        """obca_fleet_tracks on the solve just applied (``self._last``), after obca_fleet_step on the same stream"""
        r = self._last[0]
        self._tdesc.set(step=int(step), xopt=r.xopt, status=r.status)
        _lib.launch(self.lib.obca_fleet_tracks, ctypes.byref(self._tdesc), dev=self.device)

    def _after_step(self, measure, step):
        self._fleet_step(measure, step)
        if self.predict == "plan":
            self._tracks(self.steps_enqueued - 1)            # beyond the cap k == step + 1 fails: every mask word 0

    def read(self):
        """``PoolLoop.read()``'s dict and agent_clear [B,S] (the smallest distance to another car of the world over every
        interval the car drove, +inf where nothing was measured), agent_min_clear [B]"""
        out = super().read()
        out.update(agent_clear=self.agent_clear.clone(), agent_min_clear=self.agent_clear.min(dim=1).values)
        return out


class TrackLoop(PoolLoop):
    """``PoolLoop`` whose worlds also hold obstacles that follow timed tracks: recorded or scripted road users that turn, brake,
    stop or set off later.  The caller's pool -- pool_A [B,Ks,4,2], pool_b [B,Ks,4] and optionally pool_v [B,Ks,2], or None for
    Ks = 0 -- is the static part; the loop appends Kt slots, slot Ks + j being track j of the rollout's block: tracks
    [Bt,Kt,L,3] poses (x, y, heading; unwrap the headings), track_t [Bt,Kt,L] strictly increasing times, track_len [Bt,Kt]
    (0: the slot is a spare), track_size [Bt,Kt,4] in ego's convention (None: the ego's), rollout b of B = Bt * group reading
    block b // group.  Before its first time an obstacle stands at its first knot, after its last it parks at the last one.
    The clock of rollout b is t0[b] + k Ts[b] (t0 None: 0).  Tracks given as host arrays are checked here and an unusable one
    raises; device tensors are taken at their word and an unusable track becomes a spare (``read()``'s track_state -1).

    predict="track": the next solve reads the track's rows at its own stage times (obca_scene_select_staged, stage_group 1);
    "velocity": the rectangle now, translating at the chord velocity of the next step; "static": the rectangle now.  The pool
    slots themselves, and with them obca_pool_loop_advance's ``clear``, are the chord prediction under every word; what the
    car really kept from the tracked obstacles is ``read()``'s track_clear [B,S], measured against the tracks themselves at
    track_n_sub + 1 samples per driven interval (0: not measured); a car closer than ``track_clearance`` ends with flag
    "collision" (None: measured, never stopped).  Variant 8 only: the clock needs a fixed step.  rounds >= 1 is refused under
    "track": ``solve_scene`` is not staged.

    One step: x_prev = x0, ``PoolLoop``'s step, then obca_pool_tracks (arithmetic and serial definition in
    csrc/obca_pool_tracks_core.h) with measure = 1; ``reset()`` calls it with measure = 0.

        loop = TrackLoop(solver, walls_A, walls_b, start, goal, path, path_len, 1.5, tracks, track_t, track_len, margin=0.1).run()
        out = loop.read()                                         # out["flags"], out["track_min_clear"], out["track_state"], ...
    """

    def __init__(self, solver, pool_A, pool_b, start, goal, path, path_len, Ts, tracks, track_t, track_len, track_size=None,
                 group=1, t0=None, predict="track", margin=0.0, far=100.0, track_clearance=None, track_n_sub=8, pool_v=None, **kw):
        import numpy as np
        import torch
        _lib.require_gpu("scene.TrackLoop")
        dev = solver.device
        if predict not in _lib.TRACK_PREDICT:
            raise ValueError("predict is one of %s" % sorted(_lib.TRACK_PREDICT))
        if predict == "track" and int(kw.get("rounds", 0)) >= 1:
            raise ValueError('predict="track" needs rounds = 0: solve_scene is not staged')
        if kw.get("variant") not in (None, 8):
            raise ValueError("variant %r: the tracks' clock needs a fixed step, the loop runs obca_mpc8 (8) only" % (kw["variant"],))
        kw["variant"] = 8
        f64 = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous()
        on_host = lambda a: not (isinstance(a, torch.Tensor) and a.is_cuda)
        shape = tuple(np.shape(tracks) if on_host(tracks) else tracks.shape)
        if len(shape) != 4 or shape[3] != 3 or shape[1] < 1 or shape[2] < 1:
            raise ValueError("expected tracks [Bt,Kt,L,3], got %s" % (shape,))
        Bt, Kt, L = shape[:3]
        if track_size is None:
            track_size = np.tile(np.asarray(kw.get("ego", DEFAULT_EGO), float), (Bt, Kt, 1))
        for a, want in ((track_t, (Bt, Kt, L)), (track_len, (Bt, Kt)), (track_size, (Bt, Kt, 4))):
            if tuple(np.shape(a) if on_host(a) else a.shape) != want:
                raise ValueError("expected shape %s next to tracks %s, got %s" % (want, shape, tuple(np.shape(a) if on_host(a) else a.shape)))
        if all(on_host(a) for a in (tracks, track_t, track_len, track_size)):
            check_tracks(tracks, track_t, track_len, track_size)
        start = torch.as_tensor(start, dtype=torch.float64, device=dev)
        B, group = int(start.shape[0]), int(group)
        if group < 1 or Bt * group != B:
            raise ValueError("B = %d rollouts are not %d track blocks of group = %d" % (B, Bt, group))
        # the tracked slots start as spares; obca_pool_tracks writes them at every reset and after every step
        full_A, full_b, full_v, self.Ks = _with_spare_slots(solver, B, pool_A, pool_b, pool_v, Kt, float(far), "Kt")
        self.Kt, self.L, self.group, self.predict, self.margin, self.far = Kt, L, group, predict, float(margin), float(far)
        self.tracks, self.track_t, self.track_size = f64(tracks), f64(track_t), f64(track_size)
        self.track_len = torch.as_tensor(track_len, dtype=torch.int32, device=dev).contiguous()
        self.t0 = None if t0 is None else solver._dev(torch.as_tensor(t0, dtype=torch.float64).expand(B)
                                                      if torch.as_tensor(t0).dim() == 0 else t0, (B,))
        self.track_clearance = NEVER_STOP if track_clearance is None else float(track_clearance)
        self.track_n_sub = int(track_n_sub)
        self._tdesc = None                                   # made by the first reset, which PoolLoop's constructor ends with
        super().__init__(solver, full_A, full_b, start, goal, path, path_len, Ts, pool_v=full_v, **kw)

    def _make_tracks(self):
        torch, dev, B, Kt, N1 = self.torch, self.device, self.B, self.Kt, self.N + 1
        self.track_clear = torch.zeros(B, self.max_steps, dtype=torch.float64, device=dev)
        self.stage_A = torch.zeros(B, Kt, N1, 4, 2, dtype=torch.float64, device=dev)
        self.stage_b = torch.zeros(B, Kt, N1, 4, dtype=torch.float64, device=dev)
        self.stage_ok = torch.zeros(B, Kt, dtype=torch.int32, device=dev)
        self.track_state = torch.zeros(B, Kt, dtype=torch.int32, device=dev)
        self._tdesc = _pool_tracks_desc(
            B, self.K, Kt, self.N, self.L, self.group, self.max_steps, self.track_n_sub, self.predict, self.track_clearance,
            self.margin, self.far, self.ego, track_x=self.tracks, track_t=self.track_t, track_len=self.track_len,
            track_size=self.track_size, t0=self.t0, Ts=self.Ts, x_prev=self.x_prev, x0=self.x0, k=self.k, flags=self.flags,
            pool_A=self.pool_A, pool_b=self.pool_b, pool_v=self.pool_v, stage_A=self.stage_A, stage_b=self.stage_b,
            stage_ok=self.stage_ok, track_state=self.track_state, track_clear_hist=self.track_clear, xref_out=self.xref,
            variant_out=self.variant_out)

    def _tensors(self):
        own = super()._tensors() + [self.tracks, self.track_t, self.track_len, self.track_size]
        if self.t0 is not None:
            own.append(self.t0)
        if self._tdesc is not None:
            own += [self.track_clear, self.stage_A, self.stage_b, self.stage_ok, self.track_state]
        return own

    def _staged(self):
        track = self.predict == "track"
        return dict(stage_A=self.stage_A, stage_b=self.stage_b, stage_ok=self.stage_ok, stage_group=1) if track else {}

    def _pool_tracks(self, measure, step):
        self._tdesc.set(step=int(step))
        _lib.launch(self.lib.obca_pool_tracks, ctypes.byref(self._tdesc), int(measure), dev=self.device)

    _after_step = _pool_tracks

    def _after_reset(self):
        if self._tdesc is None:
            self._make_tracks()
        self.track_clear.fill_(float("inf"))
        self._pool_tracks(0, 0)

    def read(self):
        """``PoolLoop.read()``'s dict and track_clear [B,S] (the smallest distance to a tracked obstacle over every interval the
        car drove, measured against the tracks themselves; +inf where nothing was measured), track_min_clear [B] and
        track_state [B,Kt] (1 usable, 0 a length of 0, -1 not usable: a spare)"""
        out = super().read()
        out.update(track_clear=self.track_clear.clone(), track_min_clear=self.track_clear.min(dim=1).values,
                   track_state=self.track_state.clone())
        return out


def drive_maps(solver, grids, start_cells, goal_cells, start, goal, Ts, K, pad=None, far=100.0, dilation=1, path_max=None, **loop):
    """B occupancy grids and B start/goal pairs -> B driven trajectories, each measured against its whole map, on the current
    stream without host synchronisation: ``grid_pool(grids, K, pad=pad, far=far)`` gives the pools,
    ``openloop.route_search(grids, start_cells, goal_cells, dilation=dilation)`` the routes (the dilated map's where it has
    one, else the plain map's), ``PoolLoop(solver, pool_A, pool_b, start, goal, path, path_len, Ts, **loop).run()`` drives
    them.  Arguments as ``solve_maps``; ``loop`` are ``PoolLoop``'s keyword arguments.  Resolution 1 only.

    An instance whose pool is incomplete (grid_pool's ok == 0) or that has no route (path_len < 1) is masked on the device --
    its path_len becomes 0, so it starts FAILED and is never solved -- and reported, never raised on.  Returns (loop, info):
    the ``PoolLoop`` after its run (``loop.read()`` gives the histories) and a dict of device tensors: pool (grid_pool's dict),
    path, path_len (as driven: 0 where masked), pool_ok [B] and source [B] (2 = the dilated route, 1 = the plain route,
    0 = none)."""
    import torch
    from .openloop import route_search
    dev = solver.device
    if not isinstance(grids, torch.Tensor):                  # one upload for the cover and both searches
        import numpy as np
        grids = torch.as_tensor(np.ascontiguousarray(grids), device=dev)
    pool = grid_pool(grids, K, resolution=1.0, pad=pad, far=far, device=dev)
    path, plen, src = route_search(grids, start_cells, goal_cells, dilation=dilation, path_max=path_max, device=dev)
    source = torch.where(plen >= 1, src, 0).to(torch.int32)
    plen = torch.where((pool["ok"] != 0) & (source != 0), plen, 0).to(torch.int32)
    lp = PoolLoop(solver, pool["pool_A"], pool["pool_b"], start, goal, path, plen, Ts, **loop).run()
    return lp, {"pool": pool, "path": path, "path_len": plen, "pool_ok": pool["ok"], "source": source}
