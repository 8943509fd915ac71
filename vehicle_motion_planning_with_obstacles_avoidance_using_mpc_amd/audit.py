"""Collision audit on the GPU: true clearance of batched plans and closed-loop rollouts, in fp64.

``plan_clearance`` measures ``BatchSolver`` outputs against the rows the solver was given (obca_plan_clearance), at the
knots; ``plan_sweep`` measures them between the knots as well and bounds the continuous motion from below
(obca_plan_sweep), ``plan_summary`` turns a sweep into counts; ``plan_tighten`` is one round of the clearance repair
(obca_plan_tighten: measure, grow the rows where the plan comes too close; the loop around it is ``clear.solve_clear``);
``DeviceRollouts.audit`` / ``RolloutCohorts.audit`` measure closed-loop rollouts against the static obstacles and every
present moving box, between the knots too (obca_rollouts_audit); ``summary`` turns an audit into counts.  Read-only: no
solver or rollout state changes.  Geometry and the certified bound: csrc/obca_audit_core.h.
"""
import ctypes

import numpy as np

from . import _lib
from .solver import DEFAULT_EGO


def _device_tensor(a, dtype, device):
    import torch
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a, dtype=dtype, device=device).contiguous()


def _plan_batch(x, A, b, m, ego, variant, device, status=None, tighten=False):
    """The batch the three plan calls share, on the device: resolves the device (``device``, else x's if x is a device
    tensor, else the current one), moves and reshapes x, A, b, variant (None: NULL unless ``tighten``) and, for
    ``tighten``, status.  Returns (dev, B, N1, m, keep, head): head = the leading arguments of the C call up to b, keep = the
    tensors head points into, to be held until the call is made."""
    import torch
    dev = torch.device(device) if device is not None else (x.device if isinstance(x, torch.Tensor) and x.is_cuda else
                                                           torch.device("cuda", torch.cuda.current_device()))
    m = [int(v) for v in m]
    x = _device_tensor(x, torch.float64, dev)
    B, N1, M = int(x.shape[0]), int(x.shape[2]), sum(m)
    x = x.reshape(B, 3, N1)
    A = _device_tensor(A, torch.float64, dev).reshape(B, N1, M, 2)
    b = _device_tensor(b, torch.float64, dev).reshape(B, N1, M)
    ints = [None if variant is None and not tighten else _device_tensor(variant, torch.int32, dev).reshape(B)]
    if tighten:
        ints.append(_device_tensor(status, torch.int32, dev).reshape(B))
    ego_c = (ctypes.c_double * 4)(*[float(v) for v in ego])
    m_c = (ctypes.c_int32 * max(len(m), 1))(*m)
    keep = ints + [x, A, b]
    head = [ego_c, len(m), m_c, N1 - 1, B] + [_lib.ptr(t) for t in keep]
    return dev, B, N1, m, keep, head


def plan_clearance(x, A, b, m, ego=DEFAULT_EGO, variant=None, per_stage=False, device=None):
    """x [B,3,N+1], A [B,N+1,M,2], b [B,N+1,M] (torch tensors or numpy arrays), m: rows per obstacle; variant [B] or None
    (4: every stage against stage 0's rows, as obca_mpc4 reads them).  Returns a dict of device tensors on the current
    stream: min_clear [B], arg_stage [B], arg_obst [B] and, with per_stage, stage_obst [B,N+1,n_obs]."""
    import torch
    dev, B, N1, m, keep, head = _plan_batch(x, A, b, m, ego, variant, device)
    out = {"min_clear": torch.empty(B, dtype=torch.float64, device=dev),
           "arg_stage": torch.empty(B, dtype=torch.int32, device=dev),
           "arg_obst": torch.empty(B, dtype=torch.int32, device=dev)}
    if per_stage:
        out["stage_obst"] = torch.empty(B, N1, len(m), dtype=torch.float64, device=dev)
    p = _lib.ptr
    _lib.launch(_lib.load().obca_plan_clearance, *head, p(out["min_clear"]), p(out["arg_stage"]), p(out["arg_obst"]),
                p(out.get("stage_obst")), dev=dev)
    return out


def plan_sweep(x, A, b, m, n_sub=16, ego=DEFAULT_EGO, variant=None, per_interval=False, device=None):
    """plan_clearance's arguments; every interval stage s -> s + 1 is measured at n_sub + 1 samples (n_sub = 1: the knots
    only), pose and obstacle rows interpolated linearly.  Returns a dict of device tensors on the current stream:
    min_clear, lower_bound (certified for translating obstacles, else NaN), arg_interval, arg_obst, first_collision [B]
    and, with per_interval, interval_min [B,N]."""
    import torch
    dev, B, N1, m, keep, head = _plan_batch(x, A, b, m, ego, variant, device)
    out = {"min_clear": torch.empty(B, dtype=torch.float64, device=dev),
           "lower_bound": torch.empty(B, dtype=torch.float64, device=dev),
           "arg_interval": torch.empty(B, dtype=torch.int32, device=dev),
           "arg_obst": torch.empty(B, dtype=torch.int32, device=dev),
           "first_collision": torch.empty(B, dtype=torch.int32, device=dev)}
    if per_interval:
        out["interval_min"] = torch.empty(B, max(N1 - 1, 0), dtype=torch.float64, device=dev)
    p = _lib.ptr
    _lib.launch(_lib.load().obca_plan_sweep, *head, int(n_sub), p(out["min_clear"]), p(out["lower_bound"]), p(out["arg_interval"]),
                p(out["arg_obst"]), p(out["first_collision"]), p(out.get("interval_min")), dev=dev)
    return out


def plan_tighten(x, A, b, m, variant, status, grow=None, b_out=None, n_sub=16, certified=False, target=0.0, gain=1.0,
                 grow_max=2.0, ego=DEFAULT_EGO, device=None):
    """One round of the clearance repair (obca_plan_tighten): plan_sweep's arguments plus status [B] of the solve and the
    in/out state grow [B,N+1,n_obs] (None: zeros).  Every feasible plan (variant != 0, status 0 / 1) is measured per
    interval and obstacle against A / b; where it comes closer than target, that obstacle grows at the two stages next to
    the interval by gain times the shortfall, up to grow_max.  Returns a dict of device tensors on the current stream: grow
    (the tensor passed in, updated in place), b_out [B,N+1,M] = b + grow |a| (the rows to solve again with; written into
    b_out if given, which must not be b), variant_out [B] (variant where grow rose, else 0: the variant argument of the
    next solve) and min_clear [B] (NaN: not measured, or not finite)."""
    import torch
    dev, B, N1, m, keep, head = _plan_batch(x, A, b, m, ego, variant, device, status, tighten=True)
    M = sum(m)
    if grow is None:
        grow = torch.zeros(B, N1, len(m), dtype=torch.float64, device=dev)
    if b_out is None:
        b_out = torch.empty(B, N1, M, dtype=torch.float64, device=dev)
    for t, shape in ((grow, (B, N1, len(m))), (b_out, (B, N1, M))):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and
                tuple(t.shape) == shape):
            raise ValueError("grow / b_out: expected a contiguous float64 device tensor of shape %s" % (shape,))
    out = {"grow": grow, "b_out": b_out, "variant_out": torch.empty(B, dtype=torch.int32, device=dev),
           "min_clear": torch.empty(B, dtype=torch.float64, device=dev)}
    p = _lib.ptr
    _lib.launch(_lib.load().obca_plan_tighten, *head, int(n_sub), int(bool(certified)), float(target), float(gain), float(grow_max),
                p(grow), p(b_out), p(out["variant_out"]), p(out["min_clear"]), dev=dev)
    return out


def plan_summary(sweep, knots=None):
    """counts and worst values of a plan sweep (plan_sweep): plans with a sampled collision, with a negative certified
    bound, with a bound that is not certified (NaN) and, given the knot audit of the same plans (plan_clearance), plans
    that are clear at every knot and collide between them.  Plans that measure NaN are counted apart and are not the worst."""
    g = lambda d, k: np.asarray(d[k].cpu() if hasattr(d[k], "cpu") else d[k])
    mc, lb, fc = g(sweep, "min_clear"), g(sweep, "lower_bound"), g(sweep, "first_collision")
    out = {"plans": int(len(mc)),
           "collisions": int((mc < 0).sum()),
           "negative_lower_bound": int((lb < 0).sum()),
           "uncertified_lower_bound": int(np.isnan(lb).sum()),
           "not_finite": int(np.isnan(mc).sum()),
           "first_collision_interval_histogram": np.bincount(fc[fc >= 0]).tolist()}
    if knots is not None:
        kc = g(knots, "min_clear")
        out["collisions_at_a_knot"] = int((kc < 0).sum())
        out["collisions_between_clear_knots"] = int(((mc < 0) & (kc >= 0)).sum())
    if np.isfinite(mc).any():
        worst = int(np.nanargmin(mc))
        out.update({"worst_min_clear": float(mc[worst]), "worst_plan": worst,
                    "worst_interval": int(g(sweep, "arg_interval")[worst]), "worst_obstacle": int(g(sweep, "arg_obst")[worst])})
    if np.isfinite(lb).any():
        out["worst_lower_bound"] = float(np.nanmin(lb))
    return out


def summary(audit, dmin):
    """counts and worst values of a rollout audit (DeviceRollouts.audit): rollouts with a sampled collision, with a knot
    closer than dmin, with a sampled distance below dmin anywhere, with a negative certified lower bound"""
    g = lambda k: np.asarray(audit[k].cpu() if hasattr(audit[k], "cpu") else audit[k])
    mc, lb = g("min_clear"), g("lower_bound")
    fc, fv = g("first_collision"), g("first_violation")
    worst = int(np.argmin(mc))
    return {"rollouts": int(len(mc)),
            "collisions": int((fc >= 0).sum()),
            "knot_violations": int((fv >= 0).sum()),
            "below_dmin_sampled": int((mc < float(dmin) - 1e-6).sum()),
            "negative_lower_bound": int((lb < 0).sum()),
            "worst_min_clear": float(mc[worst]),
            "worst_rollout": worst,
            "worst_step": int(g("arg_step")[worst]),
            "worst_obstacle": int(g("arg_obst")[worst]),
            "worst_lower_bound": float(lb.min()),
            "dmin": float(dmin)}
