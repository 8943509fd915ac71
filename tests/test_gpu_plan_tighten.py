"""GPU tier of the clearance repair (obca_plan_tighten through the C ABI, audit.plan_tighten and clear.solve_clear): the
device against the host build of the same core (tests/native/plan_tighten_host.cpp) on every output word at the edges of the
lane layout, with sentinels around every output; the refused calls; and the driver end to end on demo9's open-loop plan
and on gated C3 instances.

Bounds.  Integers are compared exactly, doubles to 1e-9 (the bound of every audit test: the device build contracts
multiply-adds and has its own libm).  An instance whose variant_out hangs on a measurement within 1e-7 of the target is
not "settled" and is left out of the integer comparison only."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import test_audit_core as core
from tests import test_plan_sweep_core as sweep_core
from tests import test_plan_tighten_core as tcore
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import plan_sweep, plan_tighten
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.clear import solve_clear

pytestmark = pytest.mark.gpu
EGO = tcore.EGO
TOL = 1e-9
PAD = 32
SENT_F, SENT_I = -777.25, -777


@pytest.fixture(scope="module")
def host():
    return tcore.load_host()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _guarded(n, dt, fill=None):
    """a buffer of sentinels with the n output words in its middle (pre-filled with `fill` if given): (buffer, view)"""
    buf = torch.full((n + 2 * PAD,), SENT_F if dt == torch.float64 else SENT_I, dtype=dt, device="cuda")
    if fill is not None:
        buf[PAD:PAD + n] = torch.as_tensor(np.ascontiguousarray(fill).ravel(), dtype=dt, device="cuda")
    return buf, buf[PAD:PAD + n]


def _edges_untouched(g):
    for name, (buf, _) in g.items():
        s = SENT_F if buf.dtype == torch.float64 else SENT_I
        assert (buf[:PAD] == s).all() and (buf[-PAD:] == s).all(), name


def raw_call(g, dev, m, **over):
    """obca_plan_tighten itself on the device tensors dev (x, A, b, variant, status), outputs into the guarded buffers g;
    `over` replaces arguments of the C call by name"""
    a = dict(ego=(ctypes.c_double * 4)(*EGO), n_obs=len(m), m=(ctypes.c_int32 * len(m))(*m), N=dev["x"].shape[2] - 1,
             B=dev["x"].shape[0], variant=_ptr(dev["variant"]), status=_ptr(dev["status"]), x=_ptr(dev["x"]), A=_ptr(dev["A"]),
             b=_ptr(dev["b"]), n_sub=16, certified=0, target=0.0, gain=1.0, grow_max=2.0, device=torch.cuda.current_device())
    a.update({k: _ptr(v[1]) for k, v in g.items()})
    a.update(over)
    return _lib.load().obca_plan_tighten(a["ego"], a["n_obs"], a["m"], a["N"], a["B"], a["variant"], a["status"], a["x"], a["A"], a["b"],
                                         a["n_sub"], a["certified"], a["target"], a["gain"], a["grow_max"], a["grow"], a["b_out"],
                                         a["variant_out"], a["min_clear"], a["device"],
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def to_device(c):
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    return dict(x=t(c["x"]), A=t(c["A"]), b=t(c["b"]), variant=t(c["variant"], torch.int32), status=t(c["status"], torch.int32))


def device_tighten(c, dev, grow=None, **kw):
    """the case on the device through the C ABI with guarded outputs: numpy dict in host_tighten's layout (without d)"""
    B, N1, M, n_obs = c["x"].shape[0], c["x"].shape[2], sum(c["m"]), len(c["m"])
    g = {"grow": _guarded(B * N1 * n_obs, torch.float64, np.zeros((B, N1, n_obs)) if grow is None else grow),
         "b_out": _guarded(B * N1 * M, torch.float64), "variant_out": _guarded(B, torch.int32), "min_clear": _guarded(B, torch.float64)}
    assert raw_call(g, dev, c["m"], **kw) == 0
    torch.cuda.synchronize()
    _edges_untouched(g)
    out = {k: v[1].cpu().numpy() for k, v in g.items()}
    out["grow"], out["b_out"] = out["grow"].reshape(B, N1, n_obs), out["b_out"].reshape(B, N1, M)
    return out


def settled(ref, target, eps=1e-7):
    with np.errstate(invalid="ignore"):
        return ~(np.abs(ref["d"] - target) < eps).any((1, 2))


def assert_equals_host(dev, ref, target, tag):
    for k in ("grow", "b_out", "min_clear"):
        assert np.array_equal(np.isnan(dev[k]), np.isnan(ref[k])), (tag, k)
        assert np.abs(np.nan_to_num(dev[k] - ref[k])).max() <= TOL, (tag, k, float(np.abs(np.nan_to_num(dev[k] - ref[k])).max()))
    ok = settled(ref, target)
    assert ok.sum() >= max(1, len(ok) - 2), tag
    assert np.array_equal(dev["variant_out"][ok], ref["variant_out"][ok]), tag
    assert not (dev["b_out"] == SENT_F).any() and not (dev["variant_out"] == SENT_I).any() and not (dev["min_clear"] == SENT_F).any(), tag


def layout_case(N, B, m, seed):
    rng = np.random.default_rng(seed)
    x, A, b = sweep_core.translating_plans(rng, B, N, m)
    c = tcore.unnormalised(dict(x=x, A=A, b=b, m=list(m)), seed + 1)
    c["variant"] = np.array([4, 6, 8] * B, np.int32)[:B]
    c["status"] = np.array([0, 1] * B, np.int32)[:B]
    return c


def compare_two_calls(host, c, tag, target=3.0, gain=0.25, **kw):
    """two consecutive calls on the same grow, each against the host core.  Target 3 m at gain 0.25: nearly every random
    plan is short somewhere, by amounts that reach the cap of 2 m in the second call for some and not for others."""
    dev = to_device(c)
    kw = dict(kw, target=target, gain=gain)
    r1 = tcore.tighten(host, c, **kw)
    d1 = device_tighten(c, dev, **kw)
    assert_equals_host(d1, r1, target, tag + (1,))
    r2 = tcore.tighten(host, c, grow=d1["grow"], **kw)                          # from the device's own state
    d2 = device_tighten(c, dev, grow=d1["grow"], **kw)
    assert_equals_host(d2, r2, target, tag + (2,))
    assert (d2["grow"] >= d1["grow"]).all()
    return bool((d1["grow"] > 0).any()) + bool((d2["grow"] > d1["grow"]).any())


M_EIGHT = (4,) * 8


# ------------------------------------------------------------------------------------------------------ lane-layout edges
@pytest.mark.parametrize("certified", [0, 1])
@pytest.mark.parametrize("N,m", [(1, (2, 3)), (2, (1,)), (3, M_EIGHT), (5, (2, 3)), (64, (1,)), (65, (2, 3)), (130, M_EIGHT)])
def test_lane_layout_edges(host, N, m, certified):
    """N = 1: one lane owns both stages; 2, 3, 5: idle lanes in a segment; 64: segment = wavefront; 65, 130: a stage whose
    two intervals lie in different passes of different lanes.  B = 1 and one more than fills the last wavefront."""
    seg = 1
    while seg < N and seg < 64:
        seg *= 2
    rose = [compare_two_calls(host, layout_case(N, B, m, 7000 + 10 * N + B), (N, B, m, certified), certified=certified)
            for B in (1, 64 // seg + 1)]
    assert rose[1] == 2, rose                                   # grow rose in both calls of the larger batch


@pytest.mark.parametrize("m", [(1,), (2, 3), M_EIGHT])
@pytest.mark.parametrize("certified", [0, 1])
def test_row_counts(host, m, certified):
    for N in (5, 65):
        assert compare_two_calls(host, layout_case(N, 3, m, 8000 + N + len(m)), (N, m, certified), certified=certified, gain=0.04,
                                 grow_max=0.6) >= 1


@pytest.mark.parametrize("certified", [0, 1])
@pytest.mark.parametrize("N", [5, 65])
def test_mixed_batch(host, N, certified):
    """variants 0 / 4 / 6 / 8 with statuses 0 / 1 / 2 / -1 and one NaN pose: the passed-through instances keep their grow"""
    c = layout_case(N, 17, sweep_core.M3, 9000 + N)
    c["variant"] = np.array([0, 4, 6, 8] * 5, np.int32)[:17]
    c["status"] = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, -1, -1, -1, -1, 0], np.int32)
    c["variant"][16] = 6
    c["x"][16, 1, N // 2 + 1] = np.nan
    g0 = np.random.default_rng(5).uniform(0, 0.4, (17, N + 1, 3))
    dev = to_device(c)
    ref = tcore.tighten(host, c, target=0.5, certified=certified, grow=g0)
    got = device_tighten(c, dev, target=0.5, certified=certified, grow=g0)
    assert_equals_host(got, ref, 0.5, (N, certified))
    off = ~((c["variant"] != 0) & (c["status"] >= 0) & (c["status"] <= 1))
    off[16] = True
    assert off.sum() == 11
    assert np.array_equal(got["grow"][off], g0[off]) and not got["variant_out"][off].any() and np.isnan(got["min_clear"][off]).all()
    assert np.isfinite(got["min_clear"][~off]).all() and (got["grow"][~off] > g0[~off]).any()


def test_wrapper_equals_the_c_call(host):
    c = tcore.case_random()
    got = plan_tighten(c["x"], c["A"], c["b"], c["m"], c["variant"], c["status"], target=0.5, ego=EGO)
    torch.cuda.synchronize()
    raw = device_tighten(c, to_device(c), target=0.5)
    for k in raw:
        assert np.array_equal(got[k].cpu().numpy(), raw[k]), k


# -------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [dict(n_sub=0), dict(gain=0.0), dict(grow_max=3.0), "alias", dict(certified=2), dict(target=math.nan),
                                 dict(gain=8.5), dict(grow_max=-0.1), dict(variant=None), dict(status=None), dict(grow=None),
                                 dict(b_out=None), dict(variant_out=None), dict(N=0), dict(B=0), dict(n_obs=9), dict(device=-1)])
def test_refused_calls_leave_every_output_alone(bad):
    c = tcore.case_random()
    B, N1, M, n_obs = 9, 5, sum(c["m"]), 3
    dev = to_device(c)
    g = {"grow": _guarded(B * N1 * n_obs, torch.float64), "b_out": _guarded(B * N1 * M, torch.float64),
         "variant_out": _guarded(B, torch.int32), "min_clear": _guarded(B, torch.float64)}
    b0 = dev["b"].clone()
    over = dict(b_out=_ptr(dev["b"])) if bad == "alias" else bad
    assert raw_call(g, dev, c["m"], **over) == core.E_INVAL
    torch.cuda.synchronize()
    for name, (buf, _) in g.items():
        assert (buf == (SENT_F if buf.dtype == torch.float64 else SENT_I)).all(), name
    assert torch.equal(dev["b"], b0)
    g["grow"][1].zero_()
    assert raw_call(g, dev, c["m"]) == 0                        # and the same call, unchanged, runs
    torch.cuda.synchronize()
    _edges_untouched(g)
    assert not (g["b_out"][1] == SENT_F).any() and not (g["variant_out"][1] == SENT_I).any()


# ------------------------------------------------------------------------------------------------------------ the driver
def _words(t):
    return t.contiguous().view(torch.uint8)


def test_solve_clear_without_rounds_is_solve():
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams
    N, B = 5, 64
    bt = sc.make_batch(B, N)
    s = BatchSolver(N, bt["m"], max_batch=B)
    args = (bt["variant"], bt["x0"], bt["u0"], bt["xref"], bt["A"], bt["b"], bt["Ts"], bt["term"], SolverParams())
    ref = s.solve(*args)
    got, info = solve_clear(s, *args, ego=sc.EGO, rounds=0)
    sw = plan_sweep(ref.xopt, bt["A"], bt["b"], bt["m"], n_sub=16, ego=sc.EGO, variant=bt["variant"])
    torch.cuda.synchronize()
    s.close()
    for k in ("xopt", "uopt", "ts_opt", "status", "iters", "info"):
        assert torch.equal(_words(getattr(got, k)), _words(getattr(ref, k))), k
    assert ref.feas.all() and torch.equal(_words(info["min_clear"]), _words(sw["min_clear"]))
    assert torch.equal(_words(info["min_clear"]), _words(info["min_clear_first"])) and not info["rounds_used"].any()
    assert not info["grow"].any() and torch.equal(info["b_used"], torch.as_tensor(bt["b"], device="cuda"))
    assert torch.equal(info["clear"], sw["min_clear"] >= 0.0)


class _Recorder:
    """an `obca`-shaped object that keeps the arguments of the open-loop call and solves nothing"""

    def obca_mpc4(self, *a, start_order=None):
        self.args = a
        N = a[4]
        return np.zeros((3, N + 1)), np.zeros((2, N)), False, float(a[0])


def demo9_open_loop(N):
    """demo9's open-loop free-time problem as closedLoop.mpc_openLoop_freeTime packs it, and its solver parameters"""
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.closed_loop import closedLoop
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.demo_setting import problemSetting
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import SolverParams, pack_reference_call
    rec = _Recorder()
    cl = closedLoop(problemSetting("demo9"), solver=rec)
    cl.N_free = N
    cl.mpc_openLoop_freeTime()
    Ts, P, Q, R, N, x0, xL, xU, uL, uU, xref, nObs, vObs, AObs, bObs, dmin, ego, u0 = rec.args
    m, x0v, u0v, xr, A, b, Tsv, term = pack_reference_call(4, Ts, N, x0, xref, nObs, vObs, AObs, bObs, u0)
    prm = SolverParams(Q_free=Q, R_free=R, P_free=P, xL=xL, xU=xU, uL=uL, uU=uU, ego=ego, dmin=dmin, start_order="x0")
    return m, (4, x0v[None], u0v[None], xr[None], A[None], b[None], np.array([Tsv]), term[None], prm), tuple(float(v) for v in ego)


def test_demo9_open_loop_plan_is_repaired():
    """demo9, N = 20: the plan cuts static obstacle 1 in interval 7 between clear knots.  After at most four
    rounds the held plan is strictly clearer against the original rows, every held word is finite, and where the driver
    calls the plan clear an independent sweep agrees.
    MEASURED on the MI355X (gain 1, n_sub 16, target 0): -1.184 m -> -0.036 m after 3 re-solves; the next one has no feasible
    point, so the plan is NOT clear within four rounds and `>= 0` is not asserted (N = 30 ... 74 are repaired)."""
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver
    m, args, ego = demo9_open_loop(20)
    s = BatchSolver(20, m, max_batch=1)
    base = s.solve(*args)
    A, b = args[4], args[5]
    judge = lambda x: plan_sweep(x, A, b, m, n_sub=16, ego=ego, variant=np.array([4], np.int32))
    sw0, kn0 = judge(base.xopt.clone()), plan_sweep(base.xopt, A, b, m, n_sub=1, ego=ego, variant=np.array([4], np.int32))
    held, info = solve_clear(s, *args, ego=ego, rounds=4)
    sw1 = judge(held.xopt)
    torch.cuda.synchronize()
    s.close()
    print("demo9 N=20: min_clear %.6f (interval %d, obstacle %d) -> %.6f after %d re-solves, clear %s" %
          (sw0["min_clear"].item(), sw0["arg_interval"].item(), sw0["arg_obst"].item(), sw1["min_clear"].item(),
           info["rounds_used"].item(), bool(info["clear"].item())))
    assert base.feas.all() and sw0["min_clear"].item() < 0 and kn0["min_clear"].item() > 0
    assert (sw0["arg_interval"].item(), sw0["arg_obst"].item()) == (7, 1)
    assert held.feas.all() and 1 <= info["rounds_used"].item() <= 4
    for k in ("xopt", "uopt", "ts_opt", "info"):
        assert torch.isfinite(getattr(held, k)).all(), k
    assert torch.equal(_words(info["min_clear_first"]), _words(sw0["min_clear"]))
    assert torch.equal(_words(info["min_clear"]), _words(sw1["min_clear"]))
    assert sw1["min_clear"].item() > sw0["min_clear"].item()
    if info["clear"].item():
        assert sw1["min_clear"].item() >= 0.0 and sw1["first_collision"].item() == -1


# seeds of scenarios.make_instance_c3 whose lidar gate is on (obca_mpc6 against five obstacles with rows per stage), chosen on
# the CPU (tests/native_build.lpi_solve and the host sweep, n_sub = 16): the first 24 gated seeds, every one feasible there, 13 of
# them cut between clear knots (0.11 to 0.46 m deep), 11 clear; the test asks the device for at least GATED_CUT
GATED_SEEDS = (2, 4, 5, 7, 12, 14, 15, 20, 24, 25, 27, 28, 30, 31, 34, 35, 36, 37, 38, 44, 50, 51, 52, 54)
GATED_CUT = 8


def test_gated_instances_are_repaired():
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams
    ins = [sc.make_instance_c3(i, 20) for i in GATED_SEEDS]
    assert all(q["gated"] for q in ins) and len(ins) <= 64
    B, m = len(ins), ins[0]["m"]
    st = lambda k: np.stack([q[k] for q in ins])
    A, b, var = st("A"), st("b"), np.full(B, 6, np.int32)
    args = (var, st("x0"), st("u0"), st("xref"), A, b, np.array([q["Ts_fix"] for q in ins]), st("term"), SolverParams())
    s = BatchSolver(20, m, max_batch=B)
    base = s.solve(*args)
    judge = lambda x, n_sub=16: plan_sweep(x, A, b, m, n_sub=n_sub, ego=sc.EGO, variant=var)
    sw0, kn0 = judge(base.xopt), judge(base.xopt, 1)
    keep = {k: getattr(base, k).clone() for k in ("xopt", "uopt", "ts_opt", "status", "iters")}
    held, info = solve_clear(s, *args, ego=sc.EGO, rounds=4)
    sw1 = judge(held.xopt)
    torch.cuda.synchronize()
    s.close()
    mc0, mc1 = sw0["min_clear"], sw1["min_clear"]
    cut = (mc0 < 0) & (kn0["min_clear"] >= 0)
    print("gated C3: %d instances, %d feasible, %d cut between clear knots; clear %d -> %d; rounds %s; largest grow %.3f" %
          (B, int(base.feas.sum()), int(cut.sum()), int((mc0 >= 0).sum()), int(info["clear"].sum()),
           torch.bincount(info["rounds_used"].long(), minlength=5).tolist(), info["grow"].max().item()))
    assert base.feas.all() and int(cut.sum()) >= GATED_CUT
    assert torch.equal(_words(info["min_clear_first"]), _words(mc0)) and torch.equal(_words(info["min_clear"]), _words(mc1))
    assert held.feas.all() and (mc1[info["clear"]] >= 0.0).all()                   # an independent sweep, the original rows
    assert (mc1 >= info["min_clear_first"]).all()
    assert int(info["clear"].sum()) > int((mc0 >= 0).sum())
    was = mc0 >= 0
    assert was.any() and not info["rounds_used"][was].any()
    for k, v in keep.items():
        assert torch.equal(_words(getattr(held, k)[was]), _words(v[was])), k
