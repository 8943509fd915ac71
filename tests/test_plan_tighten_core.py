"""CPU tier of the clearance repair (audit::plan_tighten_* of csrc/obca_audit_core.h, obca_plan_tighten's per-instance work),
built for the host from tests/native/plan_tighten_host.cpp: the measurement per (interval, obstacle) against the swept audit's
host build (word for word) and against tests/kkt_check.py at the knots (1e-9, the bound of every audit test against that
helper), the update rule restated in numpy (word for word: the host build is compiled without contraction and calls the
same libm hypot as numpy), pass-through, a half-plane whose offset is known in closed form, and one repair end to end on the
CPU solver.  The cases and helpers are shared with tests/test_gpu_plan_tighten.py."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import native_build
from tests import test_audit_core as core
from tests import test_plan_sweep_core as sweep_core

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "plan_tighten_host.cpp")
EGO = core.EGO
TOL = 1e-9
_p = core._p


def load_host():
    lib = native_build.build_shim("plan_tighten_host", [SRC])
    lib.plan_tighten_host.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def sweep_host():
    return sweep_core.load_host()


def host_tighten(host, x, A, b, m, variant, status, n_sub=16, certified=0, target=0.0, gain=1.0, grow_max=2.0, grow=None,
                 ego=EGO, rc=0):
    """plan_tighten_host: dict of grow [B,N+1,n_obs] (a copy of `grow`, updated; None: zeros), b_out [B,N+1,M], variant_out,
    min_clear [B] and d [B,N,n_obs]"""
    B, N = x.shape[0], x.shape[2] - 1
    x, A, b = (np.ascontiguousarray(a, float) for a in (x, A, b))
    var, st = np.ascontiguousarray(variant, np.int32), np.ascontiguousarray(status, np.int32)
    o = {"grow": np.zeros((B, N + 1, len(m))) if grow is None else np.array(grow, float), "b_out": np.full(b.shape, -777.25),
         "variant_out": np.full(B, -777, np.int32), "min_clear": np.full(B, -777.25), "d": np.zeros((B, N, len(m)))}
    got = host.plan_tighten_host(_p(np.asarray(ego, float)), len(m), _p(np.asarray(m, np.int32)), N, B, _p(var), _p(st), _p(x), _p(A),
                                 _p(b), int(n_sub), int(certified), ctypes.c_double(target), ctypes.c_double(gain),
                                 ctypes.c_double(grow_max), _p(o["grow"]), _p(o["b_out"]), _p(o["variant_out"]), _p(o["min_clear"]),
                                 _p(o["d"]))
    assert got == rc
    return o


def rows_norm(A, m):
    """|a| of every row as the core takes it (hypot), and the obstacle of every row: [B,N+1,M], [M]"""
    return np.hypot(A[..., 0], A[..., 1]), np.repeat(np.arange(len(m)), m)


def expected_update(d, A, b, m, variant, grow0, target, gain, grow_max):
    """the issue's rule in numpy from the measurements d [B,N,n_obs] of repaired instances: grow, b_out, variant_out"""
    B, N, _ = d.shape
    need = np.where(d < target, gain * (target - d), 0.0)
    left = np.concatenate([np.zeros((B, 1, len(m))), need], 1)               # need[k-1] at stage k
    right = np.concatenate([need, np.zeros((B, 1, len(m)))], 1)              # need[k]
    inc = np.maximum(left, right)
    v4 = np.asarray(variant) == 4
    inc[v4] = need[v4].max(1, keepdims=True)
    grow = np.maximum(grow0, np.minimum(grow_max, grow0 + inc))
    nrm, obst = rows_norm(A, m)
    return grow, b + grow[:, :, obst] * nrm, np.where((grow > grow0).any((1, 2)), variant, 0).astype(np.int32)


def words(a):
    return np.ascontiguousarray(a, float).view(np.uint64)


def unnormalised(c, seed):
    """the case with every row scaled by a factor of its own (the same at every stage: the obstacle still translates)"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.2, 5.0, (c["A"].shape[0], 1, c["A"].shape[2]))
    return dict(c, A=c["A"] * f[..., None], b=c["b"] * f)


def case_random(seed=201, B=9, N=4):
    x, A, b = sweep_core.translating_plans(np.random.default_rng(seed), B, N, sweep_core.M3)
    c = unnormalised(dict(x=x, A=A, b=b, m=sweep_core.M3), seed + 1)
    c["variant"] = np.array([4, 6, 8] * B, np.int32)[:B]
    c["status"] = np.array([0, 1] * B, np.int32)[:B]
    return c


def case_mixed():
    """variants 0 / 4 / 6 / 8 against statuses 0 / 1 / 2 / -1, and a NaN pose in an instance that would be repaired"""
    c = case_random(203, 17, 5)
    c["variant"] = np.array([0, 4, 6, 8] * 5, np.int32)[:17]
    c["status"] = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, -1, -1, -1, -1, 0], np.int32)
    c["variant"][16] = 6
    c["x"][16, 1, 3] = np.nan
    return c


# the half-plane {y <= 0} given by the unnormalised row (0, 2.5) q <= 0 and a car that stands at (3, Y0) and turns from
# theta = 0 (stages 0, 1) to pi / 2 (stages 2, 3, 4).  Its footprint (3.4 x 1.5 m about the pose point) reaches
# 1.7 sin(theta) + 0.75 cos(theta) below the pose: 0.75 and 1.7 at the knots, up to 1.858 while it turns.
Y0, SCALE = 1.8, 2.5


def case_half_plane(variant=6):
    N = 4
    x = np.zeros((1, 3, N + 1))
    x[0, 0], x[0, 1], x[0, 2, 2:] = 3.0, Y0, math.pi / 2
    A = np.zeros((1, N + 1, 1, 2))
    A[..., 1] = SCALE
    return dict(x=x, A=A, b=np.zeros((1, N + 1, 1)), m=[1], variant=np.array([variant], np.int32), status=np.zeros(1, np.int32))


def half_plane_dip(n_sub, target):
    """target minus the smallest sampled distance of the turning interval, from the footprint's closed form"""
    th = np.array([sweep_core.lerp(0.0, math.pi / 2, n_sub, j) for j in range(n_sub + 1)])
    return target - (Y0 - (1.7 * np.sin(th) + 0.75 * np.cos(th))).min()


def tighten(host, c, **kw):
    return host_tighten(host, c["x"], c["A"], c["b"], c["m"], c["variant"], c["status"], **kw)


# --------------------------------------------------------------------------------------------------------- measurement
@pytest.mark.parametrize("n_sub", [1, 16])
def test_d_is_the_sweep_per_obstacle(host, sweep_host, n_sub):
    c = case_random()
    got = tighten(host, c, n_sub=n_sub, target=-50.0)
    sw = sweep_core.host_sweep(sweep_host, c["x"], c["A"], c["b"], c["m"], c["variant"], n_sub)
    assert np.array_equal(words(got["d"].min(2)), words(sw["interval_min"]))
    assert np.array_equal(words(got["min_clear"]), words(sw["min_clear"]))
    assert (got["d"] < 0).any() and (got["d"] > 0).any()
    assert not got["variant_out"].any() and not got["grow"].any()             # nothing is below -50
    if n_sub == 1:                                                             # the knot values, per obstacle
        d = sweep_core.numpy_samples(c["x"], c["A"], c["b"], c["m"], c["variant"], 1)
        assert np.abs(got["d"] - d.min(2)).max() <= TOL


def test_certified_d_is_the_obstacles_own_bound(host, sweep_host):
    c = case_random()
    samp, cert = tighten(host, c, target=-50.0), tighten(host, c, certified=1, target=-50.0)
    sw = sweep_core.host_sweep(sweep_host, c["x"], c["A"], c["b"], c["m"], c["variant"], 16)
    assert np.isfinite(cert["d"]).all() and (cert["d"] <= samp["d"]).all() and (cert["d"] < samp["d"] - 1e-3).any()
    # the sweep charges every obstacle the largest move among them: its bound is the smaller one
    assert (cert["min_clear"] >= sw["lower_bound"]).all()
    one = sweep_core.case_translating_box()                                    # one obstacle: the same words
    one.update(variant=np.array([6], np.int32), status=np.zeros(1, np.int32))
    sw1 = sweep_core.host_sweep(sweep_host, one["x"], one["A"], one["b"], one["m"], one["variant"], 8)
    assert np.array_equal(words(tighten(host, one, n_sub=8, certified=1, target=-50.0)["min_clear"]), words(sw1["lower_bound"]))


# -------------------------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("target,gain,grow_max", [(0.0, 1.0, 2.0), (0.5, 1.7, 2.0), (0.5, 8.0, 0.3)])
def test_update_rule_word_for_word(host, target, gain, grow_max):
    c = case_random()
    g0 = np.zeros((9, 5, 3))
    got = tighten(host, c, target=target, gain=gain, grow_max=grow_max)
    grow, b_out, vout = expected_update(got["d"], c["A"], c["b"], c["m"], c["variant"], g0, target, gain, grow_max)
    assert np.array_equal(words(got["grow"]), words(grow)) and np.array_equal(words(got["b_out"]), words(b_out))
    assert np.array_equal(got["variant_out"], vout) and vout.any()
    assert got["grow"].max() <= grow_max and (got["grow"] > 0).any()
    # b_out - b is grow |a| for unnormalised rows: the offset in metres is grow itself
    nrm, obst = rows_norm(c["A"], c["m"])
    assert np.abs(nrm - 1.0).max() > 0.5
    assert np.abs((got["b_out"] - c["b"]) / nrm - got["grow"][:, :, obst]).max() <= 1e-12
    # a second call on the same plans: grow is in/out, rises again and stays capped
    again = tighten(host, c, target=target, gain=gain, grow_max=grow_max, grow=got["grow"])
    grow2, b_out2, vout2 = expected_update(again["d"], c["A"], c["b"], c["m"], c["variant"], got["grow"], target, gain, grow_max)
    assert np.array_equal(words(again["d"]), words(got["d"]))                   # measured against the original rows
    assert np.array_equal(words(again["grow"]), words(grow2)) and np.array_equal(words(again["b_out"]), words(b_out2))
    assert np.array_equal(again["variant_out"], vout2)
    assert (again["grow"] >= got["grow"]).all() and again["grow"].max() <= grow_max
    if grow_max == 0.3:
        assert (got["grow"] == grow_max).any()
        capped = tighten(host, c, target=target, gain=gain, grow_max=grow_max, grow=np.where(got["d"].min(1, keepdims=True) < target, 0.3, 0.0)
                         * np.ones((1, 5, 1)))
        assert not capped["variant_out"].any()                                  # every short obstacle is at its cap: nothing rose


def test_grow_never_decreases(host):
    """a state above this call's cap stays where it is"""
    c = case_random()
    g0 = np.full((9, 5, 3), 0.75)
    got = tighten(host, c, target=0.5, grow_max=0.25, grow=g0)
    assert np.array_equal(got["grow"], g0) and not got["variant_out"].any()
    nrm, obst = rows_norm(c["A"], c["m"])
    assert np.array_equal(words(got["b_out"]), words(c["b"] + 0.75 * nrm))


def test_half_plane_moves_out_by_the_dip(host):
    c = case_half_plane()
    e = half_plane_dip(16, 0.0)
    assert 0.05 < e < 0.06                                                     # 1.858 - 1.8: the knots are clear (1.05, 0.1)
    got = tighten(host, c)
    assert np.abs(got["d"][0, :, 0] - [Y0 - 0.75, -e, Y0 - 1.7, Y0 - 1.7]).max() <= 1e-12
    # the deficit of interval 1 raises stages 1 and 2 and no other
    assert got["grow"][0, [0, 3, 4], 0].tolist() == [0.0, 0.0, 0.0]
    assert np.abs(got["grow"][0, [1, 2], 0] - e).max() <= 1e-12 and got["variant_out"][0] == 6
    # and the tightened half-plane {y <= b_out / 2.5} lies e further out
    assert np.abs(got["b_out"][0, :, 0] / SCALE - [0, e, e, 0, 0]).max() <= 1e-12
    assert abs(got["min_clear"][0] + e) <= 1e-12
    # target 0.2: intervals 2 and 3 are 0.1 short, interval 1 0.2 + e: a stage takes the larger of its two intervals
    got = tighten(host, c, target=0.2)
    assert np.abs(got["grow"][0, :, 0] - [0, 0.2 + e, 0.2 + e, 0.1, 0.1]).max() <= 1e-12
    got = tighten(host, c, target=0.2, gain=0.5, grow_max=0.1)
    assert np.abs(got["grow"][0, :, 0] - [0, 0.1, 0.1, 0.05, 0.05]).max() <= 1e-12


def test_variant_4_gets_the_largest_need_at_every_stage(host):
    c = case_half_plane(variant=4)
    c["A"][0, 1:, 0] = [[3.0, 4.0]] * 4                                         # other rows after stage 0: measured never,
    e = half_plane_dip(16, 0.2)                                                 # offset with their own |a| = 5
    got = tighten(host, c, target=0.2)
    assert np.abs(got["grow"][0, :, 0] - e).max() <= 1e-12 and got["variant_out"][0] == 4
    assert np.abs(got["b_out"][0, :, 0] - e * np.array([SCALE, 5, 5, 5, 5])).max() <= 1e-12
    r = case_random()
    got = tighten(host, r, target=0.5)
    v4 = r["variant"] == 4
    assert v4.sum() >= 2 and (got["grow"][v4] == got["grow"][v4][:, :1]).all() and (got["grow"][v4] > 0).any()
    assert not (got["grow"][~v4] == got["grow"][~v4][:, :1]).all()


# -------------------------------------------------------------------------------------------------------- pass-through
def test_pass_through(host):
    c = case_mixed()
    g0 = np.random.default_rng(5).uniform(0, 0.4, (17, 6, 3))
    got = tighten(host, c, target=0.5, grow=g0)
    repaired = (c["variant"] != 0) & (c["status"] >= 0) & (c["status"] <= 1)
    repaired[16] = False                                                       # the NaN pose
    assert repaired.sum() == 6 and set(c["variant"][repaired]) == {4, 6, 8}
    nrm, obst = rows_norm(c["A"], c["m"])
    off = ~repaired
    assert np.array_equal(words(got["grow"][off]), words(g0[off])) and not got["variant_out"][off].any()
    assert np.array_equal(words(got["b_out"][off]), words((c["b"] + g0[:, :, obst] * nrm)[off]))
    assert np.isnan(got["min_clear"][off]).all() and np.isfinite(got["min_clear"][repaired]).all()
    assert np.isnan(got["d"][off & (np.arange(17) < 16)]).all()                                   # variant 0, bad status: not measured
    assert np.array_equal(np.isnan(got["d"][16]).any(1), [False, False, True, True, False])   # measured: NaN at stage 3
    grow, b_out, vout = expected_update(got["d"][repaired], c["A"][repaired], c["b"][repaired], c["m"], c["variant"][repaired],
                                        g0[repaired], 0.5, 1.0, 2.0)
    assert np.array_equal(words(got["grow"][repaired]), words(grow)) and np.array_equal(words(got["b_out"][repaired]), words(b_out))
    assert np.array_equal(got["variant_out"][repaired], vout) and vout.all()


def test_certified_passes_a_turning_obstacle_through(host):
    c = sweep_core.case_nan()                                                  # instance 2: obstacle 1 turns between stages 1 and 2
    c.update(variant=np.full(4, 6, np.int32), status=np.zeros(4, np.int32))
    samp, cert = tighten(host, c, target=50.0), tighten(host, c, target=50.0, certified=1)
    assert np.isfinite(samp["min_clear"][[0, 2, 3]]).all() and samp["variant_out"][[0, 2, 3]].tolist() == [6, 6, 6]
    assert np.isfinite(cert["min_clear"][0]) and cert["variant_out"][0] == 6
    for i in (1, 2, 3):                                                        # NaN pose; rows that turn; rows that change shape
        assert np.isnan(cert["min_clear"][i]) and cert["variant_out"][i] == 0 and not cert["grow"][i].any()
        assert np.array_equal(words(cert["b_out"][i]), words(c["b"][i]))
    assert np.isnan(cert["d"][2, 1, 1]) and np.isfinite(np.delete(cert["d"][2].ravel(), 1 * 3 + 1)).all()


def test_refused_calls(host):
    c = case_half_plane()
    for bad in (dict(n_sub=0), dict(gain=0.0), dict(gain=8.5), dict(grow_max=3.0), dict(grow_max=-0.1), dict(target=math.nan),
                dict(certified=2)):
        got = tighten(host, c, rc=core.E_INVAL, **bad)
        assert (got["b_out"] == -777.25).all() and (got["variant_out"] == -777).all() and not got["grow"].any()


# ---------------------------------------------------------------------------------------------------------- end to end
ROUNDS = 4


def demo9_open_loop(N=20):
    """demo9's open-loop free-time problem at horizon N as closedLoop.mpc_openLoop_freeTime packs it: the arrays of the
    solver call and the solver parameters of that call"""
    from oracle import c_oracle
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.closed_loop import closedLoop
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.demo_setting import problemSetting
    s = native_build.LpiObca()
    cl = closedLoop(problemSetting("demo9"), solver=s)
    cl.N_free = N
    cl.mpc_openLoop_freeTime()
    c = s.calls[-1]
    assert cl.feas and c["variant"] == 4 and c["status"] in (0, 1)
    prm = c_oracle.default_params(xL=cl.xL[:2], xU=cl.xU[:2], uL=cl.uL, uU=cl.uU, ego=cl.ego, dmin=cl.dmin, start_order="x0",
                                  Qf=cl.Q_free, Pf=cl.P_free, R1f=cl.R_free[0], R2f=cl.R_free[1])
    return c, prm, np.asarray(cl.xOpt, float), tuple(float(v) for v in cl.ego)


def repair_on_host(host, c, prm, x_first, ego, rounds, **kw):
    """clear.solve_clear's loop for one instance with tests/native_build.lpi_solve as the solver and the host tighten
    function: the held plan, its clearance, round 0's clearance and the re-solves used"""
    N, m = x_first.shape[1] - 1, c["m"]
    A, b, var = c["A"][None], c["b"][None], np.array([c["variant"]], np.int32)
    t = host_tighten(host, x_first[None], A, b, m, var, np.array([c["status"]], np.int32), ego=ego, **kw)
    held, mc, first, used = x_first, t["min_clear"][0], t["min_clear"][0], 0
    for _ in range(rounds):
        if not t["variant_out"][0]:
            break
        o = native_build.lpi_solve(t["variant_out"], N, m, c["x0"][None], c["u0"][None], c["xref"][None], A, t["b_out"], [c["Ts"]],
                                   c["term"][None], prm)
        used += 1
        t = host_tighten(host, o["xopt"], A, b, m, t["variant_out"], o["status"], grow=t["grow"], ego=ego, **kw)
        if t["min_clear"][0] > mc:
            held, mc = o["xopt"][0], t["min_clear"][0]
    return held, mc, first, used


def test_demo9_open_loop_plan_is_repaired_on_the_cpu(host, sweep_host):
    """demo9, N = 20: the open-loop plan is clear at its knots and cuts a static obstacle between two of them.  After at most
    four rounds the held plan is strictly clearer against the original rows, and where the loop calls it clear the swept
    audit agrees.
    MEASURED on the host build of the solver (gain 1, n_sub 16, target 0).  Its plan is another local optimum than the
    device's of DESIGN 5d (interval 7, obstacle 1, 1.18 m): every start order of the host build ends at Ts_opt = 6.3013 s with
    the cut in interval 12 against obstacle 2, 0.924 m deep, so the place is printed and only the sign is asserted.  Round 1
    (obstacle 2 grown by 0.924 m at every stage, obstacle 4 by 0.464 m) gives a feasible plan that still cuts 0.311 m; round
    2's re-solve has no feasible point (status 2) and the instance ends: -0.924 -> -0.311 after 2 re-solves, NOT clear in
    four rounds.  Gains 0.5 and 1.5 and target 0.05 end the same way or at once.  So the strict improvement is asserted and
    reaching >= 0 is not."""
    c, prm, x0, ego = demo9_open_loop(20)
    judge = lambda x: sweep_core.host_sweep(sweep_host, x[None], c["A"][None], c["b"][None], c["m"], np.array([4], np.int32), 16, ego=ego)
    base = judge(x0)
    assert base["min_clear"][0] < 0 and base["first_collision"][0] >= 0
    print("baseline cut: interval %d, obstacle %d" % (base["arg_interval"][0], base["arg_obst"][0]))
    assert sweep_core.host_sweep(sweep_host, x0[None], c["A"][None], c["b"][None], c["m"], np.array([4], np.int32), 1, ego=ego)["min_clear"][0] > 0
    held, mc, first, used = repair_on_host(host, c, prm, x0, ego, ROUNDS)
    after = judge(held)
    print("demo9 N=20 on the CPU: min_clear %.6f -> %.6f after %d re-solves" % (base["min_clear"][0], after["min_clear"][0], used))
    assert words(first) == words(base["min_clear"][0]) and words(mc) == words(after["min_clear"][0])
    assert np.isfinite(held).all() and 1 <= used <= ROUNDS
    assert after["min_clear"][0] > base["min_clear"][0]
    if mc >= 0.0:
        assert after["min_clear"][0] >= 0.0 and after["first_collision"][0] == -1
