"""GPU parity: the HIP path (through the C ABI) against the oracle on the same inputs.

Tolerances (fp64): where the oracle and the kernel follow the same iterate sequence (equal iteration counts)
the trajectories agree to 1e-9; otherwise both must be KKT points of the same NLP -- the trajectories are then
compared to 1e-5 when the objective values agree, and each is certified separately when they landed in
different local optima (non-convex problem; see DESIGN.md "Parity").
"""
import json
import os

import numpy as np
import pytest
import torch

from __graft_entry__ import host_cpus
from oracle import ipm_dense
from oracle.obca_nlp import Problem
from tests.test_oracle_nlp import build

pytestmark = pytest.mark.gpu

ORDER = ["Ts", "P", "Q", "R", "N", "x0", "xL", "xU", "uL", "uU", "xref", "nObs", "vObs", "AObs", "bObs", "dmin",
         "ego", "u0"]


def ref_args(case):
    a = case["inputs"]
    args = [a[k] for k in ORDER]
    args[1], args[2], args[3] = np.array(args[1]), np.array(args[2]), [np.array(r) for r in args[3]]
    if case["variant"] == 6:
        args += [a["uOpt"], np.array(a["terminal_set"])]
    if case["variant"] == 8:
        args += [a["uOpt"]]
    return args


@pytest.fixture(scope="module")
def solver_cls():
    import __graft_entry__ as ge
    ge.build()
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.obca import obca
    return obca


TIGHT = ["demo1_N6_mpc4_step0", "demo9_N5_mpc4_step0", "demo8_N5_mpc4_step0", "slanted_asym_mpc4",
         "slanted_asym_mpc6", "slanted_asym_mpc8"]


@pytest.mark.parametrize("name", TIGHT)
def test_golden_scenarios_match_oracle(nlp_golden, solver_cls, name):
    case = [c for c in nlp_golden if c["name"] == name][0]
    x, u, feas, ts = getattr(solver_cls(), "obca_mpc%d" % case["variant"])(*ref_args(case))
    r = ipm_dense.solve(build(case))
    assert feas and r.feas
    assert x.shape == (3, case["inputs"]["N"] + 1) and u.shape == (2, case["inputs"]["N"])
    np.testing.assert_allclose(x, r.xopt, rtol=0, atol=1e-9)
    np.testing.assert_allclose(u, r.uopt, rtol=0, atol=1e-9)
    assert ts == pytest.approx(float(r.Ts_opt), abs=1e-9)


def test_known_answers_on_gpu(nlp_golden, solver_cls):
    """analytic demo8 optimum and the SciPy-converged demo1/demo9 optima"""
    s = solver_cls()
    for name, T in (("demo8_N5_mpc4_step0", 20.0), ("demo1_N6_mpc4_step0", 20.378864),
                    ("demo9_N5_mpc4_step0", 30.451762)):
        case = [c for c in nlp_golden if c["name"] == name][0]
        x, u, feas, ts = s.obca_mpc4(*ref_args(case))
        assert feas and ts == pytest.approx(T * 0.1, abs=2e-6)
        assert np.allclose(u[0], 0.6, atol=1e-6)
    x, u, feas, ts = s.obca_mpc4(*ref_args([c for c in nlp_golden if c["name"] == "demo8_N5_mpc4_step0"][0]))
    np.testing.assert_allclose(x, [[3 + 1.2 * k for k in range(6)], [4.0] * 6, [0.0] * 6], atol=1e-6)


def test_infeasible_instance_reports_feas_false(nlp_golden, solver_cls):
    case = [c for c in nlp_golden if c["name"] == "demo1_N5_mpc4_step0"][0]
    x, u, feas, ts = solver_cls().obca_mpc4(*ref_args(case))
    assert feas is False
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u))           # last iterate is returned, like the reference


@pytest.mark.parametrize("name", ["demo1_dyn_mpc6", "demo1_dyn_mpc8"])
def test_hard_fixed_time_cases_are_certified(nlp_golden, solver_cls, name):
    """long non-convex runs.  demo1_dyn_mpc6 is SURVEY Appendix C's "mpc6 witness": from the reference's cold start the
    method ends at an infeasible stationary point (the plan that dives under the moving box), the window start finds the
    plan that passes above it -- the survey's criterion is feas = True with f <= 0.02974."""
    case = [c for c in nlp_golden if c["name"] == name][0]
    p = build(case)
    x, u, feas, ts = getattr(solver_cls(), "obca_mpc%d" % case["variant"])(*ref_args(case))
    r = ipm_dense.solve(p)
    assert feas and r.feas
    np.testing.assert_allclose(x, r.xopt, rtol=0, atol=1e-5)
    np.testing.assert_allclose(u, r.uopt, rtol=0, atol=1e-5)
    if name == "demo1_dyn_mpc6":
        assert r.starts_used == 1                                       # the default order starts obca_mpc6 at the window, which finds it
        assert ipm_dense.solve(p, dict(start_order="x0")).restarted     # (from x0 the method ends under the box first)
        assert r.f <= 0.02974 + 1e-6
    # primal feasibility of the kernel's trajectory in the ORIGINAL NLP (dynamics + bounds on x,u)
    z = p.start_point()
    for k in range(p.N + 1):
        z[p.ip(k):p.ip(k) + 3] = x[:, k]
        if k < p.N:
            z[p.iu(k):p.iu(k) + 2] = u[:, k]
    c = p.eq(z)
    lay = p.eq_layout()
    dyn = np.array([abs(c[i]) for i, row in enumerate(lay) if row[0] in ("init", "dyn")])
    assert dyn.max() < 1e-7
    assert p.objective(z) == pytest.approx(r.f, abs=1e-7)


def test_batch_matches_oracle_and_is_permutation_invariant():
    """C2 generator: a batch through the batched API equals instance-by-instance oracle solves, and the result
    of an instance does not depend on its position in the batch."""
    import __graft_entry__ as ge
    ge.build()
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams
    import os
    B, N = (768 if (os.cpu_count() or 1) >= 64 else 96), 5       # the oracle needs ~0.2 s per instance and core
    b = sc.make_batch(B, N)
    s = BatchSolver(N, b["m"], max_batch=B)
    out = s.solve(b["variant"], b["x0"], b["u0"], b["xref"], b["A"], b["b"], b["Ts"], b["term"], SolverParams())
    torch.cuda.synchronize()
    st = out.status.cpu().numpy()
    xo, uo, ts = out.xopt.cpu().numpy(), out.uopt.cpu().numpy(), out.ts_opt.cpu().numpy()
    assert np.mean((st == 0) | (st == 1)) > 0.95
    perm = np.random.default_rng(0).permutation(B)
    out2 = s.solve(b["variant"][perm], b["x0"][perm], b["u0"][perm], b["xref"][perm], b["A"][perm], b["b"][perm],
                   b["Ts"][perm], b["term"][perm], SolverParams())
    torch.cuda.synchronize()
    assert np.array_equal(out2.xopt.cpu().numpy(), xo[perm])            # bit-exact: no cross-instance coupling
    assert np.array_equal(out2.status.cpu().numpy(), st[perm])
    from oracle import c_oracle
    ref = c_oracle.solve_batch(4, N, b["m"], b["x0"], b["u0"], b["xref"], b["A"], b["b"], b["Ts"],
                               threads=host_cpus())                 # the C restatement, every instance
    it_gpu = out.iters.cpu().numpy()
    n_tight = 0
    for i in range(B):
        feas_ref = ref["status"][i] in (0, 1)
        assert feas_ref == bool(st[i] in (0, 1))
        if feas_ref:
            same_path = ref["iters"][i] == it_gpu[i]
            tol = 1e-9 if same_path else 1e-5
            n_tight += same_path
            np.testing.assert_allclose(xo[i], ref["xopt"][i], rtol=0, atol=tol)
            np.testing.assert_allclose(uo[i], ref["uopt"][i], rtol=0, atol=tol)
            assert ts[i] == pytest.approx(ref["ts_opt"][i], abs=tol)
    # the structured and the dense solve take the same inertia decisions: nearly every instance follows the oracle's
    # iterate sequence exactly (the rest differ by roundoff in a pivot sign on long non-convex runs)
    assert n_tight >= int(0.85 * B)
    for i in range(4):                                                    # and the numpy specification on a few
        p = Problem(4, N, b["m"], b["x0"][i], b["u0"][i], b["xref"][i], b["A"][i], b["b"][i], sc.TS,
                    0.1 * np.eye(3), 0.01 * np.eye(2), 0.1 * np.eye(2), 0.1 * np.eye(3), sc.XL, sc.XU,
                    [-0.6, -np.pi / 6], [0.6, np.pi / 6], sc.EGO, sc.DMIN)
        r = ipm_dense.solve(p)
        np.testing.assert_allclose(xo[i], r.xopt, rtol=0, atol=1e-5)


def test_full_size_properties():
    """B = 8192 (BASELINE size): size-independent properties -- dynamics residual of every returned trajectory,
    bounds, time-scale consistency, and determinism of a repeated launch."""
    import __graft_entry__ as ge
    ge.build()
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams
    B, N = 8192, 5
    small = sc.make_batch(256, N)
    rep = B // 256
    b = {k: (np.concatenate([v] * rep) if isinstance(v, np.ndarray) else v) for k, v in small.items()}
    s = BatchSolver(N, b["m"], max_batch=B)
    out = s.solve(b["variant"], b["x0"], b["u0"], b["xref"], b["A"], b["b"], b["Ts"], b["term"], SolverParams())
    torch.cuda.synchronize()
    st = out.status.cpu().numpy()
    x, u, ts = out.xopt.cpu().numpy(), out.uopt.cpu().numpy(), out.ts_opt.cpu().numpy()
    ok = (st == 0) | (st == 1)
    assert ok.mean() > 0.95
    # replicas of the same instance give bit-identical answers wherever they sit in the grid
    assert np.array_equal(x[:256], x[-256:]) and np.array_equal(st[:256], st[-256:])
    h = ts[:, None]
    xn = x[:, 0, :-1] + h * u[:, 0] * np.cos(x[:, 2, :-1])
    yn = x[:, 1, :-1] + h * u[:, 0] * np.sin(x[:, 2, :-1])
    tn = x[:, 2, :-1] + h * u[:, 1]
    res = np.max(np.abs(np.stack([xn - x[:, 0, 1:], yn - x[:, 1, 1:], tn - x[:, 2, 1:]])), axis=(0, 2))
    assert res[ok].max() < 1e-7
    assert np.abs(x[ok, :, 0] - b["x0"][ok]).max() < 1e-7                 # initial condition
    assert np.abs(x[ok, :, -1] - b["xref"][ok][:, :, -1]).max() < 1e-7    # terminal equality of obca_mpc4
    assert np.abs(u[ok, 0]).max() <= 0.6 + 1e-7 and np.abs(u[ok, 1]).max() <= np.pi / 6 + 1e-7
    assert (ts[ok] > 0).all()


def test_headline_batch_against_the_independent_oracle():
    """The product path (obca_solve_batch, compile-time-shape wave kernel) against an oracle that shares NOTHING with it: oracle/
    ipopt_like.py -- IPOPT's published algorithm on the NLP as the reference poses it (hard equalities, slack bounds, restoration
    phase), from the reference's literal zero start.  Seeded C2 instances of the headline workload: same status (feasible), Ts_opt to
    2e-7 s, poses to 1e-6 m, objective to 1e-6 relative (tests/test_ipopt_like.py has the same check on the host build)."""
    import os
    from oracle import ipopt_like
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams
    cores = os.cpu_count() or 1
    B, N = 256, 5
    idx = list(range(0, B, 2 if cores >= 64 else 16))               # 128 instances on the GPU box's host (2-3 s each), 16 on a small one
    b = sc.make_batch(B, N)
    s = BatchSolver(N, b["m"], max_batch=B)
    out = s.solve(b["variant"], b["x0"], b["u0"], b["xref"], b["A"], b["b"], b["Ts"], b["term"], SolverParams())
    torch.cuda.synchronize()
    st, xo, uo, ts, info = (getattr(out, k).cpu().numpy() for k in ("status", "xopt", "uopt", "ts_opt", "info"))
    ref = ipopt_like.solve_c2_sample(B, N, idx, procs=min(host_cpus(), 64))
    n_ok = 0
    for i, (rst, rts, rf, rx, ru, nres) in zip(idx, ref):
        assert st[i] in (0, 1)
        if rst != ipopt_like.OK:
            continue                                                  # (the oracle alone ending elsewhere is its own matter: counted below)
        n_ok += 1
        assert ts[i] == pytest.approx(rts, abs=2e-7), i
        np.testing.assert_allclose(xo[i], rx, rtol=0, atol=1e-6)
        np.testing.assert_allclose(uo[i], ru, rtol=0, atol=1e-5)
        assert info[i, 0] == pytest.approx(rf, rel=1e-6)
    assert n_ok >= 0.95 * len(idx), (n_ok, len(idx))
    s.close()
