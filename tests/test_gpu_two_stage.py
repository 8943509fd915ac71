"""The batched two-stage open-loop planner on the device (…_amd/openloop.py; obca_plan_refine = csrc/obca_refine.hip on
csrc/obca_refine_core.h).

1. the refinement kernel against the host build of the same core (tests/test_plan_refine_core.py pins that one to the
   project's mirror of the reference word for word) at shapes that cross a block and a wavefront boundary;
2. the pipeline on demo1 / demo8 against ``closedLoop`` driven by the CPU build of the solver, as tests/test_gpu_open_loop.py
   does: stage 1 and stage 2's INPUTS against the CPU run, stage 2's outputs against the model (roundoff picks among
   equivalent plans of the long fixed-time solve);
3. a stage-1 failure (demo9 at N_free = 10, infeasible by construction) is masked and leaves no NaN behind;
4. obca_mpc8 answers an instance whose obca_mpc6 fails, and its neighbour is not disturbed."""
import functools
import math

import numpy as np
import pytest

from tests import kkt_check, native_build
from tests import test_plan_refine_core as core
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.closed_loop import closedLoop
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.demo_setting import problemSetting

pytestmark = pytest.mark.gpu
EGO, DMIN = (1.7, 0.75, 1.7, 0.75), 0.05
POS_TOL, TS_RTOL, YAW_TOL = 1e-12, 1e-14, 1e-9
STATUS_SKIPPED = -5


def _np(t):
    return t.detach().cpu().numpy()


def _check_refined(got_xref, got_ts, ref_xref, ref_ts, what):
    dp = float(np.abs(got_xref[:, :2] - ref_xref[:, :2]).max())
    dt = float(np.max(np.abs(got_ts - ref_ts) / np.abs(ref_ts)))
    dy = float(core.wrapped(got_xref[:, 2], ref_xref[:, 2]).max())
    print("%s: max |position - ref| %.3e m (words equal: %s), max rel |ts - ref| %.3e (words equal: %s), max yaw difference %.3e rad"
          % (what, dp, np.array_equal(core.words(got_xref[:, :2]), core.words(ref_xref[:, :2])), dt,
             np.array_equal(core.words(got_ts), core.words(ref_ts)), dy))
    assert dp <= POS_TOL and dt <= TS_RTOL and dy <= YAW_TOL


@pytest.mark.parametrize("B,N,ratio", [(67, 2, 2), (5, 5, 1), (3, 3, 4), (9, 13, 5)])
def test_kernel_matches_the_host_core(B, N, ratio):
    """335 lanes in two blocks; ratio 1; 13 points; 66 points per instance, so that instances straddle wavefronts"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.openloop import refine
    x, ts = core.random_plans(500 + B, B, N)
    status = np.array([0, 1, 2, 0, -1, 1, -5, 0, 0], np.int32)[np.arange(B) % 9]
    x[1, 1, N // 2] = np.nan                                       # one NaN plan, with a feasible status
    assert status[1] == 1
    host = core.host_refine(core.load_host(), x, ts, ratio, status=status)
    xref, ts_out, var = (_np(t) for t in refine(torch.as_tensor(x), torch.as_tensor(ts), ratio, torch.as_tensor(status)))
    torch.cuda.synchronize()
    assert xref.shape == (B, 3, ratio * N + 1) and np.isfinite(xref).all() and np.isfinite(ts_out).all()
    passed = (status > 1) | (status < 0)
    passed[1] = True
    assert np.array_equal(var, np.where(passed, 0, 6).astype(np.int32)) and np.array_equal(var, host["variant_out"])
    assert np.array_equal(core.words(xref[passed]), core.words(host["xref"][passed]))          # the fill, exactly
    assert np.array_equal(core.words(ts_out[passed]), core.words(host["ts_out"][passed]))
    fill, ts_fill = core.expected_fill(x, ts, ratio)
    assert np.array_equal(core.words(xref[passed]), core.words(fill[passed]))
    assert np.array_equal(core.words(ts_out[passed]), core.words(ts_fill[passed]))
    ok = ~passed
    _check_refined(xref[ok], ts_out[ok], host["xref"][ok], host["ts_out"][ok], "B %d N %d ratio %d" % (B, N, ratio))
    # variant_ok is what refined instances get, a NULL status counts as feasible
    _, _, var8 = refine(torch.as_tensor(x), torch.as_tensor(ts), ratio, None, variant_ok=8)
    expect = np.full(B, 8, np.int32)
    expect[1] = 0
    assert np.array_equal(_np(var8), expect)


def test_refused_calls_raise():
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.openloop import refine
    x, ts = core.random_plans(541, 2, 5)
    for kw in (dict(ratio=0), dict(ratio=26), dict(ratio=2, variant_ok=5)):
        with pytest.raises(RuntimeError, match="code -22"):
            refine(torch.as_tensor(x), torch.as_tensor(ts), **kw)


def _dyn_res(x, u, h):
    nxt = x[:, :-1] + h * np.stack([u[0] * np.cos(x[2, :-1]), u[0] * np.sin(x[2, :-1]), u[1]])
    return float(np.max(np.abs(nxt - x[:, 1:])))


def _gpu_plan(demo, n_free, ratio, B, term_edit=None):
    """the device planner on B copies of a demo: numpy copies of everything ``plan`` returns, and the arguments"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import openloop
    a = openloop.from_settings([problemSetting(demo) for _ in range(B)])
    if term_edit is not None:
        term_edit(a.term)
    pl = openloop.TwoStagePlanner(n_free, ratio, a.m_static, a.n_box, max_batch=B)
    p = pl.plan(**a.kwargs())
    torch.cuda.synchronize()
    out = {"args": a, "m_fix": a.m_static + [4] * a.n_box}
    for stage in ("free", "fix"):
        r = getattr(p, stage)
        out[stage] = {k: _np(getattr(r, k)) for k in ("xopt", "uopt", "ts_opt", "status", "iters")}
    for k in ("xref_fix", "ts_fix", "A_fix", "b_fix", "term", "variant_fix", "feas"):
        out[k] = _np(getattr(p, k))
    pl.close()
    return out


@functools.lru_cache(maxsize=None)
def _pipeline(demo, n_free):
    """B = 3 copies at ratio 2 on the device, and the CPU run of the mirror with its recorded solver calls"""
    g = _gpu_plan(demo, n_free, 2, 3)
    cpu = native_build.LpiObca()
    cl = closedLoop(problemSetting(demo), solver=cpu)
    cl.N_free, cl.N_fix = n_free, 2 * n_free
    cl.mpc_openLoop_freeTime()
    free = (np.array(cl.xOpt), np.array(cl.uOpt), bool(cl.feas), float(cl.Ts_opt))
    cl.mpc_openLoop_fixTime()
    return g, dict(free=free, feas=bool(cl.feas), call6=[q for q in cpu.calls if q["variant"] == 6][0], cl=cl)


@pytest.mark.parametrize("demo,n_free", [("demo1", 10), ("demo8", 5)])
def test_pipeline_against_the_host_mirror(demo, n_free):
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.openloop import refine
    g, c = _pipeline(demo, n_free)
    n_fix, B = 2 * n_free, 3
    xf, uf, ts_f = g["free"]["xopt"], g["free"]["uopt"], g["free"]["ts_opt"]
    # stage 1 against the CPU run (the tolerances of tests/test_gpu_open_loop.py)
    assert c["free"][2] and np.all(g["free"]["status"] <= 1) and np.all(g["free"]["status"] >= 0)
    for i in range(B):
        np.testing.assert_allclose(xf[i], c["free"][0], rtol=0, atol=1e-6)
        np.testing.assert_allclose(uf[i], c["free"][1], rtol=0, atol=1e-6)
        assert ts_f[i] == pytest.approx(c["free"][3], abs=1e-8)
    # stage 2's inputs against the CPU's recorded obca_mpc6 call
    call = c["call6"]
    assert g["m_fix"] == call["m"] and g["xref_fix"].shape == (B, 3, n_fix + 1)
    np.testing.assert_allclose(g["ts_fix"], n_free * ts_f / n_fix, rtol=1e-12, atol=0)
    for i in range(B):
        assert g["ts_fix"][i] == pytest.approx(call["Ts"], abs=1e-8)
        np.testing.assert_allclose(g["A_fix"][i], call["A"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(g["b_fix"][i], call["b"], rtol=0, atol=1e-5)
        assert np.array_equal(g["term"][i], call["term"])
        np.testing.assert_allclose(g["xref_fix"][i, :2], call["xref"][:2], rtol=0, atol=1e-6)
    # refine of the GPU's own stage-1 plan against the numpy mirror of that same plan
    ref, ts_ref = core.mirror_batch(xf, ts_f, 2)
    _check_refined(g["xref_fix"], g["ts_fix"], ref, ts_ref, "%s pipeline" % demo)
    xr, tr, vr = refine(torch.as_tensor(xf), torch.as_tensor(ts_f), 2, torch.as_tensor(g["free"]["status"]))
    assert np.array_equal(core.words(_np(xr)), core.words(g["xref_fix"])) and np.array_equal(core.words(_np(tr)), core.words(g["ts_fix"]))
    assert np.all(_np(vr) == 6)
    # the three copies equal each other word for word, inputs and outputs
    for k in ("xref_fix", "ts_fix", "A_fix", "b_fix"):
        assert np.array_equal(core.words(g[k][1:]), core.words(g[k][:1].repeat(2, 0))), k
    for stage in ("free", "fix"):
        for k in ("xopt", "uopt", "ts_opt"):
            assert np.array_equal(core.words(g[stage][k][1:]), core.words(g[stage][k][:1].repeat(2, 0))), (stage, k)
        assert len(set(g[stage]["iters"].tolist())) == 1 and len(set(g[stage]["status"].tolist())) == 1
    # stage 2's outputs against the model
    assert c["feas"] and g["feas"].all() and np.all((g["fix"]["status"] == 0) | (g["fix"]["status"] == 1))
    assert np.all((g["variant_fix"] == 6) | (g["variant_fix"] == 8))
    x2, u2, ts2 = g["fix"]["xopt"][0], g["fix"]["uopt"][0], float(g["fix"]["ts_opt"][0])
    assert ts2 == pytest.approx(n_free * float(ts_f[0]) / n_fix, rel=1e-12)        # fixed time: Ts_opt <- N_free Ts_opt / N_fix
    assert _dyn_res(x2, u2, ts2) < 1e-7
    assert np.abs(u2[0]).max() <= 0.6 + 1e-7 and np.abs(u2[1]).max() <= math.pi / 6 + 1e-7
    clear = kkt_check.min_clearance(x2, EGO, g["m_fix"], g["A_fix"][0], g["b_fix"][0])
    print("%s: obca_mpc%d answered, %d iterations, clearance at the knots %.4f m" % (demo, g["variant_fix"][0], g["fix"]["iters"][0], clear))
    assert clear >= DMIN - 1e-6
    if g["variant_fix"][0] == 6:
        t = g["term"][0]
        assert x2[0, -1] >= t[0] - 1e-6 and t[1] - 1e-6 <= x2[1, -1] <= t[2] + 1e-6


def test_stage_one_failure_is_masked():
    """demo9 at N_free = 10 has no feasible free-time plan (tests/test_gpu_open_loop.py): stage 2 is skipped, nothing is NaN"""
    g = _gpu_plan("demo9", 10, 2, 2)
    assert np.all(g["free"]["status"] == 2)
    assert np.all(g["variant_fix"] == 0) and np.all(g["fix"]["status"] == STATUS_SKIPPED) and not g["feas"].any()
    assert np.all(g["fix"]["iters"] == 0)
    for k in ("xref_fix", "ts_fix", "A_fix", "b_fix"):
        assert np.isfinite(g[k]).all(), k
    for k in ("xopt", "uopt", "ts_opt"):
        assert np.isfinite(g["fix"][k]).all(), k
    assert g["xref_fix"].shape == (2, 3, 21) and g["A_fix"].shape == (2, 21, 18, 2)


def test_mpc8_answers_a_failed_mpc6():
    """instance 1's terminal set cannot be reached: the terminal screen answers its obca_mpc6 without a solve (iters 0), so
    what ``fix.iters`` reports for it is the obca_mpc8 launch's count alone; instance 0 is the pipeline test's answer"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver

    def edit(term):
        term[1, 0] = 1e3
    g = _gpu_plan("demo8", 5, 2, 2, term_edit=edit)
    base, _ = _pipeline("demo8", 5)
    assert g["variant_fix"][1] == 8 and g["feas"][1] and g["fix"]["status"][1] in (0, 1)
    assert g["term"][1, 0] == 1e3
    assert g["variant_fix"][0] == base["variant_fix"][0] and g["fix"]["iters"][0] == base["fix"]["iters"][0]
    for k in ("xopt", "uopt", "ts_opt"):
        assert np.array_equal(core.words(g["fix"][k][0]), core.words(base["fix"][k][0])), k
    # the obca_mpc8 launch alone, on the inputs the planner built
    a = g["args"]
    s = BatchSolver(10, g["m_fix"], max_batch=1)
    out = s.solve(8, a.start[1:2], np.zeros((1, 2)), g["xref_fix"][1:2], g["A_fix"][1:2], g["b_fix"][1:2], g["ts_fix"][1:2],
                  g["term"][1:2], a.params)
    torch.cuda.synchronize()
    assert int(out.status[0]) in (0, 1) and int(out.iters[0]) > 0
    assert g["fix"]["iters"][1] == int(out.iters[0])
    assert np.array_equal(core.words(_np(out.xopt)[0]), core.words(g["fix"]["xopt"][1]))
    s.close()
    x2, u2 = g["fix"]["xopt"][1], g["fix"]["uopt"][1]
    assert _dyn_res(x2, u2, float(g["fix"]["ts_opt"][1])) < 1e-7
    assert kkt_check.min_clearance(x2, EGO, g["m_fix"], g["A_fix"][1], g["b_fix"][1]) >= DMIN - 1e-6
