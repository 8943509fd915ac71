"""GPU tier of the fleet's prediction by plans: obca_fleet_tracks and obca_scene_select_staged against their host cores
(tests/test_fleet_tracks_core.py, tests/test_staged_select_core.py), and ``scene.FleetLoop(predict="plan")`` against
``scene.PoolLoop``, against the velocity loop and against the host loop of tests/test_fleet_plan_loop_host.py.

Words and bounds.  obca_fleet_tracks: masks and spares word for word, rows word for word at heading 0 with dyadic numbers and
within tests/test_fleet_core.py's A_TOL / ROW_TOL elsewhere (the device's sin / cos against the host libm's).
obca_scene_select_staged: scores and min_clear within TOL = 1e-9 m, the bound tests/test_gpu_fleet.py uses for rotated
rectangles; selection, masks, fill and gathered rows exactly -- a selection could differ between host and device only where
two scores of a pool are closer than TOL, and the generator keeps all scores of every pool more than SEPARATION = 1e-6 m apart,
which ``staged_cases`` asserts on the host's scores.  The loop: every solve within TOL of the host yardstick, re-seeded from
the device's state before each step (the idiom of tests/test_gpu_fleet.py::test_a_parked_car_is_an_obstacle)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_fleet_core as core
from tests import test_fleet_loop_host as fl
from tests import test_fleet_plan_loop_host as plh
from tests import test_fleet_tracks_core as ftc
from tests import test_gpu_fleet as tgf
from tests import test_gpu_scene as tgs
from tests import test_pool_loop_core as plc
from tests import test_scene_core as tsc
from tests import test_staged_select_core as ssc
from tests.descriptor_case import PAD, TOL, _np, check_struct_mirror, device_descriptor_call
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib, scene
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver

pytestmark = pytest.mark.gpu

SEPARATION = 1e-6
RUN, GOAL, CAP, FAILED, COLLISION = core.RUN, core.GOAL, core.CAP, core.FAILED, core.COLLISION
N, S, TS, N_SEL, KS = fl.N, fl.S, fl.TS, fl.N_SEL, fl.KS


# ------------------------------------------------------------------------------------------------ 1. obca_fleet_tracks
@pytest.fixture(scope="module")
def tracks_host():
    return ftc.load_host()


def device_tracks(case, rc=0, null=(), device=None, **over):
    """obca_fleet_tracks itself on the buffers of ``case`` uploaded between sentinels (``device_descriptor_call``)"""
    return device_descriptor_call(case, _lib.load().obca_fleet_tracks, (), ftc.READ, ftc.INT, rc=rc, null=null, device=device, **over)


def mixed_plans(G, V, N_, rng, exact, see):
    """``ftc.fill_plans`` with what a running fleet holds: car 1 of every world has ended (GOAL in even worlds, FAILED in odd
    ones), car 0 of world 0 did not step, the last car of the last world has no pose, one plan has a word that is no number and
    one solve is infeasible"""
    c = ftc.fill_plans(ftc.Case(G, V, N_, step=3, see=see, margin=0.25, exact=exact), rng)
    B = G * V
    if V > 1:
        for g in range(G):
            c["flags"][g * V + 1] = GOAL if g % 2 == 0 else FAILED
        c["k"][0] = 3
        c["x0"][B - 1, 1] = np.nan
    if V > 2:
        c["xopt"][2, 1, N_] = np.inf
        c["status"][B - 2] = 2
    return c


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rotated"))
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 5), (2, 16, 127), (1, 16, 1)], ids=lambda s: "G%d_V%d_N%d" % s)
def test_tracks_kernel_equals_the_host_core(tracks_host, shape, exact):
    """both ``see`` values on every shape, all plans usable and the mixed world: one car, the longest horizon with sixteen cars
    (V (N + 1) = 2048 pairs for 256 threads), the shortest"""
    G, V, N_ = shape
    worst = 0.0
    for see in (core.SEE_ALL, core.SEE_LOWER):
        rng = np.random.default_rng(100 * G + V + N_)
        for mixed in (False, True):
            c = mixed_plans(G, V, N_, rng, exact, see) if mixed else \
                ftc.fill_plans(ftc.Case(G, V, N_, step=3, see=see, margin=0.25, exact=exact), rng)
            dev = device_tracks(c)
            ftc.tracks_host(tracks_host, c)
            want = dict(c.a)
            want["_car"] = ftc.car_mask(c)
            worst = max(worst, ftc.compare(c, dev, want, label=(see, mixed)))
            if mixed and V > 1:
                assert np.all(c["track_ok"][:, 1] == 0) and np.all(c["track_ok"][:V, 0] == 0)
            if not mixed and V > 1:
                assert c["track_ok"][V - 1, 0] == 1
    print("G %d V %d N %d %s: largest |device - host| rows %.3e (bound %.3e)" % (G, V, N_, "exact" if exact else "rotated", worst,
                                                                               core.ROW_TOL))
    if exact:
        assert worst == 0.0


def test_refused_tracks_calls_launch_nothing():
    rng = np.random.default_rng(6)
    c = mixed_plans(2, 3, 4, rng, False, core.SEE_ALL)
    for over in ftc.REFUSED:
        device_tracks(c, rc=ftc.E_INVAL, **over)
    for name in ftc.READ + ftc.WRITTEN:
        device_tracks(c, rc=ftc.E_INVAL, null=(name,))
    device_tracks(c, rc=ftc.E_INVAL, device=-1)
    assert _lib.load().obca_fleet_tracks(None, 0, None) == ftc.E_INVAL
    check_struct_mirror(None, _lib.load().obca_fleet_tracks_init, _lib.ObcaFleetTracks)


# ------------------------------------------------------------------------------------------------ 2. obca_scene_select_staged
@pytest.fixture(scope="module")
def staged_host():
    return ssc.load_host()


def device_select_staged(pool_A, pool_b, x, n_sel, stage=None, pool_v=None, Ts=None, x0=None, variant=None, status=None, n_sub=1,
                         state=None):
    """obca_scene_select_staged itself on guarded outputs: numpy in, numpy out (the sentinels are checked here).  stage:
    (stage_A, stage_b, stage_ok, stage_group), or None for Kt = 0 with NULL pointers"""
    B, K, E = pool_b.shape
    N_ = x.shape[2] - 1
    g = tgs._guarded(B, K, E, N_, n_sel)
    up = lambda a, dt=torch.float64: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    ins = [up(pool_A), up(pool_b), up(pool_v), up(Ts), up(x), up(x0), up(variant, torch.int32), up(status, torch.int32)]
    sA, sb, sok, group = stage if stage is not None else (None, None, None, 1)
    st = [up(sA), up(sb), up(sok, torch.int32)]
    Kt = 0 if sok is None else sok.shape[1]
    if state is not None:
        g["score"][1].copy_(up(state[0]))
        g["sel"][1].copy_(up(state[1], torch.int32))
    rc = _lib.load().obca_scene_select_staged((ctypes.c_double * 4)(*tsc.EGO), B, K, E, N_, n_sel, n_sub, 0 if state is None else 1,
                                              *[tgs._ptr(t) for t in ins], Kt, group, *[tgs._ptr(t) for t in st],
                                              *[tgs._ptr(g[k][1]) for k in ("score", "sel", "A", "b", "variant_out", "ok", "min_clear")],
                                              torch.cuda.current_device(), _lib.stream_ptr(torch.device("cuda")))
    assert rc == 0
    torch.cuda.synchronize()
    for name, (buf, view, fill) in g.items():
        assert (buf[:PAD] == fill).all() and (buf[-PAD:] == fill).all(), name
    return {k: v[1].cpu().numpy() for k, v in g.items()}


def assert_all_separated(score, ok):
    """all scores of every usable pool are more than SEPARATION apart: host and device rank them alike"""
    if score.shape[1] > 1:
        s = np.sort(score[ok == 1], axis=1)
        assert np.all(np.diff(s, axis=1) > SEPARATION)


# B, K, Kt, E, N, n_sub, stage_group: every B of {1, 5}, K of {1, 4, 64}, Kt of {0, 1, 16, K}, E of 1 .. 4, N of {1, 5, 127},
# n_sub of {1, 16}, stage_group 1 and V (= 5: one block for the ragged batch)
STAGED_CASES = [(1, 1, 1, 1, 1, 1, 1), (5, 4, 1, 2, 5, 16, 1), (5, 4, 4, 4, 5, 1, 5), (5, 64, 16, 4, 5, 16, 5), (1, 64, 64, 3, 5, 1, 1),
                (5, 64, 16, 4, 127, 1, 1), (5, 4, 0, 4, 5, 16, 1), (5, 64, 1, 1, 1, 16, 5)]


def staged_cases(host, case):
    """the inputs of one case and the host's outputs of both calls: mode 0 from a reference and x0, then mode 1 on plans next
    to it with every kind of instance (variant 4 and 8, status 0, 1 and 2, masked).  The separation of the host's scores is
    asserted here, for both calls."""
    B, K, Kt, E, N_, n_sub, group = case
    rng = np.random.default_rng(sum(c * 7 ** i for i, c in enumerate(case)))
    pool_A, pool_b = tsc.random_pool(rng, B, K, E, (1.0, 12.0 + min(N_, 20)), (-3.0, 13.0))
    x, x0 = tsc.random_poses(rng, B, N_)
    if N_ > 20:                                                    # a long horizon stays in the corridor: 0.1 m steps
        x[:, :2] = x[:, :2, :1] + 0.1 * (x[:, :2] - x[:, :2, :1])
    v, Ts = rng.uniform(-0.5, 0.5, (B, K, 2)), rng.uniform(0.5, 1.5, B)
    variant = np.array([8, 4, 8, 0, 8], np.int32)[:B] if B > 1 else np.array([4], np.int32)
    status = np.array([0, 1, 2, 0, 1], np.int32)[:B]
    n_sel = min(3, K)
    stage = None
    if Kt > 0:
        sA, sb = ssc.turning_track(rng, B // group, Kt, N_, E, turn=0.3 if N_ <= 20 else 0.02)
        ok = rng.integers(0, 4, (B, Kt)).astype(np.int32)          # three in four staged, any non-zero word counts
        ok[0, 0] = 1
        stage = (sA, sb, ok, group)
    kw = dict(pool_v=v, Ts=Ts, variant=variant, n_sub=n_sub)
    hkw = {} if stage is None else dict(stage_A=stage[0], stage_b=stage[1], stage_ok=stage[2], stage_group=group)
    h0 = ssc.host_select_staged(host, pool_A, pool_b, x, n_sel, x0=x0, **hkw, **kw)
    assert_all_separated(h0["score"], h0["ok"])
    plan = x + rng.uniform(-0.3, 0.3, x.shape)
    h1 = ssc.host_select_staged(host, pool_A, pool_b, plan, n_sel, status=status, state=(h0["score"], h0["sel"]), **hkw, **kw)
    assert_all_separated(h1["score"], h1["ok"])
    return dict(pool_A=pool_A, pool_b=pool_b, x=x, x0=x0, plan=plan, n_sel=n_sel, stage=stage, status=status, kw=kw), h0, h1


@pytest.mark.parametrize("case", STAGED_CASES, ids=lambda c: "B%d_K%d_Kt%d_E%d_N%d_sub%d_g%d" % c)
def test_staged_kernel_equals_the_host_core(staged_host, case):
    a, h0, h1 = staged_cases(staged_host, case)
    d0 = device_select_staged(a["pool_A"], a["pool_b"], a["x"], a["n_sel"], stage=a["stage"], x0=a["x0"], **a["kw"])
    tgs.assert_same(d0, h0, a["n_sel"])
    d1 = device_select_staged(a["pool_A"], a["pool_b"], a["plan"], a["n_sel"], stage=a["stage"], status=a["status"],
                              state=(d0["score"], d0["sel"]), **a["kw"])
    tgs.assert_same(d1, h1, a["n_sel"])
    assert np.all(h0["ok"] == 1)
    if case[2] == 0:                                               # Kt = 0: obca_scene_select's device words
        p0 = tgs.device_select(a["pool_A"], a["pool_b"], a["x"], a["n_sel"], x0=a["x0"], **a["kw"])
        p1 = tgs.device_select(a["pool_A"], a["pool_b"], a["plan"], a["n_sel"], status=a["status"], state=(p0["score"], p0["sel"]),
                               **a["kw"])
        assert ssc.same_outputs(d0, p0) and ssc.same_outputs(d1, p1)


def test_unstaged_slots_and_spoilt_tracks_on_the_device(staged_host):
    """every stage_ok 0 over tracks of NaN: obca_scene_select's device words; a NaN or a zero row in a staged track: the fill,
    as the host core gives it"""
    a, h0, _ = staged_cases(staged_host, (5, 4, 4, 4, 5, 1, 5))
    sA, sb, ok, group = a["stage"]
    none = (np.full_like(sA, np.nan), np.full_like(sb, np.nan), np.zeros_like(ok), group)
    d = device_select_staged(a["pool_A"], a["pool_b"], a["x"], a["n_sel"], stage=none, x0=a["x0"], **a["kw"])
    p = tgs.device_select(a["pool_A"], a["pool_b"], a["x"], a["n_sel"], x0=a["x0"], **a["kw"])
    assert ssc.same_outputs(d, p)
    for spoil in ("nan", "zero row"):
        sA2, ok2 = sA.copy(), ok.copy()
        ok2[:, 2] = (1, 0, 1, 1, 1)                                # instance 1 does not read slot 2's track
        if spoil == "nan":
            sA2[0, 2, 5, 3, 1] = np.nan
        else:
            sA2[0, 2, 3, 1] = 0.0
        h = ssc.host_select_staged(staged_host, a["pool_A"], a["pool_b"], a["x"], a["n_sel"], stage_A=sA2, stage_b=sb, stage_ok=ok2,
                                   stage_group=group, x0=a["x0"], **a["kw"])
        d = device_select_staged(a["pool_A"], a["pool_b"], a["x"], a["n_sel"], stage=(sA2, sb, ok2, group), x0=a["x0"], **a["kw"])
        assert list(h["ok"]) == [0, 1, 0, 0, 0]
        tgs.assert_same(d, h, a["n_sel"])


def test_the_python_wrappers_are_the_calls(staged_host):
    """``scene.fleet_tracks`` and ``scene.select`` with stage rows give the words of the C calls on the same inputs"""
    c = mixed_plans(3, 3, 5, np.random.default_rng(8), False, core.SEE_LOWER)
    out = scene.fleet_tracks(c["x0"], c["flags"], c["k"], c["xopt"], c["status"], 3, 3, see="lower", margin=0.25)
    dev = device_tracks(c)
    for k in ftc.WRITTEN:
        assert core.same_words(_np(out[k]), dev[k]), k
    a, _, _ = staged_cases(staged_host, (5, 4, 4, 4, 5, 1, 5))
    sA, sb, ok, group = a["stage"]
    s = scene.select(a["pool_A"], a["pool_b"], a["x"], a["n_sel"], x0=a["x0"], stage_A=sA, stage_b=sb, stage_ok=ok, stage_group=group,
                     **a["kw"])
    d = device_select_staged(a["pool_A"], a["pool_b"], a["x"], a["n_sel"], stage=a["stage"], x0=a["x0"], **a["kw"])
    torch.cuda.synchronize()
    assert ssc.same_outputs({k: _np(s[k]) for k in ssc.OUT}, d)
    with pytest.raises(ValueError):
        scene.select(a["pool_A"], a["pool_b"], a["x"], a["n_sel"], stage_A=sA, stage_b=sb, **a["kw"])          # no stage_ok


# ------------------------------------------------------------------------------------------------ 3. the loop
@pytest.fixture(scope="module")
def hosts():
    return plc.load_host(), ssc.load_host(), core.load_host(), ftc.load_host()


def test_one_car_per_world_is_pool_loops_words():
    """V = 1 under "plan": the only agent slot is a spare and its mask word is 0, so every history equals a plain ``PoolLoop``
    over the same static pool with the spare appended by hand"""
    w = fl.head_on_world(2)
    solver, lp = tgf.make_fleet(w, 1, margin=fl.MARGIN, predict="plan")
    got = tgf.read_np(lp.run())
    ps, plain = tgf.make_plain(w, 1)
    ref = tgf.read_np(plain.run())
    for k in ref:
        assert core.same_words(got[k], ref[k]), k
    assert np.all(got["flags"] == GOAL) and not _np(lp.track_ok).any()
    solver.close()
    ps.close()


def test_the_first_step_is_the_velocity_loops():
    """before any plan exists every mask word is 0: after one step the two loops hold the same words; after the second they
    do not (car 1 has seen car 0's plan)"""
    w = plh.cut_in_world(G=2)
    solver, lp = tgf.make_fleet(w, 2, see="lower", margin=fl.MARGIN, predict="plan")
    vs, lv = tgf.make_fleet(w, 2, see="lower", margin=fl.MARGIN)
    a, b = tgf.read_np(lp.run(1)), tgf.read_np(lv.run(1))
    for k in b:
        assert core.same_words(a[k], b[k]), k
    assert list(_np(lp.track_ok).reshape(-1)) == [0, 0, 1, 0] * 2
    a, b = tgf.read_np(lp.run(1)), tgf.read_np(lv.run(1))
    assert core.same_words(a["x_closed"][0::2], b["x_closed"][0::2]) and not core.same_words(a["x_closed"][1::2], b["x_closed"][1::2])
    solver.close()
    vs.close()


def test_cut_in_plan_passes_where_velocity_fails(hosts):
    """the cut-in worlds of tests/test_fleet_plan_loop_host.py.  predict="velocity": a solve of car 1 goes infeasible and it
    ends FAILED -- this is the contrast that fails without the feature.  predict="plan": every solve is held to the host
    yardstick (staged host select on the device's tracks, host solver), re-seeded from the device's state before every step;
    every solve is feasible, car 0 reaches its goal, car 1 does not fail and agent_clear >= 0 throughout."""
    G = 2
    w = plh.cut_in_world(G=G)
    vs, lv = tgf.make_fleet(w, 2, see="lower", margin=fl.MARGIN)
    ref = tgf.read_np(lv.run())
    print("velocity: flags %s steps %s agent_min_clear %s" % (ref["flags"].tolist(), ref["steps"].tolist(), ref["agent_min_clear"].tolist()))
    assert np.all(ref["flags"][1::2] == FAILED) and np.all(ref["flags"][0::2] == GOAL)
    vs.close()

    solver, lp = tgf.make_fleet(w, 2, see="lower", margin=fl.MARGIN, predict="plan")
    B = 2 * G
    c, f = fl.host_cases(w, 2, see="lower", margin=fl.MARGIN)
    t = plh.tracks_case(c, f, 2)
    Ts = np.full(B, TS)
    worst = 0.0
    for step in range(S):
        torch.cuda.synchronize()
        for k, name in (("x0", "x0"), ("u0", "u0"), ("xref_out", "xref"), ("variant_out", "variant_out"), ("pool_A", "pool_A"),
                        ("pool_b", "pool_b"), ("pool_v", "pool_v")):
            c[k][...] = _np(getattr(lp, name))
        for k in ("track_A", "track_b", "track_ok"):
            t[k][...] = _np(getattr(lp, k))
        s, o, on = plh.host_step_plan(hosts[1], c, t, Ts, 2)
        assert np.all(np.isin(o["status"][on], (0, 1))), (step, o["status"])          # the scenario's own condition
        lp.step()
        torch.cuda.synchronize()
        r, sel = lp._last
        assert np.array_equal(_np(sel)[on], s["sel"][on]) and np.array_equal(_np(r.status), o["status"]), step
        for k in ("xopt", "uopt", "ts_opt"):
            diff = float(np.max(np.abs(_np(getattr(r, k)) - o[k])[on])) if on.any() else 0.0
            worst = max(worst, diff)
            assert diff < TOL, (step, k, diff)
    got = tgf.read_np(lp)
    print("plan: flags %s steps %s agent_min_clear %s; largest |device - host| of a single solve %.3e"
          % (got["flags"].tolist(), got["steps"].tolist(), got["agent_min_clear"].tolist(), worst))
    assert np.all(got["flags"][0::2] == GOAL) and np.all(got["flags"][1::2] != FAILED)
    assert np.all(got["agent_clear"] >= 0.0) and np.all(np.isfinite(got["agent_min_clear"]))
    lp.step()                                                      # beyond the cap nobody steps: every mask word 0
    torch.cuda.synchronize()
    assert not _np(lp.track_ok).any()
    solver.close()


def test_plan_refuses_rounds_and_unknown_words():
    w = fl.head_on_world(1)
    solver = BatchSolver(N, [4] * N_SEL, 2)
    args = (w["pool_A"], w["pool_b"], w["start"], w["goal"], w["path"], w["path_len"])
    with pytest.raises(ValueError):
        scene.FleetLoop(solver, 2, *args, TS, predict="plan", rounds=1)
    with pytest.raises(ValueError):
        scene.FleetLoop(solver, 2, *args, TS, predict="plans")
    solver.close()


def test_plan_run_on_a_side_stream_gives_the_same_words():
    w = plh.cut_in_world(G=2)
    solver, lp = tgf.make_fleet(w, 2, see="lower", margin=fl.MARGIN, predict="plan")
    ref = tgf.read_np(lp.run())
    ins = {k: torch.as_tensor(v, device="cuda") for k, v in w.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lp2 = scene.FleetLoop(solver, 2, ins["pool_A"], ins["pool_b"], ins["start"], ins["goal"], ins["path"], ins["path_len"], TS,
                              see="lower", margin=fl.MARGIN, predict="plan", max_steps=S, goal_tol2=fl.GOAL_TOL2).run()
    del ins
    junk = [torch.full((4, KS + 2, 4, 2), 7.0, dtype=torch.float64, device="cuda") for _ in range(16)]
    torch.cuda.synchronize()
    del junk
    got = tgf.read_np(lp2)
    for k in ref:
        assert core.same_words(got[k], ref[k]), k
    assert np.all(ref["flags"][0::2] == GOAL)
    solver.close()
