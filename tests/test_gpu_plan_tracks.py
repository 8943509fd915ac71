"""GPU tier of the plans measured against timed tracks: obca_plan_tracks against its host core
(tests/test_plan_tracks_core.py), ``scene.plan_track_clearance`` against the raw C call, and ``scene.solve_tracks`` against
``scene.solve_scene``, against ``solver.solve`` and against the host loop of tests/test_solve_tracks_host.py.

Words and bounds, as on the CPU tier.  States and the placement of +inf, NaN and untouched words are compared word for word
(the knot times and the track's pose round every operation on their own on host and device); distances are within
tests/test_fleet_core.py's DIST_TOL = 1e-12 m (the device contracts the measurement's products and has its own sin and cos;
coordinates stay below 100 m).  ``solve_tracks``: every solve within TOL = 1e-9 of the host yardstick re-seeded from the
device's inputs (tests/test_gpu_pool_tracks.py's tolerance for the same comparison)."""
import numpy as np
import pytest
import torch

from tests import test_fleet_core as core
from tests import test_plan_tracks_core as pc
from tests import test_pool_tracks_core as ptc
from tests import test_solve_tracks_host as sth
from tests.descriptor_case import TOL, _np, check_struct_mirror, device_descriptor_call
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib, scene
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return pc.load_host()


# ------------------------------------------------------------------------------------------------ 1. kernel against host core
def device_call(case, rc=0, null=(), device=None, stream=None, **over):
    """obca_plan_tracks itself on the buffers of ``case`` uploaded between sentinels (``device_descriptor_call``)"""
    return device_descriptor_call(case, _lib.load().obca_plan_tracks, (), pc.READ, pc.INT, rc=rc, null=null, device=device,
                                  stream=stream, **over)


def both(host, case, label="", null=()):
    """the device on the buffers as they are, then the host core in place; compared by the CPU tier's rules.  Returns the
    device's buffers and the largest deviation of a distance"""
    dev = device_call(case, null=null)
    pc.call_host(host, case, null=null)
    return dev, pc.compare(case, dev, case.a, label=label)


@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.SHAPE_ID)
def test_kernel_equals_the_host_core(host, shape):
    """the CPU tier's shapes and worlds -- one plan with one one-knot track and two samples, a ragged batch (B = 5, 6: a
    workgroup with idle wavefronts, two workgroups), the longest horizon with sixteen tracks (508 samples for 64 lanes), every
    slot tracked (Kt = K = 64: both halves of the state masks, 10 samples) -- with every optional pointer given and NULL"""
    B, Kt, N, L, group, n_sub = shape
    rng = np.random.default_rng(sum(c * 11 ** i for i, c in enumerate(shape)) + 1)
    worst = 0.0
    for exact, null in ((True, ()), (False, ()), (False, ("x0",)), (False, ("variant", "status", "t0")), (False, ("score",))):
        case = pc.fill_world(pc.Case(B, Kt, N, L, group, n_sub, null=null), rng, exact=exact)
        _, d = both(host, case, label=(shape, exact, null))
        worst = max(worst, d)
    print("%s: largest |device - host| of a distance %.3e (bound %.3e)" % (pc.SHAPE_ID(shape), worst, pc.DIST_TOL))


@pytest.mark.parametrize("with_x0", (False, True), ids=("plan", "plan_and_x0"))
@pytest.mark.parametrize("N,n_sub", ((7, 8), (8, 7), (5, 12)), ids=("63", "64", "65"))
def test_lane_layout_edges(host, N, n_sub, with_x0):
    """63, 64 and 65 samples per track for 64 lanes, and one more with x0; B = 5: a ragged last workgroup.  The nearest sample
    of plan 0 is put at the last index, the one a wrong stride would drop."""
    rng = np.random.default_rng(100 * N + n_sub)
    case = pc.fill_world(pc.Case(5, 3, N, 4, 1, n_sub, null=() if with_x0 else ("x0",)), rng, mixed=False)
    case["track_len"][0, 0] = 1
    case["track_x"][0, 0, 0] = case["x0"][0] if with_x0 else case["x"][0, :, N]
    dev, d = both(host, case, label=(N, n_sub, with_x0))
    assert dev["track_clear"][0, 0] < -0.7 and np.all(np.isfinite(dev["track_min"]))
    print("N %d n_sub %d x0 %s: largest |device - host| %.3e" % (N, n_sub, with_x0, d))


def test_edge_content_on_the_device(host):
    """what the CPU tier checks one by one, on the device against the host core: every reason a track is unusable, lengths
    outside 1 .. L, x0, poses that are not finite at one knot and at every knot, distances and knot differences that overflow,
    the score's folding rules, numbers that are not dyadic, the track between the stage times"""
    for why in ptc.REASONS + ["nan_ts", "zero_ts", "negative_ts", "inf_t0"]:
        case, state = pc.spoilt_case(why, np.random.default_rng(67))
        dev, _ = both(host, case, label=why)
        assert dev["track_state"][0, 1] == state
    for ln in (-1, 4, 2 ** 31 - 1, -2 ** 31):
        case = pc.fill_world(pc.Case(3, 4, 5, 3, 1, 2), np.random.default_rng(29), mixed=False)
        case["track_len"][:, 3] = ln
        dev, _ = both(host, case, label=ln)
        assert np.all(dev["track_state"][:, 3] == -1)
    knots, times = np.array([(0.0, 10.0, 0.0)]), np.array([0.0])
    c = pc.one_plan(knots, times, pc.STRAIGHT, 1.5, size=core.EGO_OFF, x0=(0.0, 7.0, 0.0))
    dev, _ = both(host, c, label="x0")
    assert dev["track_clear"][0, 0] == 1.625 and dev["score"][0, 0] == 1.625
    x = pc.STRAIGHT.copy()
    x[2, 2] = np.inf
    dev, _ = both(host, pc.one_plan(np.array([(8.0, 3.0, 0.0)]), times, x, 1.5), label="one knot")
    assert np.isfinite(dev["track_clear"][0, 0])
    x[0, :] = np.nan
    dev, _ = both(host, pc.one_plan(np.array([(8.0, 3.0, 0.0)]), times, x, 1.5, x0=(np.nan, 0.0, 0.0)), label="every knot")
    assert np.isnan(dev["track_clear"][0, 0]) and np.isnan(dev["track_min"][0]) and dev["score"][0, 0] == 50.0
    c = pc.fill_world(pc.Case(1, 2, 5, 2, 1, 2, K=2), np.random.default_rng(3), mixed=False)
    c["track_len"][...] = 1
    c["track_x"][0, 1, 0] = (1.7e308, 1.7e308, np.pi / 4)
    old = c["score"].copy()
    dev, _ = both(host, c, label="overflow")
    assert np.all(np.isnan(dev["track_clear"])) and core.same_words(dev["score"], old)
    c = pc.one_plan(np.array([(-1.7e308, 0.0, 0.0), (1.7e308, 0.0, 0.0)]), np.array([0.0, 8.0]), pc.STRAIGHT, 1.5)
    dev, _ = both(host, c, label="overflowing difference")
    assert np.isnan(dev["track_clear"][0, 0]) and dev["track_state"][0, 0] == 1
    case = pc.fill_world(pc.Case(6, 3, 5, 4, 2, 4, K=7), np.random.default_rng(41), mixed=False)
    case["variant"][1], case["status"][2], case["status"][3] = 0, 2, 1
    case["score"][:, 4:] = np.array([-50.0, 50.0, np.nan])
    old = case["score"].copy()
    dev, _ = both(host, case, label="score")
    on = np.array([True, False, False, True, True, True])
    assert core.same_words(dev["score"][:, :4], old[:, :4]) and core.same_words(dev["score"][~on], old[~on])
    assert np.all(dev["score"][on, 4] == -50.0) and core.same_words(dev["score"][on, 5:], dev["track_clear"][on, 1:])
    rng = np.random.default_rng(17)
    case = pc.fill_world(pc.Case(5, 3, 7, 6, 1, 5), rng, mixed=False)
    case["dt"][...], case["t0"][...] = rng.uniform(0.2, 0.7, 5), rng.uniform(-1.0, 1.0, 5)
    case["track_t"][...] = np.cumsum(rng.uniform(0.1, 0.9, case["track_t"].shape), axis=2) - 1.0
    _, d = both(host, case, label="not dyadic")
    print("not dyadic: largest |device - host| %.3e" % d)
    dev, _ = both(host, pc.between_knots_case(), label="between the knots")
    assert dev["track_clear"][0, 0] == -1.5


def test_refused_calls_launch_nothing():
    rng = np.random.default_rng(73)
    c = pc.fill_world(pc.Case(4, 2, 3, 3, 2, 2, K=4), rng)
    for over in pc.REFUSED:
        device_call(c, rc=pc.E_INVAL, **over)
    for name in pc.READ + pc.WRITTEN:
        if name not in pc.OPTIONAL:
            device_call(c, rc=pc.E_INVAL, null=(name,))
    device_call(c, rc=pc.E_INVAL, device=-1)
    assert _lib.load().obca_plan_tracks(None, 0, None) == pc.E_INVAL
    check_struct_mirror(None, _lib.load().obca_plan_tracks_init, _lib.ObcaPlanTracks)


def test_a_side_stream_and_a_null_t0_give_the_same_words():
    rng = np.random.default_rng(79)
    c = pc.fill_world(pc.Case(6, 16, 9, 7, 3, 5), rng)
    ref = device_call(c)
    side = torch.cuda.Stream()
    got = device_call(c, stream=side)
    for name in pc.WRITTEN:
        assert core.same_words(got[name], ref[name]), name
    c["t0"][...] = 0.0
    ref = device_call(c)
    got = device_call(c, null=("t0",))
    for name in pc.WRITTEN:
        assert core.same_words(got[name], ref[name]), name


# ------------------------------------------------------------------------------------------------ 2. the wrapper
def test_the_wrapper_shows_the_track_between_the_stage_times():
    """``scene.track_rows`` and the staged ``scene.select`` score the track of the CPU tier's contrast 4.5 m away; through
    ``scene.plan_track_clearance`` with that state the slot's running minimum becomes the track's own -1.5 m"""
    c = pc.between_knots_case()
    tracks, track_t, track_len = c["track_x"].copy(), c["track_t"].copy(), c["track_len"].copy()
    rows = scene.track_rows(tracks, track_t, track_len, 1.5, 5)
    x = torch.as_tensor(pc.STRAIGHT[None], device="cuda")
    s = scene.select(rows["pool_A"], rows["pool_b"], x, 1, pool_v=rows["pool_v"], Ts=1.5, variant=8, n_sub=16, stage_A=rows["stage_A"],
                     stage_b=rows["stage_b"], stage_ok=rows["stage_ok"])
    assert rows["Ks"] == 0 and _np(rows["track_state"]).tolist() == [[1]] and _np(s["score"]).tolist() == [[4.5]]
    out = scene.plan_track_clearance(x, tracks, track_t, track_len, 1.5, score=s["score"], variant=8, status=s["ok"] * 0)
    assert _np(out["track_clear"]).tolist() == [[-1.5]] and _np(out["track_min"]).tolist() == [-1.5] and _np(s["score"]).tolist() == [[-1.5]]
    assert _np(out["track_state"]).tolist() == [[1]]
    bad_t = track_t.copy()
    bad_t[0, 0, 2] = bad_t[0, 0, 1]
    with pytest.raises(ValueError):
        scene.plan_track_clearance(x, tracks, bad_t, track_len, 1.5)
    out = scene.plan_track_clearance(x, tracks, torch.as_tensor(bad_t, device="cuda"), track_len, 1.5)      # at its word
    assert _np(out["track_state"]).tolist() == [[-1]] and _np(out["track_min"]).tolist() == [np.inf]
    with pytest.raises(ValueError):
        scene.plan_track_clearance(x, tracks, track_t, track_len, 1.5, group=2)
    with pytest.raises(ValueError):
        scene.plan_track_clearance(x, tracks, track_t, track_len, 1.5, score=torch.zeros(1, 1, device="cuda"))      # float32


def test_the_wrapper_and_the_c_call_agree():
    rng = np.random.default_rng(83)
    c = pc.fill_world(pc.Case(6, 4, 9, 7, 3, 5, K=6), rng)
    dev = device_call(c)
    score = torch.as_tensor(c["score"].copy(), device="cuda")
    out = scene.plan_track_clearance(c["x"], torch.as_tensor(c["track_x"], device="cuda"), c["track_t"], c["track_len"], c["dt"],
                                     track_size=c["track_size"], t0=c["t0"], x0=c["x0"], variant=c["variant"], status=c["status"],
                                     group=3, n_sub=5, score=score, ego=c.ego)
    for name in ("track_clear", "track_min", "track_state"):
        assert core.same_words(_np(out[name]), dev[name]), name
    assert core.same_words(_np(score), dev["score"])


# ------------------------------------------------------------------------------------------------ 3. solve_tracks
STANDING = np.array([(9.0, 4.5, 0.0), (12.5, 0.5, 0.0)])                 # heading 0, dyadic: ref_car_rows gives the device's words


def standing_poses(B):
    """[B,2,3]: the two standing cars of world g, moved with it"""
    return STANDING[None] + np.arange(B)[:, None, None] * np.array(sth.SHIFT + (0.0,))[None, None]


def standing_world(B=3):
    """the overtake world's three boxes and start / goal, its oncoming car replaced by two cars that stand -- one in the
    oncoming lane beside the block, one beyond the goal: one of one knot, one of three equal knots"""
    w = sth.overtake_world(B)
    tracks = np.zeros((B, 2, 3, 3))
    poses = standing_poses(B)
    tracks[:, 0, 0], tracks[:, 1, :] = poses[:, 0], poses[:, 1, None]
    track_t = np.tile(np.array([0.0, 3.0, 4.5]), (B, 2, 1))
    track_len = np.tile(np.array([1, 3], np.int32), (B, 1))
    return w, tracks, track_t, track_len


@pytest.mark.parametrize("rounds", (0, 2))
def test_standing_tracks_are_solve_scenes_words(rounds):
    """two tracks that stand, margin 0: ``solve_tracks`` equals ``solve_scene`` on a pool whose two extra static slots hold
    ``ref_car_rows`` of those poses -- plans, status, sel and rounds_used word for word, min_clear within 1e-12 -- and with
    rounds = 0 both are ``solver.solve`` on the staged selection's rows"""
    w, tracks, track_t, track_len = standing_world()
    B = len(w["x0"])
    solver = BatchSolver(sth.N, [4] * sth.N_SEL, B)
    args = (8, w["x0"], np.zeros((B, 2)), w["xref"])
    params = sth.device_params()
    r, info = scene.solve_tracks(solver, *args, w["pool_A"], w["pool_b"], sth.TS, tracks, track_t, track_len, rounds=rounds, params=params)
    got = {k: _np(getattr(r, k)) for k in ("xopt", "uopt", "ts_opt", "status", "iters")}
    got.update({k: _np(v) for k, v in info.items()})
    rows = [[core.ref_car_rows(p, core.EGO, 0.0) for p in ps] for ps in standing_poses(B)]
    pool_A = np.concatenate([w["pool_A"], np.array([[q[0] for q in rw] for rw in rows])], axis=1)
    pool_b = np.concatenate([w["pool_b"], np.array([[q[1] for q in rw] for rw in rows])], axis=1)
    r2, info2 = scene.solve_scene(solver, *args, pool_A, pool_b, sth.TS, pool_v=np.zeros((B, pool_b.shape[1], 2)), rounds=rounds,
                                  params=params)
    for k in ("xopt", "uopt", "ts_opt", "status", "iters"):
        assert core.same_words(got[k], _np(getattr(r2, k))), k
    for k in ("sel", "rounds_used", "A_used", "b_used", "clear"):
        assert core.same_words(got[k], _np(info2[k])), k
    for k in ("min_clear", "min_clear_first"):
        assert np.max(np.abs(got[k] - _np(info2[k]))) <= 1e-12, k
    print("standing tracks, rounds %d: sel %s rounds_used %s min_clear %s status %s" %
          (rounds, got["sel"].tolist(), got["rounds_used"].tolist(), got["min_clear"].tolist(), got["status"].tolist()))
    assert np.all(got["track_state"] == 1) and np.all(np.isin(got["status"], (0, 1)))
    assert np.all(got["track_min_clear"] >= got["min_clear"]) and core.same_words(got["track_clear"].min(axis=1), got["track_min_clear"])
    if rounds == 0:
        rows = scene.track_rows(tracks, track_t, track_len, sth.TS, sth.N, w["pool_A"], w["pool_b"])
        s = scene.select(rows["pool_A"], rows["pool_b"], torch.as_tensor(w["xref"], device="cuda"), sth.N_SEL, pool_v=rows["pool_v"],
                         Ts=sth.TS, x0=torch.as_tensor(w["x0"], device="cuda"), variant=8, n_sub=16, stage_A=rows["stage_A"],
                         stage_b=rows["stage_b"], stage_ok=rows["stage_ok"])
        r3 = solver.solve(8, w["x0"], np.zeros((B, 2)), w["xref"], s["A"], s["b"], np.full(B, sth.TS), None, params)
        for k in ("xopt", "uopt", "ts_opt", "status", "iters"):
            assert core.same_words(got[k], _np(getattr(r3, k))), k
        assert np.all(got["rounds_used"] == 0)
    solver.close()


def test_the_overtake_world_against_the_host_yardstick():
    """tests/test_solve_tracks_host.py's overtake with oncoming traffic, G = 2 (the second world shifted): every solve of the
    device's loop is within 1e-9 of the host yardstick's solve re-seeded from the device's inputs, and the loop shows the
    yardstick's contrast -- round 0 selects the three boxes and its plan is hit by the oncoming car, with rounds = 2 the tracked
    slot is selected and the held plan is clear"""
    hosts = sth.load_hosts()
    w, tracks, track_t, track_len = sth.overtake_case(G=2)
    B = len(w["x0"])
    solver = BatchSolver(sth.N, [4] * sth.N_SEL, B)
    seen = []
    solve = solver.solve

    def spy(variant, x0, u0, xref, A, b, Ts, *a, **kw):
        r = solve(variant, x0, u0, xref, A, b, Ts, *a, **kw)
        torch.cuda.synchronize()
        seen.append((_np(variant).copy(), _np(A).copy(), _np(b).copy(), {k: _np(getattr(r, k)).copy() for k in ("xopt", "uopt", "ts_opt", "status")}))
        return r
    solver.solve = spy
    r, info = scene.solve_tracks(solver, 8, w["x0"], np.zeros((B, 2)), w["xref"], w["pool_A"], w["pool_b"], sth.TS, tracks, track_t,
                                 track_len, rounds=2, params=sth.device_params())
    solver.solve = solve
    info = {k: _np(v) for k, v in info.items()}
    worst = 0.0
    for var, A, b, out in seen:
        on = var != 0
        if not on.any():
            continue
        o = sth.host_solve(w, on, A, b)
        assert np.array_equal(out["status"][on], o["status"]), (out["status"], o["status"])
        for k in ("xopt", "uopt", "ts_opt"):
            worst = max(worst, float(np.max(np.abs(out[k][on] - o[k]))))
    print("overtake G = 2: %d solves, largest |device - host| of a single solve %.3e (bound %.0e); min_clear_first %s min_clear %s sel %s"
          % (len(seen), worst, TOL, info["min_clear_first"].tolist(), info["min_clear"].tolist(), info["sel"].tolist()))
    assert worst < TOL
    h = sth.host_solve_tracks(hosts, w, tracks, track_t, track_len, rounds=2)
    assert np.array_equal(info["sel"], h["sel"]) and np.array_equal(info["rounds_used"], h["rounds_used"])
    assert np.max(np.abs(info["min_clear"] - h["min_clear"])) < 1e-6 and np.max(np.abs(info["min_clear_first"] - h["min_clear_first"])) < 1e-6
    sth.check_contrast(info)
    solver.close()


def test_solve_tracks_refuses_what_it_cannot_do():
    w, tracks, track_t, track_len = standing_world(2)
    solver = BatchSolver(sth.N, [4] * sth.N_SEL, 2)
    args = (w["x0"], np.zeros((2, 2)), w["xref"], w["pool_A"], w["pool_b"], sth.TS)
    with pytest.raises(ValueError):
        scene.solve_tracks(solver, 4, *args, tracks, track_t, track_len)
    with pytest.raises(ValueError):
        scene.solve_tracks(solver, np.array([8, 4]), *args, tracks, track_t, track_len)
    with pytest.raises(ValueError):
        scene.solve_tracks(solver, 8, *args, tracks, track_t, track_len, group=2)
    bad_t = track_t.copy()
    bad_t[1, 1, 2] = bad_t[1, 1, 1]
    with pytest.raises(ValueError):
        scene.solve_tracks(solver, 8, *args, tracks, bad_t, track_len)
    solver.close()
