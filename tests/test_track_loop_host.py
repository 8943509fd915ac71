"""The closed loop over scene pools with obstacles on timed tracks, on the host builds alone -- host select, plain
(tests/test_scene_core.py) or staged (tests/test_staged_select_core.py), host solver (native_build.lpi_solve, variant 8), host
pool-loop advance (tests/test_pool_loop_core.py) and the host core of obca_pool_tracks (tests/test_pool_tracks_core.py) -- as
the yardstick of tests/test_gpu_pool_tracks.py, and the recipe behind its scenario.

The world is tests/test_fleet_plan_loop_host.py's cut-in world with car 0 replaced by a TRACKED obstacle: the only rollout is
car 1 (14 route points along +x at y = 3.5 from x1), the track's knots are the trajectory car 0 drives in
``fl.host_fleet_loop(..., cut_in_world(x1), 2, see="lower", margin=0.1)``, one knot per step at times i * 1.5 s.  Under "lower"
car 0 sees nobody, so its trajectory does not depend on car 1.  N = 5, n_sel = 3, Ts = 1.5, 16 steps, margin 0.1, a
car-sized obstacle.  A synthetic track (car 0's route at a constant 0.4 m/s) does not separate the two predictions; the
driven trajectory does."""
import functools

import numpy as np
import pytest

from tests import native_build
from tests import test_fleet_core as core
from tests import test_fleet_loop_host as fl
from tests import test_fleet_plan_loop_host as fpl
from tests import test_pool_loop_core as plc
from tests import test_pool_tracks_core as ptc
from tests import test_scene_core as tsc
from tests import test_staged_select_core as ssc

N, S, TS, N_SEL, KS = fl.N, fl.S, fl.TS, fl.N_SEL, fl.KS
RUN, GOAL, CAP, FAILED, COLLISION = core.RUN, core.GOAL, core.CAP, core.FAILED, core.COLLISION
MARGIN = fl.MARGIN
X1 = fpl.X1
PREDICT = {"track": ptc.TRACK, "velocity": ptc.VELOCITY, "static": ptc.STATIC}


def load_hosts():
    """(pool-loop advance, staged select, plain select, pool tracks)"""
    return plc.load_host(), ssc.load_host(), tsc.load_host(), ptc.load_host()


@pytest.fixture(scope="module")
def hosts():
    return load_hosts()


def car_of(w, V, a):
    """the rollouts of car a of every world of a fleet world ``w`` as a world of their own"""
    return {k: v[a::V].copy() for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def cut_in_tracks(x1=X1, G=1):
    """(world of car 1 alone [G rollouts], tracks [G,1,S+1,3], track_t [G,1,S+1], track_len [G,1]): the knots are what car 0
    of world g drives in the host fleet loop under see="lower", one per step; beyond its last knot the track is padded with 0"""
    w = fpl.cut_in_world(x1, G=G)
    c, f, ok = fl.host_fleet_loop(plc.load_host(), tsc.load_host(), core.load_host(), w, 2, see="lower", margin=MARGIN)
    tracks, track_t, track_len = np.zeros((G, 1, S + 1, 3)), np.zeros((G, 1, S + 1)), np.zeros((G, 1), np.int32)
    for g in range(G):
        n = int(c["k"][2 * g]) + 1
        assert ok[2 * g] and c["flags"][2 * g] == GOAL
        tracks[g, 0, :n], track_len[g, 0] = c["x_closed"][2 * g, :n], n
        track_t[g, 0] = TS * np.arange(S + 1)
    return car_of(w, 2, 1), tracks, track_t, track_len


def host_cases(w, tracks, track_t, track_len, predict, margin=MARGIN, track_size=None, group=1, track_n_sub=8, clearance=ptc.NEVER,
               far=100.0):
    """(pool-loop case, pool-tracks case) over ONE set of buffers: the static pool with Kt spare slots appended"""
    B, P = len(w["start"]), w["path"].shape[2]
    Kt, L = tracks.shape[1], tracks.shape[2]
    c = plc.Case(B, KS + Kt, 4, N, N_SEL, P, S, moving=True, variant=8, n_sub=8, goal_tol2=fl.GOAL_TOL2)
    sA, sb = core.ref_spare_rows(far)
    c["pool_A"][:, :KS], c["pool_b"][:, :KS] = w["pool_A"], w["pool_b"]
    c["pool_A"][:, KS:], c["pool_b"][:, KS:] = sA, sb
    c["pool_v"][...] = 0.0
    for k in ("goal", "path", "path_len"):
        c[k][...] = w[k]
    c["x0"][...] = w["start"]
    t = ptc.Case(B, Kt, N, L, group, K=KS + Kt, S=S, n_sub=track_n_sub, predict=PREDICT[predict], clearance=clearance, margin=margin,
                 far=far)
    for k in ("x0", "k", "flags", "pool_A", "pool_b", "pool_v", "xref_out", "variant_out"):
        t.a[k] = c.a[k]
    t["track_x"][...], t["track_t"][...], t["track_len"][...] = tracks, track_t, track_len
    t["track_size"][...] = core.EGO if track_size is None else track_size
    t["Ts"][...], t["t0"][...] = TS, 0.0
    t["track_clear_hist"][...] = np.inf
    t["stage_A"][...], t["stage_b"][...], t["stage_ok"][...], t["track_state"][...] = 0.0, 0.0, 0, 0
    return c, t


def host_step(hosts, c, t, Ts):
    """one step's select and solve on the host builds, for the rollouts whose variant is not 0: the staged select on the
    track's stage rows (under "velocity" and "static" every mask word is 0 and it is the plain select's words)"""
    B = c.dims["B"]
    x0, u0, xref, variant = c["x0"].copy(), c["u0"].copy(), c["xref_out"].copy(), c["variant_out"].copy()
    s = ssc.host_select_staged(hosts[1], c["pool_A"], c["pool_b"], xref, N_SEL, stage_A=t["stage_A"], stage_b=t["stage_b"],
                               stage_ok=t["stage_ok"], stage_group=1, pool_v=c["pool_v"], Ts=Ts, x0=x0, variant=variant, n_sub=1)
    o = dict(xopt=np.zeros((B, 3, N + 1)), uopt=np.zeros((B, 2, N)), ts_opt=np.zeros(B), status=np.full(B, -5, np.int32),
             iters=np.zeros(B, np.int32))
    on = (variant != 0) & (s["ok"] == 1)
    if on.any():
        r = native_build.lpi_solve(8, N, [4] * N_SEL, x0[on], u0[on], xref[on], s["A"][on], s["b"][on], Ts[on])
        for k in o:
            o[k][on] = r[k]
    return s, o, on


def host_track_loop(hosts, w, tracks, track_t, track_len, predict, steps=S, **kw):
    """TrackLoop's recipe on the host builds; returns (pool-loop case, pool-tracks case, feasible_everywhere [B])"""
    c, t = host_cases(w, tracks, track_t, track_len, predict, **kw)
    B = c.dims["B"]
    Ts = np.full(B, TS)
    plc.advance(hosts[0], c, 0)
    t["x_prev"][...] = c["x0"]
    ptc.call_host(hosts[3], t, 0)
    ok = np.ones(B, bool)
    for step in range(steps):
        t["x_prev"][...] = c["x0"]
        s, o, on = host_step(hosts, c, t, Ts)
        ok &= ~on | np.isin(o["status"], (0, 1))
        for k in ("xopt", "uopt", "ts_opt", "status", "iters"):
            c[k][...] = o[k]
        c["sel"][...] = s["sel"]
        plc.advance(hosts[0], c, 1)
        t.dims["step"] = step
        ptc.call_host(hosts[3], t, 1)
    return c, t, ok


def report(tag, c, t, ok):
    print("%s: flags %s steps %s feasible %s track_min_clear %s" % (tag, c["flags"].tolist(), c["k"].tolist(), ok.tolist(),
                                                                   np.round(t["track_clear_hist"].min(axis=1), 3).tolist()))


# ---- what the host loop shows
def test_cut_in_velocity_fails_and_track_does_not(hosts):
    """x1 = 2.0.  The pool slot with its chord velocity and the plain select: a solve goes infeasible and the car ends FAILED.
    The track's rows per stage and the staged select: every solve feasible, no FAILED, and no interval the car drove comes
    nearer than 0 m to the obstacle as the track really moved."""
    w, tracks, track_t, track_len = cut_in_tracks(X1)
    c, t, ok = host_track_loop(hosts, w, tracks, track_t, track_len, "velocity")
    report("cut-in x1 %.2f velocity" % X1, c, t, ok)
    assert c["flags"][0] == FAILED and not ok[0]
    c, t, ok = host_track_loop(hosts, w, tracks, track_t, track_len, "track")
    report("cut-in x1 %.2f track" % X1, c, t, ok)
    assert ok.all() and c["flags"][0] != FAILED
    h = t["track_clear_hist"]
    assert np.all(h >= 0.0) and np.isfinite(h.min()) and np.all(t["track_state"] == 1) and np.all(t["stage_ok"] == 1)


def test_the_other_starts_are_printed(hosts):
    """measured, not asserted: the other three starts of car 1"""
    for x1 in (0.5, 1.5, 2.25):
        w, tracks, track_t, track_len = cut_in_tracks(x1)
        for predict in ("velocity", "track"):
            c, t, ok = host_track_loop(hosts, w, tracks, track_t, track_len, predict)
            report("cut-in x1 %.2f %s" % (x1, predict), c, t, ok)


@pytest.mark.parametrize("predict", ("track", "velocity"))
def test_a_parked_one_knot_track(hosts, predict):
    """a one-knot track at fl.PARKED_POSE on fl.parked_world: the obstacle stands, both predictions are the same rows, and the
    car passes it as ``FleetLoop``'s car 1 passes the parked car 0: GOAL in 14 steps, never nearer than 0.1 m"""
    w = car_of(fl.parked_world(1), 2, 1)
    tracks, track_t, track_len = np.array(fl.PARKED_POSE).reshape(1, 1, 1, 3), np.zeros((1, 1, 1)), np.ones((1, 1), np.int32)
    c, t, ok = host_track_loop(hosts, w, tracks, track_t, track_len, predict)
    report("parked " + predict, c, t, ok)
    assert ok.all() and c["flags"][0] == GOAL and c["k"][0] == 14
    assert t["track_clear_hist"].min() > 0.1 and np.all(c["pool_v"][:, KS:] == 0.0)
