"""The fleet closed loop with prediction by plans on the host builds alone -- tests/test_fleet_loop_host.py's loop with the
staged host select (tests/test_staged_select_core.py) in place of the plain one and the host tracks
(tests/test_fleet_tracks_core.py) after every fleet step -- as the yardstick of tests/test_gpu_fleet_plan.py, and the recipe
behind its scenario.

The cut-in world, in test_fleet_loop_host's corridor (N = 5, Ts = 1.5, n_sel = 3, 16 steps, margin 0.1, see="lower"): car 0
has priority; it drives 4 route points along +x at y = 6.5 from x = 3.0, then its route turns to heading -pi/4 for 7 more points
at 0.6 m spacing, across the lane of car 1, which drives 14 points along +x at y = 3.5 from x = X1.  The velocity prediction
shows car 1 the turn only once car 0's heading has changed; car 0's plan shows it five stages earlier."""
import numpy as np
import pytest

from tests import native_build
from tests import test_fleet_core as core
from tests import test_fleet_loop_host as fl
from tests import test_fleet_tracks_core as ftc
from tests import test_pool_loop_core as plc
from tests import test_staged_select_core as ssc
from tests import test_scene_core as tsc

N, S, TS, N_SEL, KS = fl.N, fl.S, fl.TS, fl.N_SEL, fl.KS
RUN, GOAL, CAP, FAILED, COLLISION = core.RUN, core.GOAL, core.CAP, core.FAILED, core.COLLISION
MARGIN = fl.MARGIN
X1 = 2.0                                   # the issue's table: 0.5, 1.5, 2.0, 2.25
CUT_STRAIGHT, CUT_TURNED, PATH_MAX = 4, 7, 14


def cut_in_route(x_first=3.0, y=6.5, straight=CUT_STRAIGHT, turned=CUT_TURNED, heading=-np.pi / 4, P=PATH_MAX):
    """[3,P]: ``straight`` points along +x at heading 0, then ``turned`` more at ``heading``, fl.SPACING apart, padded with the
    last point; path_len = straight + turned"""
    pts = [(x_first + fl.SPACING * i, y, 0.0) for i in range(straight)]
    for i in range(1, turned + 1):
        pts.append((pts[straight - 1][0] + fl.SPACING * i * np.cos(heading), y + fl.SPACING * i * np.sin(heading), heading))
    pts += [pts[-1]] * (P - len(pts))
    return np.array(pts).T


def cut_in_world(x1=X1, G=1, **route):
    plen = route.get("straight", CUT_STRAIGHT) + route.get("turned", CUT_TURNED)
    return fl.fleet_world([(cut_in_route(**route), plen), (fl.straight_route(x1, 3.5, PATH_MAX, P=PATH_MAX), PATH_MAX)], G=G, P=PATH_MAX)


def swap_world(G=1):
    """two cars on the line y = 5 whose routes make them swap places, starts 9 m apart"""
    return fl.fleet_world([(fl.straight_route(3.0, 5.0, fl.ROUTE_POINTS, P=PATH_MAX), fl.ROUTE_POINTS),
                           (fl.straight_route(12.0, 5.0, fl.ROUTE_POINTS, direction=-1.0, P=PATH_MAX), fl.ROUTE_POINTS)], G=G, P=PATH_MAX)


# ---- the host loop
def tracks_case(c, f, V):
    """the tracks descriptor over the loop's own buffers: x0, flags and k are the pool loop's, xopt and status its last solve"""
    B = c.dims["B"]
    t = ftc.Case(B // V, V, N, see=f.dims["see"], margin=f.margin, far=f.far)
    for k in ("x0", "flags", "k", "xopt", "status"):
        t.a[k] = c.a[k]
    t["track_A"][...], t["track_b"][...], t["track_ok"][...] = 0.0, 0.0, 0
    return t


def host_step_plan(staged_host, c, t, Ts, V):
    """fl.host_step with the staged select: one step's select and solve for the rollouts whose variant is not 0"""
    B = c.dims["B"]
    x0, u0, xref, variant = c["x0"].copy(), c["u0"].copy(), c["xref_out"].copy(), c["variant_out"].copy()
    s = ssc.host_select_staged(staged_host, c["pool_A"], c["pool_b"], xref, N_SEL, stage_A=t["track_A"].reshape(B // V, V, N + 1, 4, 2),
                               stage_b=t["track_b"].reshape(B // V, V, N + 1, 4), stage_ok=t["track_ok"], stage_group=V,
                               pool_v=c["pool_v"], Ts=Ts, x0=x0, variant=variant, n_sub=1)
    o = dict(xopt=np.zeros((B, 3, N + 1)), uopt=np.zeros((B, 2, N)), ts_opt=np.zeros(B), status=np.full(B, -5, np.int32),
             iters=np.zeros(B, np.int32))
    on = (variant != 0) & (s["ok"] == 1)
    if on.any():
        r = native_build.lpi_solve(8, N, [4] * N_SEL, x0[on], u0[on], xref[on], s["A"][on], s["b"][on], Ts[on])
        for k in o:
            o[k][on] = r[k]
    return s, o, on


def host_plan_loop(hosts, w, V, steps=S, **kw):
    """the whole loop on the host builds under predict="plan"; returns (pool-loop case, fleet case, tracks case,
    feasible_everywhere [B])"""
    pl_host, staged_host, fleet_host, tracks_host = hosts
    c, f = fl.host_cases(w, V, predict="velocity", **kw)
    t = tracks_case(c, f, V)
    B = c.dims["B"]
    Ts = np.full(B, TS)
    plc.advance(pl_host, c, 0)
    f["x_prev"][...] = c["x0"]
    core.step_host(fleet_host, f, 0)
    ok = np.ones(B, bool)
    for step in range(steps):
        f["x_prev"][...] = c["x0"]
        s, o, on = host_step_plan(staged_host, c, t, Ts, V)
        ok &= ~on | np.isin(o["status"], (0, 1))
        for k in ("xopt", "uopt", "ts_opt", "status", "iters"):
            c[k][...] = o[k]
        c["sel"][...] = s["sel"]
        plc.advance(pl_host, c, 1)
        f.dims["step"] = step
        core.step_host(fleet_host, f, 1)
        t.dims["step"] = step
        ftc.tracks_host(tracks_host, t)
    return c, f, t, ok


@pytest.fixture(scope="module")
def hosts():
    return plc.load_host(), ssc.load_host(), core.load_host(), ftc.load_host()


@pytest.fixture(scope="module")
def velocity_hosts():
    return plc.load_host(), tsc.load_host(), core.load_host()


def report(tag, c, f, ok):
    print("%s: flags %s steps %s feasible %s agent_min %s" % (tag, c["flags"].tolist(), c["k"].tolist(), ok.tolist(),
                                                            np.round(f["agent_clear_hist"].min(axis=1), 3).tolist()))


# ---- what the host loop shows
def test_cut_in_velocity_fails_and_plan_does_not(hosts, velocity_hosts):
    """see="lower": under the velocity prediction a solve of car 1 goes infeasible and car 1 ends FAILED; under the plan
    prediction every solve is feasible, car 0 reaches its goal, car 1 does not fail and no interval either car drove comes
    nearer than 0 m to the other"""
    w = cut_in_world()
    c, f, ok = fl.host_fleet_loop(*velocity_hosts, w, 2, see="lower", margin=MARGIN)
    report("cut-in x1 %.2f velocity" % X1, c, f, ok)
    assert c["flags"][1] == FAILED and not ok[1]
    c, f, t, ok = host_plan_loop(hosts, w, 2, see="lower", margin=MARGIN)
    report("cut-in x1 %.2f plan" % X1, c, f, ok)
    assert ok.all() and c["flags"][0] == GOAL and c["flags"][1] != FAILED
    h = f["agent_clear_hist"]
    assert np.all(h >= 0.0) and np.isfinite(h.min())
    assert np.all(t["track_ok"][0] == 0)                                       # car 0 yields to nobody


@pytest.mark.parametrize("see", ("lower", "all"))
def test_head_on_under_plans(hosts, see):
    """the head-on world of tests/test_fleet_loop_host.py under "plan": every solve feasible, both cars reach their goals and
    never touch (the host loop shows 12 / 14 steps and 0.94 m under "lower", 13 / 13 steps and 1.06 m under "all")"""
    c, f, t, ok = host_plan_loop(hosts, fl.head_on_world(1), 2, see=see, margin=MARGIN)
    report("head-on plan " + see, c, f, ok)
    assert ok.all() and list(c["flags"]) == [GOAL, GOAL] and f["agent_clear_hist"].min() >= 0.0


def test_what_plans_do_not_fix_is_printed(hosts, velocity_hosts):
    """measured, not asserted: the cut-in under see="all", where each car plans against a plan that is being
    revised against it, and two cars that must swap places on one line"""
    for tag, w, see in (("cut-in all", cut_in_world(), "all"), ("swap lower", swap_world(), "lower")):
        c, f, ok = fl.host_fleet_loop(*velocity_hosts, w, 2, see=see, margin=MARGIN)
        report(tag + " velocity", c, f, ok)
        c, f, t, ok = host_plan_loop(hosts, w, 2, see=see, margin=MARGIN)
        report(tag + " plan", c, f, ok)
