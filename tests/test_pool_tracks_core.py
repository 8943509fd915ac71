"""CPU tier of the obstacles on timed tracks (csrc/obca_pool_tracks_core.h: the serial definition of obca_pool_tracks), built
for the host from tests/native/pool_tracks_host.cpp.

Yardstick: ``ref_call``, a numpy restatement of the rules -- the state of a track, the pose at a time (numpy's searchsorted
and one rounding per operation), the stage times, ``test_fleet_core.ref_car_rows`` for the rows, the chord velocity, and for
the measurement tests/kkt_check.py's ``polytope_distance`` of ``car_corners`` against the margin-free rows at the track's pose
at every sample's time -- compared on every buffer of the call, each of which sits between guard bands.

Words and bounds.  Everything without sin or cos is compared WORD FOR WORD: flags, states, masks, spares, the static slots
(untouched), which history words are written, variant_out and xref_out, the chord velocities (differences and one quotient,
rounded alike by numpy and the core), and the rows of worlds at heading 0 (``exact``; their numbers are dyadic, so that a
stage time that falls on a knot's time is that word).  At general headings the rows are within tests/test_fleet_core.py's
A_TOL / ROW_TOL, derived there for coordinates below 100 m; the worlds here stay below 100 m.  Distances are within its
DIST_TOL = 1e-12 m (the same geometry evaluated in another order).  The helpers are shared with tests/test_gpu_pool_tracks.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import kkt_check, native_build, test_fleet_core as core
from tests.descriptor_case import DescriptorCase, check_struct_mirror
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "pool_tracks_host.cpp")
E_INVAL = core.E_INVAL
RUN, GOAL, CAP, FAILED, COLLISION = core.RUN, core.GOAL, core.CAP, core.FAILED, core.COLLISION
TRACK, VELOCITY, STATIC = 0, 1, 2
NEVER = core.NEVER
FILL_X, FILL_I = core.FILL_X, core.FILL_I
READ = ("track_x", "track_t", "track_len", "track_size", "t0", "Ts", "x_prev", "x0", "k")
WRITTEN = ("flags", "pool_A", "pool_b", "pool_v", "stage_A", "stage_b", "stage_ok", "track_state", "track_clear_hist", "xref_out",
           "variant_out")
INT = ("track_len", "k", "flags", "stage_ok", "track_state", "variant_out")
SHAPES = [(1, 1, 1, 1, 1), (5, 3, 5, 2, 1), (6, 16, 127, 7, 3), (2, 64, 5, 4, 2)]          # B, Kt, N, L, group
SHAPE_ID = lambda s: "B%d_Kt%d_N%d_L%d_g%d" % s


def load_host():
    lib = native_build.build_shim("pool_tracks_host", [SRC])
    lib.pool_tracks_host.restype = ctypes.c_int
    lib.pool_tracks_host.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.pool_tracks_layout_host.restype = ctypes.c_int
    lib.pool_tracks_pose_host.restype = None
    lib.pool_tracks_pose_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def fleet_host():
    return core.load_host()


def shapes(B, K, Kt, N, L, group, S):
    Bt = B // group
    return {"track_x": (Bt, Kt, L, 3), "track_t": (Bt, Kt, L), "track_len": (Bt, Kt), "track_size": (Bt, Kt, 4), "t0": (B,), "Ts": (B,),
            "x_prev": (B, 3), "x0": (B, 3), "k": (B,), "flags": (B,), "pool_A": (B, K, 4, 2), "pool_b": (B, K, 4), "pool_v": (B, K, 2),
            "stage_A": (B, Kt, N + 1, 4, 2), "stage_b": (B, Kt, N + 1, 4), "stage_ok": (B, Kt), "track_state": (B, Kt),
            "track_clear_hist": (B, S), "xref_out": (B, 3, N + 1), "variant_out": (B,)}


class Case(DescriptorCase):
    """the buffers of one obca_pool_tracks in host memory, every one between guard bands, and the scalars"""
    SCALARS = ("clearance", "margin", "far")

    def __init__(self, B, Kt, N=5, L=4, group=1, K=None, S=4, step=0, n_sub=4, predict=TRACK, clearance=NEVER, margin=0.0, far=100.0,
                 ego=core.EGO, exact=False):
        K = Kt + (2 if Kt < 63 else 0) if K is None else K
        self.dims = dict(B=B, K=K, Kt=Kt, N=N, L=L, group=group, max_steps=S, step=step, n_sub=n_sub, predict=predict)
        self.clearance, self.margin, self.far, self.ego, self.exact = clearance, margin, far, tuple(ego), exact
        super().__init__(_lib.ObcaPoolTracks, shapes(B, K, Kt, N, L, group, S), INT)


def call_host(host, case, measure, rc=0, null=(), **over):
    d = case.descriptor(null=null, **over)
    assert host.pool_tracks_host(ctypes.byref(d), measure) == rc


# ------------------------------------------------------------------------------------------------ the numpy restatement
def ref_state(x, t, ln, size, L, Ts, t0):
    if ln == 0:
        return 0
    ok = 1 <= ln <= L and bool(np.all(np.isfinite(size))) and np.isfinite(size[0] + size[2]) and np.isfinite(size[1] + size[3]) \
        and size[0] + size[2] > 0.0 and size[1] + size[3] > 0.0
    ok = ok and bool(np.all(np.isfinite(x[:ln])) and np.all(np.isfinite(t[:ln])) and np.all(np.diff(t[:ln]) > 0.0))
    ok = ok and bool(np.isfinite(Ts) and Ts > 0.0 and np.isfinite(t0))
    return 1 if ok else -1


def ref_pose(x, t, ln, when):
    """the pose at time ``when`` of a usable track: x [L,3], t [L]"""
    if ln == 1 or not when > t[0]:
        return x[0].copy()
    if when >= t[ln - 1]:
        return x[ln - 1].copy()
    i = int(np.searchsorted(t[:ln], when, side="right")) - 1
    if when == t[i]:
        return x[i].copy()
    a = (when - t[i]) / (t[i + 1] - t[i])
    return x[i] + a * (x[i + 1] - x[i])


def ref_time(t0, k, kk, Ts):
    return np.float64(t0) + np.float64(int(k) + kk) * np.float64(Ts)


def ref_sample_time(t_prev, t_now, n_sub, s):
    return t_prev if s == 0 else (t_now if s == n_sub else t_prev + (s / n_sub) * (t_now - t_prev))


def ref_call(case, measure):
    """what the call must leave in every written buffer, from the buffers as they are now (guard bands excluded)"""
    a = {k: v.copy() for k, v in case.a.items()}
    dm = case.dims
    B, K, Kt, N, L, group, S, step, n_sub = (dm[k] for k in ("B", "K", "Kt", "N", "L", "group", "max_steps", "step", "n_sub"))
    sA, sb = core.ref_spare_rows(case.far)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            bt = b // group
            Ts, t0, k = a["Ts"][b], a["t0"][b], a["k"][b]
            tr = [(a["track_x"][bt, j], a["track_t"][bt, j], int(a["track_len"][bt, j]), a["track_size"][bt, j]) for j in range(Kt)]
            state = [ref_state(x, t, ln, size, L, Ts, t0) for x, t, ln, size in tr]
            if measure and n_sub > 0 and k == step + 1:
                fold = np.inf
                xp, x0 = a["x_prev"][b], a["x0"][b]
                if np.all(np.isfinite(xp)) and np.all(np.isfinite(x0)):
                    t_prev, t_now = ref_time(t0, k, -1, Ts), ref_time(t0, k, 0, Ts)
                    for j, (x, t, ln, size) in enumerate(tr):
                        if state[j] != 1:
                            continue
                        for s in range(n_sub + 1):
                            p = xp if s == 0 else (x0 if s == n_sub else xp + (s / n_sub) * (x0 - xp))
                            A, bb = core.ref_car_rows(ref_pose(x, t, ln, ref_sample_time(t_prev, t_now, n_sub, s)), size, 0.0)
                            d = kkt_check.polytope_distance(kkt_check.car_corners(p, case.ego), A, bb) \
                                if np.all(np.isfinite(A)) and np.all(np.isfinite(bb)) else np.nan
                            fold = np.nan if (np.isnan(fold) or not np.isfinite(d)) else min(fold, d)
                if not np.isnan(fold):
                    a["track_clear_hist"][b, step] = fold
                was = a["flags"][b]
                now = FAILED if np.isnan(fold) else (COLLISION if (was == RUN and fold < case.clearance) else was)
                if now != was:
                    a["flags"][b], a["variant_out"][b] = now, 0
                    a["xref_out"][b] = np.where(np.isfinite(a["x0"][b]), a["x0"][b], 0.0)[:, None]
            for j, (x, t, ln, size) in enumerate(tr):
                s = K - Kt + j
                a["track_state"][b, j] = state[j]
                a["stage_ok"][b, j] = 1 if (state[j] == 1 and dm["predict"] == TRACK) else 0
                a["pool_v"][b, s] = 0.0
                if state[j] != 1:
                    a["pool_A"][b, s], a["pool_b"][b, s] = sA, sb
                    a["stage_A"][b, j], a["stage_b"][b, j] = sA, sb
                    continue
                poses = [ref_pose(x, t, ln, ref_time(t0, k, kk, Ts)) for kk in range(N + 1)]
                for kk, p in enumerate(poses):
                    a["stage_A"][b, j, kk], a["stage_b"][b, j, kk] = core.ref_car_rows(p, size, case.margin) \
                        if np.all(np.isfinite(p)) else (sA, sb)
                a["pool_A"][b, s], a["pool_b"][b, s] = a["stage_A"][b, j, 0], a["stage_b"][b, j, 0]
                if dm["predict"] != STATIC and np.all(np.isfinite(poses[0])):
                    v = (poses[1][:2] - poses[0][:2]) / Ts
                    a["pool_v"][b, s] = np.where(np.isfinite(v), v, 0.0)
    return a


def compare(case, got, want, dist_tol=core.DIST_TOL, label=""):
    """``got`` against ``want`` (``ref_call``'s dict, or another implementation's buffers): word for word except the rows of
    usable tracks of a world that is not ``exact`` (A_TOL, ROW_TOL) and the measured distances (dist_tol; which words are
    written is exact).  Returns the largest deviations (rows, distances)."""
    K, Kt = case.dims["K"], case.dims["Kt"]
    for name in ("flags", "variant_out", "xref_out", "stage_ok", "track_state"):
        assert core.same_words(got[name], want[name]), (label, name)
    h, hw = got["track_clear_hist"], want["track_clear_hist"]
    written = hw != FILL_X
    assert np.array_equal(h != FILL_X, written) and not np.isnan(h).any(), label
    assert np.array_equal(np.isinf(h), np.isinf(hw)), label
    fin = written & np.isfinite(hw)
    d_dev = float(np.max(np.abs(h[fin] - hw[fin]))) if fin.any() else 0.0
    assert d_dev <= dist_tol, (label, d_dev)
    car = want["track_state"] == 1
    r_dev = 0.0
    Ks = K - Kt
    assert core.same_words(got["pool_v"], want["pool_v"]), (label, "pool_v")
    for name, tol in (("pool_A", core.A_TOL), ("pool_b", core.ROW_TOL), ("stage_A", core.A_TOL), ("stage_b", core.ROW_TOL)):
        g, w = got[name], want[name]
        assert not np.isnan(g).any(), (label, name)
        if name.startswith("pool"):
            assert core.same_words(g[:, :Ks], w[:, :Ks]), (label, name, "static slots")
            g, w = g[:, Ks:], w[:, Ks:]
        assert core.same_words(g[~car], w[~car]), (label, name, "spares")
        if case.exact:
            assert core.same_words(g[car], w[car]), (label, name, "cars")
        elif car.any():
            with np.errstate(invalid="ignore"):
                dev = float(np.nanmax(np.abs(g[car] - w[car])))
            assert np.array_equal(np.isinf(g[car]), np.isinf(w[car])), (label, name)
            r_dev = max(r_dev, dev)
            assert dev <= tol, (label, name, dev)
    return r_dev, d_dev


def check_call(host, case, measure, label=""):
    """one call of the host core against ref_call; the read-only buffers and every guard band untouched"""
    want = ref_call(case, measure)
    before = {k: case.a[k].copy() for k in READ}
    call_host(host, case, measure)
    out = compare(case, case.a, want, label=label)
    for name in READ:
        assert core.same_words(case.a[name], before[name]), name
    assert case.bands_clean()
    return out


# ------------------------------------------------------------------------------------------------ worlds
def fill_world(case, rng, mixed=True):
    """tracks that drive and turn in a 40 m x 10 m corridor, dyadic knot times (steps of 0.25 .. 1 s from a start of -1 .. 1 s)
    and dyadic Ts, t0 and (``exact``: heading 0) coordinates, so that stage times fall before the first knot, exactly on knots,
    between knots and past the end; cars next to them.  ``mixed``: rollouts at different k, one that did not step, ended
    rollouts (GOAL, FAILED), a track of length 0, tracks of one knot, one unusable track"""
    dm = case.dims
    B, K, Kt, N, L, group, step = (dm[k] for k in ("B", "K", "Kt", "N", "L", "group", "step"))
    Bt = B // group
    q8 = lambda v: np.round(np.asarray(v) * 8.0) / 8.0
    for bt in range(Bt):
        for j in range(Kt):
            ln = int(rng.integers(1, L + 1))
            t = q8(rng.uniform(-1.0, 1.0)) + np.concatenate([[0.0], np.cumsum(rng.choice([0.25, 0.5, 1.0], L - 1))]) if L > 1 \
                else np.array([q8(rng.uniform(-1.0, 1.0))])
            p = np.array([rng.uniform(2.0, 30.0), rng.uniform(2.0, 8.0)])
            th = 0.0 if case.exact else rng.uniform(-np.pi, np.pi)
            for i in range(L):
                case["track_x"][bt, j, i] = (q8(p[0]), q8(p[1]), th) if case.exact else (p[0], p[1], th)
                th += 0.0 if case.exact else rng.uniform(-0.4, 0.4)
                p = p + rng.uniform(0.0, 1.0) * np.array([np.cos(th), np.sin(th)])
            case["track_t"][bt, j], case["track_len"][bt, j] = t, ln
            case["track_size"][bt, j] = core.EGO_OFF if (j % 2 or case.exact) else core.EGO
    case["Ts"][...] = rng.choice([0.25, 0.5, 1.0], B)
    case["t0"][...] = q8(rng.uniform(-2.0, 2.0, B))
    case["k"][...] = step + 1
    case["flags"][...] = RUN
    for b in range(B):
        x = np.array([rng.uniform(2.0, 30.0), rng.uniform(2.0, 8.0), 0.0 if case.exact else rng.uniform(-np.pi, np.pi)])
        x = q8(x) if case.exact else x
        case["x_prev"][b], case["x0"][b] = x, x + (0.5, 0.125, 0.0 if case.exact else 0.1)
    case["pool_A"][:, :K - Kt], case["pool_b"][:, :K - Kt], case["pool_v"][:, :K - Kt] = 0.5, 3.0, 0.25
    if mixed and B > 1:
        case["k"][1] = step                                             # did not step
        case["flags"][B - 1] = GOAL
        if B > 2:
            case["k"][2], case["flags"][2] = step + 3, FAILED           # another time, ended
            case["flags"][0] = CAP
        case["track_len"][0, 0] = 0
        if Kt > 1:
            case["track_len"][0, 1] = 1
        if Kt > 2:
            case["track_x"][0, 2, 0, 1] = np.nan
    return case


# ------------------------------------------------------------------------------------------------ tests
CONFIGS = [(TRACK, 1, 16), (VELOCITY, 1, 1), (STATIC, 1, 0), (TRACK, 0, 16), (VELOCITY, 0, 1)]      # predict, measure, n_sub


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
def test_the_core_matches_numpy(host, shape):
    """all three predictions, measure 0 / 1, n_sub 0 / 1 / 16, heading 0 (word for word) and turning tracks (within the derived
    bounds), on worlds with every kind of rollout and track"""
    B, Kt, N, L, group = shape
    rng = np.random.default_rng(sum(c * 11 ** i for i, c in enumerate(shape)))
    worst = [0.0, 0.0]
    for exact in (True, False):
        for predict, measure, n_sub in CONFIGS:
            case = fill_world(Case(B, Kt, N, L, group, step=2, n_sub=n_sub, predict=predict, margin=0.25, exact=exact), rng)
            r, d = check_call(host, case, measure, label=(shape, exact, predict, measure, n_sub))
            worst = [max(worst[0], r), max(worst[1], d)]
            st = case["track_state"]
            assert set(np.unique(st)) <= {-1, 0, 1} and np.array_equal(case["stage_ok"], ((st == 1) & (predict == TRACK)).astype(np.int32))
            if B > 1:
                assert np.all(st[:group, 0] == 0) and (Kt < 3 or np.all(st[:group, 2] == -1))
            if measure and n_sub > 0:
                h = case["track_clear_hist"]
                assert np.all(h[:, :2] == FILL_X) and np.all(h[:, 3:] == FILL_X)
                assert np.array_equal(h[:, 2] != FILL_X, case["k"] == 3)                # a car that did not step gets no word
            else:
                assert np.all(case["track_clear_hist"] == FILL_X)
    print("%s: largest |rows - numpy| %.3e (bound %.3e), |distance - numpy| %.3e (bound %.3e)" %
          (SHAPE_ID(shape), worst[0], core.ROW_TOL, worst[1], core.DIST_TOL))


def one_track(knots, times, size=core.EGO, **kw):
    """one rollout, one track"""
    L = len(times)
    c = Case(1, 1, L=L, K=1, **kw)
    c["track_x"][0, 0], c["track_t"][0, 0], c["track_len"][0, 0], c["track_size"][0, 0] = knots, times, L, size
    c["Ts"][...], c["t0"][...], c["k"][...], c["flags"][...] = 0.5, 0.0, 0, RUN
    c["x_prev"][...] = c["x0"][...] = (0.0, 50.0, 0.0)
    return c


KNOTS = np.array([(4.0, 3.0, 0.0), (5.0, 3.0, 0.5), (5.5, 4.0, 1.0), (5.5, 4.0, 1.0), (7.0, 6.0, -0.25)])
TIMES = np.array([1.0, 2.0, 2.5, 4.0, 4.5])


def test_times_before_on_between_and_past_the_knots(host, fleet_host):
    """Ts = 0.5 from t0 = 0.25 k = 0: stages at 0.25 .. (before the first knot), t0 = 0: stages fall ON the knots' times -- the
    rows are the knot's, word for word fleet_car_rows_host's -- t0 = 0.25: between them, stage 9 .. 12 at or past the end: the
    last knot.  The obstacle stands between knots 2 and 3 and its chord velocity is 0 there."""
    e = np.array(core.EGO)

    def rows(pose):
        A, b = np.zeros((4, 2)), np.zeros(4)
        fleet_host.fleet_car_rows_host(np.ascontiguousarray(pose, float).ctypes.data, e.ctypes.data, 0.125, A.ctypes.data, b.ctypes.data)
        return A, b
    for t0 in (0.0, 0.25, -8.0, 100.0):
        c = one_track(KNOTS, TIMES, N=12, margin=0.125)
        c["t0"][...] = t0
        check_call(host, c, 0)
        for kk in range(13):
            t = t0 + kk * 0.5
            on = np.nonzero(TIMES == t)[0]
            pose = KNOTS[0] if t <= 1.0 else (KNOTS[4] if t >= 4.5 else (KNOTS[on[0]] if len(on) else None))
            if pose is None:
                i = int(np.searchsorted(TIMES, t, side="right")) - 1
                pose = KNOTS[i] + ((t - TIMES[i]) / (TIMES[i + 1] - TIMES[i])) * (KNOTS[i + 1] - KNOTS[i])
                assert not len(on)
            A, b = rows(pose)
            assert core.same_words(c["stage_A"][0, 0, kk], A) and core.same_words(c["stage_b"][0, 0, kk], b), (t0, kk)
            p = np.zeros(3)
            host.pool_tracks_pose_host(KNOTS.ctypes.data, TIMES.ctypes.data, 5, t, p.ctypes.data)
            assert core.same_words(p, np.asarray(pose, float))
        assert tuple(c["pool_v"][0, 0]) == (0.0, 0.0)               # stage 0 -> 1 is before the first knot or past the last
    c = one_track(KNOTS, TIMES, N=2)
    c["t0"][...], c["k"][...] = 0.0, 3                                  # t = 1.5 -> 2.0: half of knot 0 -> 1, 1 m/s along x
    check_call(host, c, 0)
    assert tuple(c["pool_v"][0, 0]) == (1.0, 0.0)
    c["k"][...] = 6                                                     # t = 3.0 -> 3.5: parked between equal knots
    check_call(host, c, 0)
    assert tuple(c["pool_v"][0, 0]) == (0.0, 0.0) and core.same_words(c["stage_b"][0, 0, 0], c["stage_b"][0, 0, 1])
    for predict in (STATIC, VELOCITY):
        c = one_track(KNOTS, TIMES, N=2, predict=predict)
        c["k"][...] = 3
        check_call(host, c, 0)
        assert tuple(c["pool_v"][0, 0]) == ((0.0, 0.0) if predict == STATIC else (1.0, 0.0)) and c["stage_ok"][0, 0] == 0


def test_stage_kk_now_is_stage_kk_minus_one_a_step_later(host):
    """the time of a stage is one product and one sum of k + kk: the rows move down one stage per step, word for word, at any
    heading and for numbers that are not dyadic"""
    rng = np.random.default_rng(61)
    case = fill_world(Case(5, 3, 7, 6, 1, step=0, margin=0.1), rng, mixed=False)
    case["Ts"][...], case["t0"][...] = rng.uniform(0.2, 0.7, 5), rng.uniform(-1.0, 1.0, 5)
    case["k"][...] = np.arange(5)
    call_host(host, case, 0)
    A0, b0 = case["stage_A"].copy(), case["stage_b"].copy()
    assert not core.same_words(b0[:, :, 1:], b0[:, :, :-1])
    case["k"][...] += 1
    call_host(host, case, 0)
    assert core.same_words(case["stage_A"][:, :, :-1], A0[:, :, 1:]) and core.same_words(case["stage_b"][:, :, :-1], b0[:, :, 1:])
    Ks = case.dims["K"] - 3
    assert core.same_words(case["pool_b"][:, Ks:], b0[:, :, 1]) and core.same_words(case["pool_A"][:, Ks:], A0[:, :, 1])


def spoil(case, why):
    """one reason a track is unusable, on track 1 of block 0; returns the state the slot must get"""
    c = case
    if why == "len_0":
        c["track_len"][0, 1] = 0
        return 0
    if why == "len_negative":
        c["track_len"][0, 1] = -1
    elif why == "len_beyond_L":
        c["track_len"][0, 1] = case.dims["L"] + 1
    elif why == "nan_pose_word":
        c["track_x"][0, 1, 2, 2] = np.nan
    elif why == "inf_pose_word":
        c["track_x"][0, 1, 0, 0] = np.inf
    elif why == "nan_time":
        c["track_t"][0, 1, 1] = np.nan
    elif why == "inf_last_time":
        c["track_t"][0, 1, 3] = np.inf
    elif why == "equal_times":
        c["track_t"][0, 1, 2] = c["track_t"][0, 1, 1]
    elif why == "decreasing_times":
        c["track_t"][0, 1, 3] = c["track_t"][0, 1, 0] - 1.0
    elif why == "nan_size":
        c["track_size"][0, 1, 3] = np.nan
    elif why == "length_overflows":
        c["track_size"][0, 1] = (1.7e308, 0.5, 1.7e308, 0.5)
    elif why == "no_length":
        c["track_size"][0, 1] = (1.0, 0.5, -1.0, 0.5)
    elif why == "negative_width":
        c["track_size"][0, 1] = (1.0, 0.5, 1.0, -0.75)
    else:
        raise KeyError(why)
    return -1


REASONS = ["len_0", "len_negative", "len_beyond_L", "nan_pose_word", "inf_pose_word", "nan_time", "inf_last_time", "equal_times",
           "decreasing_times", "nan_size", "length_overflows", "no_length", "negative_width"]


def spoilt_case(why, rng, predict=TRACK):
    case = fill_world(Case(4, 3, 5, 4, 2, step=1, n_sub=4, predict=predict, margin=0.1), rng, mixed=False)
    case["track_len"][...] = 4
    if why in ("nan_ts", "zero_ts", "negative_ts", "inf_t0"):
        case["Ts" if why.endswith("ts") else "t0"][0] = {"nan_ts": np.nan, "zero_ts": 0.0, "negative_ts": -0.5, "inf_t0": np.inf}[why]
        return case, -1
    return case, spoil(case, why)


@pytest.mark.parametrize("why", REASONS + ["nan_ts", "zero_ts", "negative_ts", "inf_t0"])
def test_every_reason_a_track_is_unusable(host, why):
    """one reason at a time: the slot is a spare (state -1, or 0 for a length of 0), its mask word 0, its velocity 0, no word of
    the track reaches an output -- the track beyond the spoilt word is NaN -- and it is not measured; the other tracks of the
    block and the other block keep their rows.  A clock that is not usable (Ts, t0) spoils every track of that rollout alone."""
    rng = np.random.default_rng(67)
    case, state = spoilt_case(why, rng)
    clock = why in ("nan_ts", "zero_ts", "negative_ts", "inf_t0")
    check_call(host, case, 1, label=why)
    st = case["track_state"]
    if clock:
        assert np.all(st[0] == -1) and np.all(st[1:] == 1)
        assert case["track_clear_hist"][0, 1] == np.inf                      # stepped, nothing usable to measure
    else:
        assert np.all(st[:2, 1] == state) and np.all(st[2:] == 1) and np.all(st[:2, 0] == 1) and np.all(st[:2, 2] == 1)
    sA, sb = core.ref_spare_rows(100.0)
    b, j = 0, 1
    assert core.same_words(case["stage_b"][b, j], np.stack([sb] * 6)) and core.same_words(case["stage_A"][b, j], np.stack([sA] * 6))
    assert core.same_words(case["pool_b"][b, 2 + j], sb) and tuple(case["pool_v"][b, 2 + j]) == (0.0, 0.0) and case["stage_ok"][b, j] == 0
    for name in WRITTEN:
        assert not np.isnan(case[name].astype(float)).any(), name


def test_a_spoilt_track_is_not_measured(host):
    """the fold runs over usable slots only: with the nearest track spoilt the history word is the distance to the others"""
    rng = np.random.default_rng(71)
    case, _ = spoilt_case("nan_time", rng)
    case["track_x"][0, 1, :, :2] = case["x0"][0, :2]                   # on top of car 0 -- if it counted
    good = Case(4, 3, 5, 4, 2, step=1, n_sub=4, margin=0.1)
    for k in case.a:
        good.a[k][...] = case.a[k]
    good["track_len"][0, 1] = 0
    call_host(host, case, 1)
    call_host(host, good, 1)
    assert core.same_words(case["track_clear_hist"], good["track_clear_hist"]) and case["track_clear_hist"][0, 1] > 0.0


def test_a_distance_that_overflows_ends_the_car_failed(host):
    """a track out at 1.7e308 m, turned by pi / 4: its rows overflow to +inf, no distance to them is a number, the car ends
    FAILED without a history word and gets the masked window; a GOAL car too (obca_fleet_step's rule).  Nothing written is NaN."""
    for flag in (RUN, GOAL):
        c = one_track(np.array([(1.7e308, 1.7e308, np.pi / 4)]), np.array([0.0]), n_sub=2, step=1, S=3, N=3)
        c["k"][...], c["flags"][...] = 2, flag
        c["variant_out"][...], c["x0"][...] = 8, (1.0, 2.0, 0.5)
        check_call(host, c, 1, label="overflow")
        assert c["flags"][0] == FAILED and np.all(c["track_clear_hist"] == FILL_X) and c["variant_out"][0] == 0
        assert core.same_words(c["xref_out"][0], np.repeat(np.array([[1.0], [2.0], [0.5]]), 4, axis=1))
        assert np.isinf(c["pool_b"]).any() and not np.isnan(c["pool_b"]).any() and not np.isnan(c["stage_b"]).any()
    c = one_track(np.array([(-1.7e308, 0.0, 0.0), (1.7e308, 0.0, 0.0)]), np.array([0.0, 8.0]), N=3)        # the knots' difference overflows
    check_call(host, c, 0, label="overflowing difference")          # stage 0 is knot 0, stage 1 lies between the knots
    sA, sb = core.ref_spare_rows(100.0)
    assert c["track_state"][0, 0] == 1 and core.same_words(c["stage_b"][0, 0, 1], sb) and not core.same_words(c["stage_b"][0, 0, 0], sb)


def test_collision_stops_a_running_car_and_not_one_at_its_goal(host):
    """clearance 0.5 m, the car 0.25 m beside a parked obstacle: RUN becomes COLLISION with the masked window, GOAL stays GOAL
    and keeps its window; both get the history word.  A car without a pose is not measured (+inf)."""
    size = core.EGO_OFF
    for flag in (RUN, GOAL, CAP):
        c = one_track(np.array([(10.0, 5.0, 0.0)]), np.array([0.0]), size=size, n_sub=4, step=0, clearance=0.5, exact=True)
        c["k"][...], c["flags"][...], c["variant_out"][...] = 1, flag, 8
        c["xref_out"][...] = 3.5
        c["x_prev"][...], c["x0"][...] = (9.0, 5.625 + 0.75 + 0.25, 0.0), (9.5, 5.625 + 0.75 + 0.25, 0.0)
        check_call(host, c, 1, label=flag)
        assert c["track_clear_hist"][0, 0] == 0.25
        assert c["flags"][0] == (COLLISION if flag == RUN else flag)
        assert c["variant_out"][0] == (0 if flag == RUN else 8) and (c["xref_out"][0, 0, 0] == (9.5 if flag == RUN else 3.5))
    c["x_prev"][0, 1], c["flags"][...] = np.nan, RUN
    c["track_clear_hist"][...] = FILL_X
    check_call(host, c, 1)
    assert c["track_clear_hist"][0, 0] == np.inf and c["flags"][0] == RUN


def test_the_measurement_follows_the_track_not_a_chord(host):
    """over one interval the obstacle drives 8 m along +x and 8 m back (three knots): at the sample in the middle it is next to
    the car, at both ends 3.8 m behind it.  The chord between the interval's ends never leaves the start."""
    knots = np.array([(0.0, 0.0, 0.0), (8.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
    c = one_track(knots, np.array([0.0, 0.5, 1.0]), size=core.EGO_OFF, n_sub=2, exact=True)
    c["Ts"][...], c["k"][...] = 1.0, 1
    c["x_prev"][...] = c["x0"][...] = (8.0, 3.0, 0.0)                   # footprint y in [2.25, 3.75]; the obstacle's top edge at 0.625
    check_call(host, c, 1)
    assert c["track_clear_hist"][0, 0] == 1.625
    c["track_clear_hist"][...] = FILL_X
    c.dims["n_sub"] = 1                                                 # the ends alone
    check_call(host, c, 1)
    assert c["track_clear_hist"][0, 0] > 1.625


def test_struct_mirror_matches_the_header(host):
    check_struct_mirror(host.pool_tracks_layout_host, host.pool_tracks_init_host, _lib.ObcaPoolTracks)


SIZE = ctypes.sizeof(_lib.ObcaPoolTracks)
REFUSED = [dict(B=0), dict(Kt=0), dict(Kt=5), dict(K=65), dict(N=0), dict(N=128), dict(L=0), dict(L=4097), dict(group=0), dict(group=3),
           dict(max_steps=0), dict(max_steps=1025), dict(step=-1), dict(step=4), dict(n_sub=-1), dict(n_sub=257), dict(predict=-1),
           dict(predict=3), dict(clearance=float("nan")), dict(clearance=float("inf")), dict(margin=-0.5), dict(margin=float("inf")),
           dict(margin=float("nan")), dict(far=0.0), dict(far=-1.0), dict(far=float("inf")), dict(far=float("nan")), dict(struct_size=0),
           dict(struct_size=SIZE - 8), dict(struct_size=SIZE + 8)]


def test_refused_calls_touch_nothing(host):
    rng = np.random.default_rng(73)
    case = fill_world(Case(4, 2, 3, 3, 2, K=4), rng)
    before = case.snapshot()
    for over in REFUSED:
        call_host(host, case, 1, rc=E_INVAL, **over)
    for measure in (-1, 2):
        call_host(host, case, measure, rc=E_INVAL)
    for q in range(4):
        ego = list(case.ego)
        ego[q] = float("nan")
        call_host(host, case, 1, rc=E_INVAL, ego=(ctypes.c_double * 4)(*ego))
    for name in READ + WRITTEN:
        if name != "t0":
            call_host(host, case, 1, rc=E_INVAL, null=(name,))
    assert host.pool_tracks_host(None, 0) == E_INVAL
    assert all(core.same_words(case.whole[k], before[k]) for k in before)
    call_host(host, case, 1, null=("t0",))                             # t0 may be NULL: 0 for every rollout
    zero = fill_world(Case(4, 2, 3, 3, 2, K=4), np.random.default_rng(73))
    zero["t0"][...] = 0.0
    call_host(host, zero, 1)
    for name in WRITTEN:
        assert core.same_words(case[name], zero[name]), name
