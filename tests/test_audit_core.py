"""CPU tier of the collision audit: the geometry core csrc/obca_audit_core.h (built for the host from
tests/native/audit_host.cpp) against tests/kkt_check.py::polytope_distance on seeded car / obstacle pairs, the certified
lower bound between samples, and the argument checks of the C ABI (obca_plan_clearance, obca_rollouts_audit), which
refuse before any HIP call and so run without a GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import kkt_check, native_build
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.model_obstacle import obstacleModel, rectangle_vertices

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "audit_host.cpp")
EGO = (1.7, 0.75, 1.7, 0.75)
MAXM = 8                    # HOST_MAXM of audit_host.cpp
E_INVAL = -22


def load_host():
    lib = native_build.build_shim("audit_host", [SRC])
    lib.audit_host_distance.restype = ctypes.c_int
    lib.audit_host_interval.restype = ctypes.c_int
    lib.audit_host_box_next.restype = None
    lib.audit_host_plan_clearance.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def core_distance(host, poses, obstacles, ego=EGO):
    """poses [n,3]; obstacles: list of (A [m,2], b [m])"""
    n = len(obstacles)
    A, b = np.zeros((n, MAXM, 2)), np.zeros((n, MAXM))
    m = np.zeros(n, np.int32)
    for i, (Ai, bi) in enumerate(obstacles):
        m[i] = len(bi)
        A[i, :m[i]], b[i, :m[i]] = Ai, bi
    out = np.zeros(n)
    pose = np.ascontiguousarray(poses, float)
    assert host.audit_host_distance(n, _p(pose), _p(np.asarray(ego, float)), _p(A), _p(b), _p(m), _p(out)) == 0
    return out


def _rows(vertices):
    A, b = obstacleModel().obstacle_H_Represent(1, [len(vertices)], [vertices])
    return np.asarray(A, float), np.asarray(b, float)[:, 0]


def _clockwise(rng, k, centre, radius):
    """k points of a circle at random, clockwise (the reference's vertex order), closed by the first point again"""
    ang = np.sort(rng.uniform(0, 2 * math.pi, k))[::-1]
    pts = [[float(centre[0] + radius * math.cos(a)), float(centre[1] + radius * math.sin(a))] for a in ang]
    return pts + [pts[0]]


def _pairs(seed=7):
    """(kind, pose, A, b): half-planes, wedges, rotated boxes, convex 3-6-gons, touching cases; obstacles near the car so
    that separated and overlapping pairs both occur"""
    rng = np.random.default_rng(seed)
    out = []
    pose = lambda: np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-math.pi, math.pi)])
    for _ in range(400):                                          # half-planes (two-vertex lists)
        a = rng.uniform(0, 2 * math.pi)
        p = rng.uniform(-6, 6, 2)
        q = p + 3 * np.array([math.cos(a), math.sin(a)])
        A, b = _rows([[float(p[0]), float(p[1])], [float(q[0]), float(q[1])]])
        out.append(("halfplane", pose(), A, b))
    for _ in range(400):                                          # wedges: three consecutive clockwise points of a circle
        pts = _clockwise(rng, 5, rng.uniform(-5, 5, 2), rng.uniform(1, 6))[:3]
        A, b = _rows(pts)
        out.append(("wedge", pose(), A, b))
    for _ in range(400):                                          # boxes at arbitrary rotation
        v = rectangle_vertices(rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 5), rng.uniform(0.5, 5))
        A, b = _rows(v)
        out.append(("box", pose(), A, b))
    for k in (3, 4, 5, 6):                                        # convex k-gons
        for _ in range(200):
            A, b = _rows(_clockwise(rng, k, rng.uniform(-5, 5, 2), rng.uniform(0.5, 5)))
            out.append(("poly%d" % k, pose(), A, b))
    # touching: axis-aligned car at the origin (x in [-1.7, 1.7], y in [-0.75, 0.75]) and boxes / half-planes on its sides
    for _ in range(60):
        h = rng.uniform(0.5, 3)
        lo, hi = rng.uniform(-2, 0.5), rng.uniform(0.6, 3)
        out.append(("touch_box", np.zeros(3), *_rows([[1.7, hi], [1.7 + h, hi], [1.7 + h, lo], [1.7, lo], [1.7, hi]])))
        out.append(("touch_half", np.zeros(3), *_rows([[-5.0, -0.75], [5.0, -0.75]])))
    return out


def test_distance_equals_kkt_check(host):
    pairs = _pairs()
    keep = []
    for kind, pose, A, b in pairs:          # degenerate rows (parallel neighbours): the oracle solves a QP there, skip
        if len(b) == 2 and kkt_check._wedge_vertices(A, b) is None:
            continue
        if len(b) >= 3 and kkt_check._polygon_vertices(A, b) is None:
            continue
        keep.append((kind, pose, A, b))
    assert len(keep) >= 2000
    got = core_distance(host, np.array([q[1] for q in keep]), [(q[2], q[3]) for q in keep])
    ref = np.array([kkt_check.polytope_distance(kkt_check.car_corners(pose, EGO), A, b) for _, pose, A, b in keep])
    err = np.abs(got - ref)
    assert err.max() <= 1e-9, (err.max(), keep[int(np.argmax(err))][0])
    sure = np.abs(ref) > 1e-12
    assert (np.sign(got[sure]) == np.sign(ref[sure])).all()
    kinds = np.array([q[0] for q in keep])
    for k in ("halfplane", "wedge", "box", "poly3", "poly4", "poly5", "poly6"):       # every family separated and overlapping
        sel = kinds == k
        assert (ref[sel] > 0).sum() >= 20 and (ref[sel] < 0).sum() >= 20, k
    assert np.abs(ref[np.char.startswith(kinds, "touch")]).max() < 1e-12


def test_degenerate_rows_give_the_largest_row_gap(host):
    """parallel neighbouring rows: the documented fallback (the largest row gap)"""
    A = np.array([[0.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
    b = np.array([5.0, 6.0, 9.0])
    pose = np.array([[0.0, 0.0, 0.3]])
    got = core_distance(host, pose, [(A, b)])[0]
    car = kkt_check.car_corners(pose[0], EGO)
    gaps = (np.min(car @ A.T, axis=0) - b) / np.linalg.norm(A, axis=1)
    assert got == pytest.approx(gaps.max(), abs=1e-12)


def _interval(host, scene, p0, p1, b0, b1, n_sub):
    As, bs, m, dyn = scene
    out = np.zeros(6)
    rc = host.audit_host_interval(_p(np.asarray(EGO, float)), len(m), _p(m), _p(As), _p(bs), dyn.shape[0], _p(dyn),
                                  _p(np.asarray(p0, float)), _p(np.asarray(p1, float)), _p(np.ascontiguousarray(b0, float)),
                                  _p(np.ascontiguousarray(b1, float)), int(n_sub), _p(out))
    assert rc == 0
    return out


def test_lower_bound_below_dense_sampling(host):
    """the certified bound at n_sub = 4 never exceeds the sampled minimum at n_sub = 256"""
    rng = np.random.default_rng(11)
    hA, hb = _rows([[0.0, 9.0], [39.0, 9.0]])
    n_checked = 0
    for trial in range(300):
        box = rectangle_vertices(rng.uniform(10, 30), rng.uniform(3, 7), rng.uniform(-math.pi, math.pi), rng.uniform(1, 4), rng.uniform(1, 4))
        bA, bb = _rows(box)
        As = np.ascontiguousarray(np.concatenate([hA, bA]))
        bs = np.ascontiguousarray(np.concatenate([hb, bb]))
        m = np.array([1, 4], np.int32)
        dyn = np.zeros((2, 13))
        b0, b1 = np.zeros((2, 3)), np.zeros((2, 3))
        for j in range(2):
            th = rng.uniform(-math.pi, math.pi)
            dyn[j, 2:6] = th, 3.0, 3.0, rng.uniform(0.1, 0.5)
            dyn[j, 11], dyn[j, 12] = math.cos(th), math.sin(th)
            c0 = rng.uniform([5, 1], [35, 9])
            b0[j] = c0[0], c0[1], float(rng.uniform() < 0.8)
            c1 = c0 + rng.uniform(-0.5, 0.5, 2)
            b1[j] = c1[0], c1[1], 1.0 if b0[j, 2] else float(rng.uniform() < 0.5)    # some appear at the end knot
        p0 = np.array([rng.uniform(5, 35), rng.uniform(1, 9), rng.uniform(-math.pi, math.pi)])
        p1 = p0 + np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 0.5)])
        scene = (As, bs, m, dyn)
        coarse = _interval(host, scene, p0, p1, b0, b1, 4)
        dense = _interval(host, scene, p0, p1, b0, b1, 256)
        assert coarse[1] <= dense[0] + 1e-12, (trial, coarse, dense)
        assert coarse[1] <= coarse[0] and dense[1] <= dense[0]
        assert coarse[2] == dense[2] and coarse[3] == dense[3]             # the knots themselves do not depend on n_sub
        n_checked += 1
    assert n_checked == 300


def test_box_update_law(host):
    """appear at k == t_start, afterwards advance by T * speed along the heading (obca_rollout_core.h prepare())"""
    info = np.zeros(13)
    info[5], info[9], info[11], info[12] = 0.4, 3.0, math.cos(0.3), math.sin(0.3)
    out = np.zeros(3)
    host.audit_host_box_next(_p(info), ctypes.c_double(1.0), ctypes.c_double(2.0), 2, ctypes.c_double(0.5), _p(out))
    assert list(out) == [1.0, 2.0, 0.0]
    host.audit_host_box_next(_p(info), ctypes.c_double(1.0), ctypes.c_double(2.0), 3, ctypes.c_double(0.5), _p(out))
    assert list(out) == [1.0, 2.0, 1.0]
    host.audit_host_box_next(_p(info), ctypes.c_double(1.0), ctypes.c_double(2.0), 4, ctypes.c_double(0.5), _p(out))
    assert list(out) == [1.0 + 0.5 * 0.4 * info[11], 2.0 + 0.5 * 0.4 * info[12], 1.0]


# ------------------------------------------------------------------------------------------------ plan audit reduction
PLAN_M = {1: [1], 3: [1, 3, 1], 8: [1, 2, 3, 4, 1, 2, 3, 4]}    # obstacle 0 and TIE_OBST[n_obs] are half-planes
TIE_OBST = {1: None, 3: 2, 8: 4}


def _obstacle_rows(rng, m):
    """rows of one obstacle near the origin: half-plane (m = 1), wedge (2), triangle (3), rotated box (4)"""
    c = rng.uniform(-4, 4, 2)
    if m == 1:
        a = rng.uniform(0, 2 * math.pi)
        q = c + 3 * np.array([math.cos(a), math.sin(a)])
        return _rows([[float(c[0]), float(c[1])], [float(q[0]), float(q[1])]])
    if m == 4:
        return _rows(rectangle_vertices(c[0], c[1], rng.uniform(-math.pi, math.pi), rng.uniform(1, 4), rng.uniform(1, 4)))
    while True:
        pts = _clockwise(rng, 5, c, rng.uniform(1, 4))[:3] if m == 2 else _clockwise(rng, 3, c, rng.uniform(1, 4))
        A, b = _rows(pts)
        if (kkt_check._wedge_vertices(A, b) if m == 2 else kkt_check._polygon_vertices(A, b)) is not None:
            return A, b


def random_plans(rng, B, N, n_obs, variants=(0, 4, 6, 8)):
    """B plans over N + 1 stages against the obstacles of PLAN_M[n_obs], every stage's rows translated on their own:
    x [B,3,N+1], A [B,N+1,M,2], b [B,N+1,M], variant [B], and per instance the constructed tie (s0, s1) or None.  Poses
    over [-6, 6]^2 around obstacles in [-4, 4]^2, so both signs of distance occur.  Every other instance carries an exact
    tie: its stage s0 pose 40 m deep in half-plane 0 (the rows that stage is measured against), stage s1 > s0 a copy of
    stage s0 (pose and rows), half-plane TIE_OBST[n_obs] a copy of half-plane 0 -- so the smallest value occurs at
    (s0, 0), (s1, 0) and the copies; s1 = s0 + 64 (the same lane of a 64-wide segment) where N + 1 allows it."""
    m = PLAN_M[n_obs]
    M, N1 = sum(m), N + 1
    off = np.concatenate([[0], np.cumsum(m)]).astype(int)
    x = np.stack([rng.uniform(-6, 6, (B, N1)), rng.uniform(-6, 6, (B, N1)), rng.uniform(-math.pi, math.pi, (B, N1))], 1)
    A, b = np.zeros((B, N1, M, 2)), np.zeros((B, N1, M))
    variant = rng.choice(np.asarray(variants, np.int32), B).astype(np.int32)
    ties = []
    for i in range(B):
        rows = [_obstacle_rows(rng, mi) for mi in m]
        tie = i % 2 == 1 and (n_obs > 1 or N1 > 1)
        if tie and TIE_OBST[n_obs] is not None:
            rows[TIE_OBST[n_obs]] = rows[0]
        A0, b0 = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        for k in range(N1):
            t = rng.uniform(-1.5, 1.5, 2)
            A[i, k], b[i, k] = A0, b0 + A0 @ t
        if not tie:
            ties.append(None)
            continue
        s0 = int(rng.integers(0, N1 - 1))
        s1 = s0 + 64 if s0 + 64 < N1 and rng.uniform() < 0.5 else int(rng.integers(s0 + 1, N1))
        ks = 0 if variant[i] == 4 else s0
        a, bb = A[i, ks, 0], b[i, ks, 0]
        x[i, :2, s0] = a * bb / (a @ a) - 40.0 * a / np.linalg.norm(a)
        x[i, :, s1], A[i, s1], b[i, s1] = x[i, :, s0], A[i, s0], b[i, s0]
        ties.append((s0, s1))
    return x, A, b, variant, ties


def host_plan_clearance(host, x, A, b, m, variant=None, ego=EGO):
    """audit_host_plan_clearance: (min_clear [B], arg_stage [B], arg_obst [B], stage_obst [B,N+1,n_obs])"""
    B, N1 = x.shape[0], x.shape[2]
    mc, st, ob = np.zeros(B), np.zeros(B, np.int32), np.zeros(B, np.int32)
    so = np.zeros((B, N1, len(m)))
    x, A, b = (np.ascontiguousarray(a, float) for a in (x, A, b))
    var = None if variant is None else np.ascontiguousarray(variant, np.int32)
    rc = host.audit_host_plan_clearance(_p(np.asarray(ego, float)), len(m), _p(np.asarray(m, np.int32)), N1 - 1, B,
                                        None if var is None else _p(var), _p(x), _p(A), _p(b), _p(mc), _p(st), _p(ob), _p(so))
    assert rc == 0
    return mc, st, ob, so


def numpy_stage_obst(x, A, b, m, variant, idx, ego=EGO):
    """kkt_check.polytope_distance per (stage, obstacle) of the instances idx: [len(idx),N+1,n_obs]; stage 0's rows
    wherever the variant is 4"""
    off = np.concatenate([[0], np.cumsum(m)]).astype(int)
    out = np.zeros((len(idx), x.shape[2], len(m)))
    for r, i in enumerate(idx):
        for k in range(x.shape[2]):
            ks = 0 if variant is not None and variant[i] == 4 else k
            car = kkt_check.car_corners(x[i, :, k], ego)
            for o in range(len(m)):
                out[r, k, o] = kkt_check.polytope_distance(car, A[i, ks, off[o]:off[o + 1]], b[i, ks, off[o]:off[o + 1]])
    return out


def first_argmin(stage_obst):
    """(value, stage, obstacle) per instance under the audit's order: the first NaN in (stage, obstacle) order if there
    is one, else the first occurrence of the minimum (np.argmin does both)"""
    B, N1, n = stage_obst.shape
    flat = stage_obst.reshape(B, -1)
    am = np.argmin(flat, 1)
    return flat[np.arange(B), am], (am // n).astype(np.int32), (am % n).astype(np.int32)


@pytest.mark.parametrize("n_obs", [1, 3, 8])
def test_plan_reduction_equals_polytope_distance(host, n_obs):
    """the kernel's per-instance reduction, run serially: every (stage, obstacle) distance against kkt_check, the minimum
    and its (stage, obstacle) under the tie rule on constructed exact ties across stages and obstacles"""
    rng = np.random.default_rng(21 + n_obs)
    m = PLAN_M[n_obs]
    x, A, b, variant, ties = random_plans(rng, 48, 9, n_obs)
    mc, st, ob, so = host_plan_clearance(host, x, A, b, m, variant)
    ref = numpy_stage_obst(x, A, b, m, variant, range(len(x)))
    assert np.abs(so - ref).max() <= 1e-9
    assert (ref < 0).sum() >= 20 and (ref > 0).sum() >= 20
    v, s, o = first_argmin(so)
    assert np.array_equal(mc, v) and np.array_equal(st, s) and np.array_equal(ob, o)
    assert np.abs(mc - ref.reshape(len(x), -1).min(1)).max() <= 1e-9
    stage_ties = obst_ties = 0
    for i, t in enumerate(ties):                     # the constructed ties: the lower stage, then the lower obstacle wins
        if t is None:
            continue
        assert np.array_equal(so[i, t[0]], so[i, t[1]])
        if mc[i] == so[i, t[0]].min():
            assert (st[i], ob[i]) == (t[0], int(np.argmin(so[i, t[0]]))), (i, t, st[i], ob[i])
            stage_ties += 1
            obst_ties += TIE_OBST[n_obs] is not None and ob[i] == 0 and so[i, t[0], TIE_OBST[n_obs]] == mc[i]
    assert stage_ties >= 18 and (obst_ties >= 12 or n_obs == 1), (stage_ties, obst_ties)
    # variant 4 reads stage 0's rows only
    A2, b2 = A.copy(), b.copy()
    b2[:, 1:] -= 3.0
    mc2, st2, _, _ = host_plan_clearance(host, x, A2, b2, m, variant)
    v4 = variant == 4
    assert v4.any() and np.array_equal(mc2[v4], mc[v4]) and np.array_equal(st2[v4], st[v4])
    assert not np.array_equal(mc2[~v4], mc[~v4])


def nan_plans(rng, N=7, n_obs=3):
    """finite plans and one each of: a NaN pose at one stage, a NaN in one obstacle's row at one stage, an infinite pose,
    an all-NaN plan (variant 0).  Returns x, A, b, variant, the index of the first non-finite instance and, per non-finite
    instance, the (stage, obstacle) pairs that must measure NaN"""
    x, A, b, variant, _ = random_plans(rng, 12, N, n_obs)
    m = PLAN_M[n_obs]
    off = np.concatenate([[0], np.cumsum(m)]).astype(int)
    N1, B0 = N + 1, len(x)
    nx, nA, nb = x[:4].copy(), A[:4].copy(), b[:4].copy()
    nv = np.zeros(4, np.int32)
    bad = []
    nx[0, 1, 5] = np.nan                                            # NaN pose: every obstacle of that stage
    bad.append({(5, o) for o in range(n_obs)})
    nA[1, 3, off[n_obs - 1], 1] = np.nan                            # NaN row: that obstacle at that stage
    bad.append({(3, n_obs - 1)})
    nx[2, 0, 6] = np.inf                                            # infinite pose
    bad.append({(6, o) for o in range(n_obs)})
    nx[3] = np.nan                                                  # all NaN
    bad.append({(k, o) for k in range(N1) for o in range(n_obs)})
    return (np.concatenate([x, nx]), np.concatenate([A, nA]), np.concatenate([b, nb]), np.concatenate([variant, nv]),
            B0, bad)


def test_plan_reduction_reports_nan_for_non_finite_inputs(host):
    """a NaN or infinite pose, a NaN row, an all-NaN plan: the pairs they touch measure NaN, min_clear is NaN and the
    arg-min names the first such pair -- never the minimum of the finite rest (which would call "unknown" "safe")"""
    rng = np.random.default_rng(5)
    m = PLAN_M[3]
    x, A, b, variant, B0, bad = nan_plans(rng)
    mc, st, ob, so = host_plan_clearance(host, x, A, b, m, variant)
    assert np.isfinite(so[:B0]).all() and np.isfinite(mc[:B0]).all()
    for j, pairs in enumerate(bad):
        i = B0 + j
        got = {(int(k), int(o)) for k, o in zip(*np.nonzero(np.isnan(so[i])))}
        assert got == pairs, (j, got)
        assert np.isnan(mc[i]), (j, mc[i])
        assert (st[i], ob[i]) == min(pairs), (j, st[i], ob[i])
    assert (st[B0 + 3], ob[B0 + 3]) == (0, 0)
    ref = host_plan_clearance(host, x[:B0], A[:B0], b[:B0], m, variant[:B0])      # the finite instances do not notice
    for got, want in zip((mc, st, ob, so), ref):
        assert np.array_equal(got[:B0], want)


def test_better_orders_nan_first_then_value_stage_obstacle(host):
    """the order itself through the reduction: one instance, one stage per value, the values given directly"""
    # two obstacles, half-planes y <= b: the car at the origin (heading 0, y in [-0.75, 0.75]) measures -0.75 - b
    cases = [([7.3, np.nan, -0.7], np.nan, 1), ([7.3, 2.0, -0.7], -0.7, 2), ([np.nan] * 3, np.nan, 0),
             ([1.0, 1.0, 1.0], 1.0, 0), ([np.inf, 1.0, 2.0], np.nan, 0), ([-np.inf, 1.0, 2.0], np.nan, 0)]
    for vals, want, stage in cases:
        N1 = len(vals)
        x = np.zeros((1, 3, N1))
        A = np.zeros((1, N1, 2, 2))
        A[..., 1] = 1.0
        b = np.zeros((1, N1, 2))
        for k, v in enumerate(vals):
            b[0, k] = -0.75 - v if np.isfinite(v) else v
        mc, st, ob, so = host_plan_clearance(host, x, A, b, [1, 1])
        if np.isnan(want):
            assert np.isnan(mc[0]), (vals, mc[0])
        else:
            assert mc[0] == pytest.approx(want, abs=1e-12), (vals, mc[0])
        assert (st[0], ob[0]) == (stage, 0), (vals, st[0], ob[0])


# ------------------------------------------------------------------------------------------------ C ABI argument checks
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
    ge.build()
    return _lib.load()


def _plan_call(lib, **over):
    """obca_plan_clearance with valid host-side arguments, some replaced; the device arrays are never reached when the
    call is refused (they are plain host buffers here)"""
    buf = np.zeros(64)
    ibuf = np.zeros(64, np.int32)
    a = dict(ego=(ctypes.c_double * 4)(*EGO), n_obs=2, m=(ctypes.c_int32 * 2)(1, 4), N=5, B=4, variant=None,
             x=_p(buf), A=_p(buf), b=_p(buf), min_clear=_p(buf), arg_stage=_p(ibuf), arg_obst=_p(ibuf), stage_obst=None,
             device=0, stream=None)
    a.update(over)
    return lib.obca_plan_clearance(a["ego"], a["n_obs"], a["m"], a["N"], a["B"], a["variant"], a["x"], a["A"], a["b"],
                                   a["min_clear"], a["arg_stage"], a["arg_obst"], a["stage_obst"], a["device"], a["stream"])


@pytest.mark.parametrize("bad", [
    dict(B=0), dict(B=-3), dict(N=0), dict(n_obs=0), dict(n_obs=9), dict(m=None),
    dict(m=(ctypes.c_int32 * 2)(0, 4)), dict(m=(ctypes.c_int32 * 2)(1, 5)),
    dict(ego=None), dict(ego=(ctypes.c_double * 4)(-1.7, 0.75, 0.0, 0.75)), dict(ego=(ctypes.c_double * 4)(1.7, -0.75, 1.7, 0.0)),
    dict(ego=(ctypes.c_double * 4)(float("nan"), 0.75, 1.7, 0.75)),
    dict(x=None), dict(A=None), dict(b=None), dict(min_clear=None), dict(arg_stage=None), dict(arg_obst=None),
    dict(device=-1)])
def test_plan_clearance_rejects_bad_arguments(lib, bad):
    assert _plan_call(lib, **bad) == E_INVAL


@pytest.mark.parametrize("bad", ["handle", "n_sub0", "n_sub_neg", "min_clear", "lower_bound", "arg_step", "arg_obst",
                                 "first_collision", "first_violation"])
def test_rollouts_audit_rejects_bad_arguments(lib, bad):
    buf = np.zeros(8)
    ibuf = np.zeros(8, np.int32)
    a = dict(n_sub=8, min_clear=_p(buf), lower_bound=_p(buf), arg_step=_p(ibuf), arg_obst=_p(ibuf), first_collision=_p(ibuf),
             first_violation=_p(ibuf))
    if bad == "n_sub0":
        a["n_sub"] = 0
    elif bad == "n_sub_neg":
        a["n_sub"] = -2
    elif bad != "handle":
        a[bad] = None
    # a NULL handle (every case) -- the other checks come first, so each case is refused on its own argument as well
    rc = lib.obca_rollouts_audit(None, a["n_sub"], a["min_clear"], a["lower_bound"], a["arg_step"], a["arg_obst"],
                                 a["first_collision"], a["first_violation"], None, None)
    assert rc == E_INVAL
    assert lib.obca_strerror(rc) == b"invalid argument or shape beyond compiled limits"
