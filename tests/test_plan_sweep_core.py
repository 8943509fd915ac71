"""CPU tier of the swept plan audit (audit::plan_interval of csrc/obca_audit_core.h, obca_plan_sweep's per-instance work),
built for the host from tests/native/plan_sweep_host.cpp: samples between the knots of a plan against
tests/kkt_check.py::polytope_distance on poses and rows interpolated in numpy (1e-9, the bound of every audit test against
that helper), the arg-min's tie rule, the certified bound against dense sampling, variant 4's stage-0 rows and the NaN
rules.  The cases are built once and shared with tests/test_gpu_plan_sweep.py."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import kkt_check, native_build
from tests import test_audit_core as core
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.model_obstacle import rectangle_vertices

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "plan_sweep_host.cpp")
EGO = core.EGO
TOL = 1e-9
M3 = [1, 2, 4]                    # a half-plane, a wedge and a box


def load_host():
    lib = native_build.build_shim("plan_sweep_host", [SRC])
    lib.plan_sweep_host.restype = ctypes.c_int
    lib.plan_sweep_host_move.restype = ctypes.c_double
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


_p = core._p


def host_sweep(host, x, A, b, m, variant, n_sub, samples=False, ego=EGO):
    """plan_sweep_host: dict of min_clear, lower_bound, arg_interval, arg_obst, first_collision [B], interval_min [B,N] and,
    on request, samples [B,N,n_sub+1]"""
    B, N = x.shape[0], x.shape[2] - 1
    x, A, b = (np.ascontiguousarray(a, float) for a in (x, A, b))
    var = None if variant is None else np.ascontiguousarray(variant, np.int32)
    o = {"min_clear": np.zeros(B), "lower_bound": np.zeros(B), "arg_interval": np.zeros(B, np.int32),
         "arg_obst": np.zeros(B, np.int32), "first_collision": np.zeros(B, np.int32), "interval_min": np.zeros((B, N))}
    if samples:
        o["samples"] = np.zeros((B, N, n_sub + 1))
    rc = host.plan_sweep_host(_p(np.asarray(ego, float)), len(m), _p(np.asarray(m, np.int32)), N, B, None if var is None else _p(var),
                              _p(x), _p(A), _p(b), int(n_sub), _p(o["min_clear"]), _p(o["lower_bound"]), _p(o["arg_interval"]),
                              _p(o["arg_obst"]), _p(o["first_collision"]), _p(o["interval_min"]),
                              _p(o["samples"]) if samples else None)
    assert rc == 0
    return o


# ---------------------------------------------------------------------------------------------------------- references
def lerp(v0, v1, n_sub, j):
    """sample j of a linear interpolation, the ends being the stages' own words"""
    return v0 if j == 0 else (v1 if j == n_sub else v0 + (j / n_sub) * (v1 - v0))


def numpy_samples(x, A, b, m, variant, n_sub, ego=EGO):
    """kkt_check.polytope_distance on interpolated poses and rows: [B,N,n_sub+1,n_obs]; stage 0's rows wherever the variant
    is 4"""
    off = np.concatenate([[0], np.cumsum(m)]).astype(int)
    B, N = x.shape[0], x.shape[2] - 1
    out = np.zeros((B, N, n_sub + 1, len(m)))
    for i in range(B):
        for s in range(N):
            k0, k1 = (0, 0) if variant is not None and variant[i] == 4 else (s, s + 1)
            for j in range(n_sub + 1):
                car = kkt_check.car_corners(lerp(x[i, :, s], x[i, :, s + 1], n_sub, j), ego)
                Aj, bj = lerp(A[i, k0], A[i, k1], n_sub, j), lerp(b[i, k0], b[i, k1], n_sub, j)
                for o in range(len(m)):
                    out[i, s, j, o] = kkt_check.polytope_distance(car, Aj[off[o]:off[o + 1]], bj[off[o]:off[o + 1]])
    return out


def expected_reduction(d):
    """d [B,N,n_sub+1,n_obs] -> interval_min [B,N], min_clear, arg_interval, arg_obst [B] under the audit's order: value,
    then the lowest interval, then the lowest obstacle (a minimum on a shared knot belongs to the earlier interval)"""
    B, N = d.shape[:2]
    per = d.min(2)                                                            # [B,N,n_obs]
    imin = per.min(2)
    mc = imin.min(1)
    ai = np.array([int(np.flatnonzero(imin[i] == mc[i])[0]) for i in range(B)], np.int32)
    ao = np.array([int(np.flatnonzero(per[i, ai[i]] == mc[i])[0]) for i in range(B)], np.int32)
    return imin, mc, ai, ao


def vec_distance(poses, A, b, ego=EGO):
    """kkt_check.polytope_distance restated over K samples at once (poses [K,3], A [K,m,2], b [K,m], rows that have
    vertices): the 512 samples per interval of the bound test cost minutes one call at a time.
    test_vectorised_reference_is_polytope_distance holds it to the helper itself."""
    K, m = b.shape
    L, W = ego[0] + ego[2], ego[1] + ego[3]
    offc = L / 2 - ego[2]
    c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
    cx, cy = poses[:, 0] + c * offc, poses[:, 1] + s * offc
    car = np.stack([np.stack([cx + c * dx - s * dy, cy + s * dx + c * dy], -1)
                    for dx, dy in ((L / 2, W / 2), (L / 2, -W / 2), (-L / 2, -W / 2), (-L / 2, W / 2))], 1)    # [K,4,2]
    gaps = (np.einsum("kvc,krc->kvr", car, A).min(1) - b) / np.linalg.norm(A, axis=-1)
    if m == 1:
        return gaps[:, 0]
    cross = lambda u, v: u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    if m == 2:
        a1, a2 = A[:, 0], A[:, 1]
        det = cross(a1, a2)
        apex = np.stack([(b[:, 0] * a2[:, 1] - a1[:, 1] * b[:, 1]) / det, (a1[:, 0] * b[:, 1] - b[:, 0] * a2[:, 0]) / det], -1)
        d1 = np.stack([-a1[:, 1], a1[:, 0]], -1) / np.linalg.norm(a1, axis=-1, keepdims=True)
        d1 = np.where((np.einsum("kc,kc->k", a2, d1) > 0)[:, None], -d1, d1)
        d2 = np.stack([-a2[:, 1], a2[:, 0]], -1) / np.linalg.norm(a2, axis=-1, keepdims=True)
        d2 = np.where((np.einsum("kc,kc->k", a1, d2) > 0)[:, None], -d2, d2)
        V = np.stack([apex, apex + 1e4 * d1, apex + 1e4 * (d1 + d2), apex + 1e4 * d2], 1)
    else:
        V = []
        for j in range(m):
            a1, a2, j1 = A[:, j], A[:, (j + 1) % m], (j + 1) % m
            det = cross(a1, a2)
            V.append(np.stack([(b[:, j] * a2[:, 1] - a1[:, 1] * b[:, j1]) / det, (a1[:, 0] * b[:, j1] - b[:, j] * a2[:, 0]) / det], -1))
        V = np.stack(V, 1)
    best = gaps.max(1)
    for i in range(4):
        e = car[:, (i + 1) % 4] - car[:, i]
        n = np.stack([e[:, 1], -e[:, 0]], -1) / np.maximum(np.linalg.norm(e, axis=-1, keepdims=True), 1e-300)
        inside = np.einsum("kvc,kc->kv", car - car[:, i:i + 1], n).max(1)
        n = np.where((inside > 1e-12)[:, None], -n, n)
        best = np.maximum(best, np.einsum("kvc,kc->kv", V - car[:, i:i + 1], n).min(1))
    dm = np.full(K, np.inf)
    for P, Q in ((car, V), (V, car)):
        for i in range(Q.shape[1]):
            a0, ab = Q[:, i], Q[:, (i + 1) % Q.shape[1]] - Q[:, i]
            for v in range(P.shape[1]):
                t = np.clip(np.einsum("kc,kc->k", P[:, v] - a0, ab) / np.maximum(np.einsum("kc,kc->k", ab, ab), 1e-300), 0.0, 1.0)
                dm = np.minimum(dm, np.linalg.norm(P[:, v] - (a0 + t[:, None] * ab), axis=-1))
    return np.where(best <= 0.0, best, dm)


def dense_minimum(x, A, b, m, n_dense):
    """[B] smallest vec_distance over n_dense + 1 samples of every interval and every obstacle"""
    off = np.concatenate([[0], np.cumsum(m)]).astype(int)
    B, N = x.shape[0], x.shape[2] - 1
    t = (np.arange(n_dense + 1) / n_dense)[:, None]
    out = np.full(B, np.inf)
    for i in range(B):
        for s in range(N):
            poses = x[i, :, s][None] + t * (x[i, :, s + 1] - x[i, :, s])[None]
            Aj = A[i, s][None] + t[:, :, None] * (A[i, s + 1] - A[i, s])[None]
            bj = b[i, s][None] + t * (b[i, s + 1] - b[i, s])[None]
            for o in range(len(m)):
                out[i] = min(out[i], vec_distance(poses, Aj[:, off[o]:off[o + 1]], bj[:, off[o]:off[o + 1]]).min())
    return out


# --------------------------------------------------------------------------------------------------------------- cases
def translating_plans(rng, B, N, m, step=1.0, reach=1.5, turn=0.6):
    """B plans of N + 1 stages; every obstacle translates from stage to stage by a step of its own (up to `step` per
    coordinate), the car moves by up to `reach` per coordinate and `turn` rad per stage.  Poses over [-6, 6]^2 around
    obstacles in [-4, 4]^2, so that both signs of distance occur."""
    M, N1 = sum(m), N + 1
    off = np.concatenate([[0], np.cumsum(m)]).astype(int)
    x = np.zeros((B, 3, N1))
    A, b = np.zeros((B, N1, M, 2)), np.zeros((B, N1, M))
    for i in range(B):
        x[i, :, 0] = rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-math.pi, math.pi)
        for k in range(1, N1):
            x[i, :, k] = x[i, :, k - 1] + np.array([rng.uniform(-reach, reach), rng.uniform(-reach, reach), rng.uniform(-turn, turn)])
        for o, mi in enumerate(m):
            A0, b0 = core._obstacle_rows(rng, mi)
            c = np.zeros(2)
            for k in range(N1):
                A[i, k, off[o]:off[o + 1]], b[i, k, off[o]:off[o + 1]] = A0, b0 + A0 @ c
                c = c + rng.uniform(-step, step, 2)
    return x, A, b


def case_knots():
    """case 1: random plans, N = 3, obstacles of 1, 2 and 4 rows, B = 7"""
    x, A, b = translating_plans(np.random.default_rng(101), 7, 3, M3)
    return dict(x=x, A=A, b=b, m=M3, variant=None)


def case_ties():
    """two copies of one half-plane, the deepest pose at an interior knot: obstacle 0 and the earlier interval win"""
    x, A, b = translating_plans(np.random.default_rng(102), 4, 4, [1, 1])
    A[:, :, 1], b[:, :, 1] = A[:, :, 0], b[:, :, 0]
    for i in range(4):
        k = 1 + i % 3
        a, bb = A[i, k, 0], b[i, k, 0]
        x[i, :2, k] = a * bb / (a @ a) - 40.0 * a / np.linalg.norm(a)
    return dict(x=x, A=A, b=b, m=[1, 1], variant=None)


def case_corner_cut():
    """case 2: the square [0, 2]^2 and an axis-aligned car (3.4 x 1.5 m about its pose point) that goes from its right
    side (0.4 m clear) to above it (0.45 m clear): halfway the car covers the corner (2, 2), 0.4 m deep"""
    A0, b0 = core._rows([[0.0, 0.0], [0.0, 2.0], [2.0, 2.0], [2.0, 0.0], [0.0, 0.0]])
    x = np.array([[[4.1, 1.0], [1.5, 3.2], [0.0, 0.0]]])
    A, b = np.stack([A0, A0])[None], np.stack([b0, b0])[None]
    return dict(x=x, A=A, b=b, m=[4], variant=None)


BOX = dict(c0=np.array([1.0, -2.0]), step=np.array([0.7, 0.45]), th=0.4, length=3.0, width=1.5)


def box_rows(centre):
    return core._rows(rectangle_vertices(float(centre[0]), float(centre[1]), BOX["th"], BOX["length"], BOX["width"]))


def case_translating_box():
    """case 3: one rectangle moved by a constant step per stage, its rows built from the moved vertices at every stage
    (A equal across the stages only to roundoff); N = 4"""
    N1 = 5
    rows = [box_rows(BOX["c0"] + k * BOX["step"]) for k in range(N1)]
    A, b = np.stack([r[0] for r in rows])[None], np.stack([r[1] for r in rows])[None]
    x = np.array([[np.linspace(-3.0, 5.0, N1), np.linspace(-4.5, 2.0, N1), np.linspace(0.2, 1.3, N1)]])
    return dict(x=x, A=A, b=b, m=[4], variant=None)


def case_bound(n=200):
    """case 4: n (plan, scene) pairs of one interval each.  A random half-plane holds the car half of the time; in two
    pairs of three it is turned round where it does, so that clear and colliding pairs both occur in numbers"""
    x, A, b = translating_plans(np.random.default_rng(104), n, 1, M3)
    for i in range(n):
        if i % 3 and A[i, 0, 0] @ x[i, :2, 0] < b[i, 0, 0]:
            A[i, :, 0], b[i, :, 0] = -A[i, :, 0], -b[i, :, 0]
    return dict(x=x, A=A, b=b, m=M3, variant=None)


def case_variant4():
    """case 5: variants 4 and 6 mixed; the stages after the first hold other rows (moved and turned)"""
    rng = np.random.default_rng(105)
    x, A, b = translating_plans(rng, 8, 3, M3)
    rot = np.array([[math.cos(0.3), -math.sin(0.3)], [math.sin(0.3), math.cos(0.3)]])
    A[:, 1:] = A[:, 1:] @ rot.T
    b[:, 1:] -= 3.0
    return dict(x=x, A=A, b=b, m=M3, variant=np.array([4, 6, 4, 4, 8, 4, 0, 4], np.int32))


def case_nan():
    """case 6: instance 0 finite; 1: a NaN pose at stage 2; 2: obstacle 1 turns between stages 1 and 2 (A changes by
    1e-3); 3: obstacle 2 changes shape between stages 0 and 1 (one row of the box moves alone)"""
    x, A, b = translating_plans(np.random.default_rng(106), 1, 4, M3)
    x, A, b = np.repeat(x, 4, 0), np.repeat(A, 4, 0), np.repeat(b, 4, 0)
    x[1, 0, 2] = np.nan
    A[2, 2:, 1:3] = A[2, 2:, 1:3] @ np.array([[math.cos(1e-3), -math.sin(1e-3)], [math.sin(1e-3), math.cos(1e-3)]]).T
    b[3, 1:, 3] += 1e-3 * np.linalg.norm(A[3, 1, 3])
    return dict(x=x, A=A, b=b, m=M3, variant=None)


# (name, case, the n_sub values the device is compared at): cases 1-6 of the feature's tests
def all_cases():
    return [("knots", case_knots(), (1, 16)), ("ties", case_ties(), (1, 3)), ("corner_cut", case_corner_cut(), (1, 16)),
            ("translating_box", case_translating_box(), (1, 8)), ("bound", case_bound(), (1, 2, 5, 16)),
            ("variant4", case_variant4(), (1, 16)), ("nan", case_nan(), (1, 16))]


def sweep(host, c, n_sub, **kw):
    return host_sweep(host, c["x"], c["A"], c["b"], c["m"], c["variant"], n_sub, **kw)


# --------------------------------------------------------------------------------------------------------------- tests
def test_knots_only(host):
    c = case_knots()
    got = sweep(host, c, 1, samples=True)
    d = numpy_samples(c["x"], c["A"], c["b"], c["m"], None, 1)
    assert (d < 0).any() and (d > 0).any()
    knots = np.concatenate([d[:, :, 0], d[:, -1:, 1]], 1).min(-1)               # [B,N+1] from numpy
    assert np.abs(got["interval_min"] - np.minimum(knots[:, :-1], knots[:, 1:])).max() <= TOL
    assert np.abs(got["min_clear"] - knots.min(1)).max() <= TOL
    assert np.abs(got["samples"] - d.min(-1)).max() <= TOL
    imin, mc, ai, ao = expected_reduction(d)
    assert np.array_equal(got["arg_interval"], ai) and np.array_equal(got["arg_obst"], ao)
    assert (got["min_clear"] == got["interval_min"].min(1)).all()
    k = np.argmin(knots, 1)                                                     # a minimum on a shared knot: the earlier interval
    assert np.array_equal(ai, np.maximum(k - 1, 0)) and ((k >= 1) & (k < 3)).any(), k
    assert np.array_equal(got["first_collision"], [int(np.argmax(r < 0)) if (r < 0).any() else -1 for r in got["interval_min"]])
    assert np.isfinite(got["lower_bound"]).all() and (got["lower_bound"] <= got["min_clear"]).all()


def test_ties_go_to_the_lowest_interval_then_obstacle(host):
    c = case_ties()
    for n_sub in (1, 3):
        got = sweep(host, c, n_sub)
        assert np.array_equal(got["arg_interval"], [0, 1, 2, 0]) and np.array_equal(got["arg_obst"], [0, 0, 0, 0]), n_sub
        k = got["arg_interval"] + 1
        assert (got["interval_min"][np.arange(4), k - 1] == got["interval_min"][np.arange(4), k]).all()
        assert (got["min_clear"] < -30).all()


def test_corner_cut_between_clear_knots(host):
    """the case the sweep exists for: a knot audit calls this plan clear"""
    c = case_corner_cut()
    knots = numpy_samples(c["x"], c["A"], c["b"], c["m"], None, 1)[0, 0, :, 0]
    assert (knots >= 0.3).all(), knots
    k1 = sweep(host, c, 1)
    assert np.abs(k1["min_clear"][0] - knots.min()) <= TOL and k1["first_collision"][0] == -1
    got = sweep(host, c, 16, samples=True)
    d = numpy_samples(c["x"], c["A"], c["b"], c["m"], None, 16)
    assert np.abs(got["samples"] - d.min(-1)).max() <= TOL
    assert got["min_clear"][0] < -0.3 and abs(got["samples"][0, 0, 8] + 0.4) <= TOL    # sample 8: halfway, 0.4 m deep
    assert got["first_collision"][0] == 0 and got["arg_interval"][0] == 0 and got["arg_obst"][0] == 0
    assert got["lower_bound"][0] <= got["min_clear"][0]
    assert k1["lower_bound"][0] <= got["min_clear"][0]                           # the knots' own bound knows already


def test_translating_box(host):
    c = case_translating_box()
    A, b = c["A"][0], c["b"][0]
    assert np.abs(A[1:] - A[0]).max() <= 1e-12 * np.abs(A[0]).max()
    n_sub = 8
    got = sweep(host, c, n_sub, samples=True)
    for s in range(4):
        for j in range(n_sub + 1):
            Aj, bj = box_rows(BOX["c0"] + (s + j / n_sub) * BOX["step"])       # the box at the interpolated centre
            car = kkt_check.car_corners(lerp(c["x"][0, :, s], c["x"][0, :, s + 1], n_sub, j), EGO)
            assert abs(got["samples"][0, s, j] - kkt_check.polytope_distance(car, Aj, bj)) <= TOL, (s, j)
    assert (got["samples"] < 0).any() and (got["samples"] > 0).any()
    assert np.isfinite(got["lower_bound"][0]) and got["lower_bound"][0] <= got["min_clear"][0]
    for k in range(4):                                                          # the fitted translation is the step
        mv = host.plan_sweep_host_move(_p(A[k].copy()), _p(b[k].copy()), _p(A[k + 1].copy()), _p(b[k + 1].copy()), 4)
        assert abs(mv - np.linalg.norm(BOX["step"])) <= 1e-9


@pytest.fixture(scope="module")
def bound_case():
    c = case_bound()
    return c, dense_minimum(c["x"], c["A"], c["b"], c["m"], 512)


def test_vectorised_reference_is_polytope_distance(bound_case):
    c, _ = bound_case
    rng = np.random.default_rng(3)
    off = np.concatenate([[0], np.cumsum(c["m"])]).astype(int)
    worst, signs = 0.0, set()
    for i in rng.choice(len(c["x"]), 40, replace=False):
        t = rng.uniform(0, 1, 6)[:, None]
        poses = c["x"][i, :, 0][None] + t * (c["x"][i, :, 1] - c["x"][i, :, 0])[None]
        Aj = c["A"][i, 0][None] + t[:, :, None] * (c["A"][i, 1] - c["A"][i, 0])[None]
        bj = c["b"][i, 0][None] + t * (c["b"][i, 1] - c["b"][i, 0])[None]
        for o in range(3):
            v = vec_distance(poses, Aj[:, off[o]:off[o + 1]], bj[:, off[o]:off[o + 1]])
            for q in range(len(t)):
                ref = kkt_check.polytope_distance(kkt_check.car_corners(poses[q], EGO), Aj[q, off[o]:off[o + 1]], bj[q, off[o]:off[o + 1]])
                worst = max(worst, abs(v[q] - ref))
                signs.add((o, ref > 0))
    assert worst <= 1e-12, worst
    assert len(signs) == 6                                                      # every kind separated and overlapping


def test_bound_is_a_bound(host, bound_case):
    c, dense = bound_case
    assert (dense < 0).sum() >= 20 and (dense > 0).sum() >= 20
    lb = {}
    for n_sub in (1, 2, 5, 16):
        got = sweep(host, c, n_sub)
        lb[n_sub] = got["lower_bound"]
        assert np.isfinite(lb[n_sub]).all(), n_sub
        assert (lb[n_sub] <= dense + 1e-12).all(), (n_sub, float((lb[n_sub] - dense).max()))
        assert (lb[n_sub] <= got["min_clear"]).all(), n_sub
        if 512 % n_sub == 0:                                                     # these samples are among the 513
            assert (got["min_clear"] >= dense - TOL).all(), n_sub
    assert (lb[16] >= lb[1] - 1e-12).all()
    assert (lb[16] > lb[1] + 1e-3).any()                                         # and finer sampling does tighten it


def test_variant_4_reads_stage_0_rows(host):
    c = case_variant4()
    v4 = c["variant"] == 4
    got = sweep(host, c, 16, samples=True)
    d = numpy_samples(c["x"], c["A"], c["b"], c["m"], c["variant"], 16)
    assert np.abs(got["samples"] - d.min(-1)).max() <= TOL
    same = dict(c, A=np.repeat(c["A"][:, :1], 4, 1), b=np.repeat(c["b"][:, :1], 4, 1))     # stage 0's rows everywhere
    ref = sweep(host, same, 16, samples=True)
    for k in got:
        assert np.array_equal(got[k][v4], ref[k][v4]), k
    assert not np.array_equal(got["samples"][~v4], ref["samples"][~v4])
    assert np.isfinite(got["lower_bound"][v4]).all()                             # standing rows: certified
    assert np.isnan(got["lower_bound"][~v4]).all()                               # the others' rows turn after stage 0


def test_nan_rules(host):
    c = case_nan()
    for n_sub in (1, 16):
        got = sweep(host, c, n_sub)
        assert np.isfinite(got["min_clear"][0]) and np.isfinite(got["lower_bound"][0])
        # a NaN pose at stage 2: intervals 1 and 2 measure NaN, the first of them is reported
        assert np.isnan(got["min_clear"][1]) and got["arg_interval"][1] == 1 and got["arg_obst"][1] == 0
        assert np.array_equal(np.isnan(got["interval_min"][1]), [False, True, True, False])
        assert np.array_equal(got["interval_min"][1, [0, 3]], got["interval_min"][0, [0, 3]])
        assert np.isnan(got["lower_bound"][1])
        # a turning obstacle, one that changes shape: the samples stand, the bound is not certified
        for i in (2, 3):
            assert np.isfinite(got["interval_min"][i]).all() and np.isnan(got["lower_bound"][i]), i
            assert got["min_clear"][i] == got["interval_min"][i].min()
    d = numpy_samples(c["x"][2:], c["A"][2:], c["b"][2:], c["m"], None, 16)
    assert np.abs(sweep(host, c, 16)["interval_min"][2:] - d.min((2, 3))).max() <= TOL
