"""CPU tier of the scene-pool selection (csrc/obca_scene_core.h: obca_scene_select's per-obstacle score, per-instance ranking
and per-row gather), built for the host from tests/native/scene_host.cpp.

Yardsticks: the score against a numpy restatement built on tests/kkt_check.py (``car_corners``, ``polytope_distance`` -- the
helpers the audit tests use) at 1e-12 m: coordinates stay below 100 m, where a double resolves 1.4e-14 m, and the two
evaluation orders differ by a few of those.  The moving rows against numpy with the same operations in the same order,
word for word.  The selection against ``np.lexsort((index, score))``, the gather against fancy indexing, exactly.  Then the
loop's mechanics with scripted plans (no solver), every rule that makes an instance unusable with its exact fill, and the
refused calls with guard-banded outputs.  The helpers are shared with tests/test_gpu_scene.py."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from tests import kkt_check, native_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "scene_host.cpp")
E_INVAL = -22
EGO = (1.7, 0.75, 1.7, 0.75)
SCORE_TOL = 1e-12
GUARD = 8
FILL_X, FILL_I = -777.25, -777
FILL_B = -1e6
OUTPUTS = ("score", "sel", "A", "b", "variant_out", "ok", "min_clear")


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def load_host():
    lib = native_build.build_shim("scene_host", [SRC])
    lib.scene_select_host.restype = ctypes.c_int
    lib.scene_row_b_host.restype = ctypes.c_double
    lib.scene_row_b_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


def words(a):
    return np.ascontiguousarray(a, float).view(np.uint64)


def banded(shape, dtype, fill):
    """(whole, view): a buffer of GUARD + prod(shape) + GUARD elements filled with ``fill`` and its middle as ``shape``;
    float64 buffers are 16-byte aligned in the middle (GUARD is even and numpy aligns to 16)"""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, fill, dtype)
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def band_clean(whole, fill):
    return bool(np.all(whole[:GUARD] == fill) and np.all(whole[-GUARD:] == fill))


def out_shapes(B, K, E, N, n_sel):
    n_sel = max(int(n_sel), 1)
    return {"score": ((B, K), np.float64, FILL_X), "sel": ((B, n_sel), np.int32, FILL_I),
            "A": ((B, N + 1, n_sel * E, 2), np.float64, FILL_X), "b": ((B, N + 1, n_sel * E), np.float64, FILL_X),
            "variant_out": ((B,), np.int32, FILL_I), "ok": ((B,), np.int32, FILL_I), "min_clear": ((B,), np.float64, FILL_X)}


def host_select(host, pool_A, pool_b, x, n_sel, pool_v=None, Ts=None, x0=None, variant=None, status=None, n_sub=1, state=None,
                ego=EGO, rc=0, null=(), over=None):
    """scene_select_host on numpy arrays: a dict of the outputs (views into guard-banded buffers pre-filled with FILL_X /
    FILL_I; ``_whole`` holds the buffers).  state: (score, sel) of an earlier call, copied in (accumulate = 1).  ``null``: names
    of pointers handed over as NULL; ``over``: scalar arguments the call is told instead of the arrays' own (B, K, E, N,
    n_sel, n_sub, accumulate)"""
    pool_A, pool_b, x = (np.ascontiguousarray(a, float) for a in (pool_A, pool_b, x))
    B, K, E = pool_b.shape
    N = x.shape[2] - 1
    f = lambda a, dt=float: None if a is None else np.ascontiguousarray(a, dt)
    a = {"ego": np.ascontiguousarray(ego, float), "pool_A": pool_A, "pool_b": pool_b, "pool_v": f(pool_v), "Ts": f(Ts), "x": x,
         "x0": f(x0), "variant": f(variant, np.int32), "status": f(status, np.int32)}
    o, whole = {}, {}
    for k, (shape, dt, fill) in out_shapes(B, K, E, N, n_sel).items():
        whole[k], o[k] = banded(shape, dt, fill)
    if state is not None:
        o["score"][...] = state[0]
        o["sel"][...] = state[1]
    a.update(o)
    for k in null:
        a[k] = None
    s = dict(B=B, K=K, E=E, N=N, n_sel=n_sel, n_sub=n_sub, accumulate=0 if state is None else 1)
    s.update(over or {})
    got = host.scene_select_host(_p(a["ego"]), s["B"], s["K"], s["E"], s["N"], s["n_sel"], s["n_sub"], s["accumulate"],
                                 _p(a["pool_A"]), _p(a["pool_b"]), _p(a["pool_v"]), _p(a["Ts"]), _p(a["x"]), _p(a["x0"]),
                                 _p(a["variant"]), _p(a["status"]), _p(a["score"]), _p(a["sel"]), _p(a["A"]), _p(a["b"]),
                                 _p(a["variant_out"]), _p(a["ok"]), _p(a["min_clear"]))
    assert got == rc
    o["_whole"] = whole
    return o


def bands_clean(o, B, K, E, N, n_sel):
    return all(band_clean(o["_whole"][k], fill) for k, (_, _, fill) in out_shapes(B, K, E, N, n_sel).items())


# ------------------------------------------------------------------------------------------------ pools and poses
def box_rows(cx, cy, phi, hl, hw, scale=(1.0, 1.0, 1.0, 1.0)):
    """the four rows of a rectangle (centre, heading, half sizes), consecutive edges, row r scaled by scale[r] > 0"""
    c, s = np.cos(phi), np.sin(phi)
    nrm = np.array([[c, s], [-s, c], [-c, -s], [s, -c]])
    h = np.array([hl, hw, hl, hw])
    A = nrm * np.asarray(scale)[:, None]
    return A, (nrm @ np.array([cx, cy]) + h) * np.asarray(scale)


def random_pool(rng, B, K, E, spread=(2.0, 30.0), yspread=(-8.0, 18.0)):
    """pools of K obstacles of E rows around the corridor the poses of ``random_poses`` run in: E = 4 rotated rectangles,
    E = 2 wedges (two rows 60..120 degrees apart), E = 1 half-planes, every row scaled by a factor in [0.5, 2]"""
    A, b = np.zeros((B, K, E, 2)), np.zeros((B, K, E))
    for i, k in itertools.product(range(B), range(K)):
        cx, cy = rng.uniform(*spread), rng.uniform(*yspread)
        phi = rng.uniform(-np.pi, np.pi)
        Ar, br = box_rows(cx, cy, phi, rng.uniform(0.3, 1.5), rng.uniform(0.3, 1.5), rng.uniform(0.5, 2.0, 4))
        if E == 2:
            psi = phi + rng.uniform(np.pi / 3, 2 * np.pi / 3)
            Ar[1] = (np.cos(psi), np.sin(psi))
            br[1] = Ar[1] @ np.array([cx, cy]) + 0.4
        A[i, k], b[i, k] = Ar[:E], br[:E]
    return A, b


def random_poses(rng, B, N):
    """x [B,3,N+1]: a gently turning track of about 1 m steps starting near (3, 5), and x0 [B,3] next to its first knot"""
    x = np.zeros((B, 3, N + 1))
    for i in range(B):
        th = rng.uniform(-0.4, 0.4)
        p = np.array([rng.uniform(2, 6), rng.uniform(3, 7)])
        for k in range(N + 1):
            x[i, :, k] = (p[0], p[1], th)
            th += rng.uniform(-0.15, 0.15)
            p = p + rng.uniform(0.6, 1.2) * np.array([np.cos(th), np.sin(th)])
    x0 = x[:, :, 0] + rng.uniform(-0.3, 0.3, (B, 3))
    return x, x0


def rows_at(pool_A, pool_b, pool_v, Ts, kk):
    """numpy restatement of the moving rows: b_kk = b + (kk * Ts) * (A0 v_x + A1 v_y), one rounding per operation"""
    if pool_v is None:
        return pool_b.copy()
    t = np.float64(kk) * np.asarray(Ts, float)[:, None, None]
    dot = pool_A[..., 0] * pool_v[:, :, None, 0] + pool_A[..., 1] * pool_v[:, :, None, 1]
    return pool_b + t * dot


def numpy_score(pool_A, pool_b, x, pool_v=None, Ts=None, x0=None, variant=6, n_sub=1, ego=EGO):
    """[B,K]: smallest kkt_check.polytope_distance over x0 and the n_sub + 1 samples of every interval (pose and b
    interpolated linearly at j / n_sub, the knots taken as they are); a pose that is not finite is skipped"""
    B, K, E = pool_b.shape
    N = x.shape[2] - 1
    var = np.broadcast_to(np.asarray(variant), (B,))
    stage = [rows_at(pool_A, pool_b, pool_v, Ts, kk) for kk in range(N + 1)]
    out = np.full((B, K), np.inf)
    for i in range(B):
        bk = lambda kk: stage[0 if var[i] == 4 else kk][i]
        samples = [] if x0 is None else [(x0[i], bk(0))]
        for s in range(N):
            for j in range(0 if s == 0 else 1, n_sub + 1):
                t = j / n_sub
                pose = x[i, :, s] if j == 0 else (x[i, :, s + 1] if j == n_sub else x[i, :, s] + t * (x[i, :, s + 1] - x[i, :, s]))
                bb = bk(s) if j == 0 else (bk(s + 1) if j == n_sub else bk(s) + t * (bk(s + 1) - bk(s)))
                samples.append((pose, bb))
        for pose, bb in samples:
            if not np.all(np.isfinite(pose)):
                continue
            car = kkt_check.car_corners(pose, ego)
            for k in range(K):
                out[i, k] = min(out[i, k], kkt_check.polytope_distance(car, pool_A[i, k], bb[k]))
    return out


def numpy_select(score, n_sel):
    """ascending pool indices of the n_sel smallest scores, ties to the lower index"""
    idx = np.arange(score.shape[1])
    return np.stack([np.sort(np.lexsort((idx, s))[:n_sel]) for s in score]).astype(np.int32)


def numpy_gather(pool_A, pool_b, sel, N, pool_v=None, Ts=None):
    B, K, E = pool_b.shape
    n_sel = sel.shape[1]
    bi = np.arange(B)[:, None]
    A = np.stack([pool_A[bi, sel].reshape(B, n_sel * E, 2)] * (N + 1), axis=1)
    b = np.stack([rows_at(pool_A, pool_b, pool_v, Ts, kk)[bi, sel].reshape(B, n_sel * E) for kk in range(N + 1)], axis=1)
    return A, b


# ------------------------------------------------------------------------------------------------ score
@pytest.mark.parametrize("E", [1, 2, 4])
def test_score_matches_numpy(host, E):
    """static and moving pools, variant 4 against 6, n_sub 1 and 5, x0 given and not; instance 1 has a pose that is not
    finite at knot 1, which drops that knot and the interior samples on either side of it"""
    rng = np.random.default_rng(100 + E)
    B, K, N = 2, 5, 3
    pool_A, pool_b = random_pool(rng, B, K, E, (1.0, 11.0), (1.0, 9.0))      # next to the track and across it
    x, x0 = random_poses(rng, B, N)
    x0[:, :2] += (-0.8, 0.6)
    x[1, 1, 1] = np.nan
    v, Ts = rng.uniform(-0.5, 0.5, (B, K, 2)), rng.uniform(0.5, 1.5, B)
    for moving, variant, n_sub, with_x0 in itertools.product((False, True), (4, 6), (1, 5), (False, True)):
        kw = dict(pool_v=v if moving else None, Ts=Ts if moving else None, x0=x0 if with_x0 else None, n_sub=n_sub)
        o = host_select(host, pool_A, pool_b, x, 2, variant=np.full(B, variant, np.int32), **kw)
        ref = numpy_score(pool_A, pool_b, x, variant=variant, **kw)
        assert np.max(np.abs(o["score"] - ref)) < SCORE_TOL
        assert np.all(o["ok"] == 1) and np.all(o["variant_out"] == variant)
        assert np.max(np.abs(o["min_clear"] - ref.min(axis=1))) < SCORE_TOL
        assert bands_clean(o, B, K, E, N, 2)


def test_every_kind_of_sample_counts(host):
    """a world built so that each option decides the score: one interval from (0, 0) to (8, 0), box 0 beside its midpoint at a
    gap of 0.2 m (seen only between the knots), box 1 at 0.3 m from x0 = (4, -5) and 5 m from the track, box 0 moving away
    at 1 m/s (seen only where stage 1 has rows of its own)"""
    rows = [box_rows(4.0, 0.75 + 0.5 + 0.2, 0.0, 0.5, 0.5), box_rows(4.0, -5.0 - 0.75 - 0.5 - 0.3, 0.0, 0.5, 0.5)]
    pool_A, pool_b = np.stack([r[0] for r in rows])[None], np.stack([r[1] for r in rows])[None]
    x = np.array([[[0.0, 8.0], [0.0, 0.0], [0.0, 0.0]]])
    x0 = np.array([[4.0, -5.0, 0.0]])
    v, Ts = np.array([[[0.0, 1.0], [0.0, 0.0]]]), np.array([1.0])
    corner = np.hypot(3.5 - 1.7, 0.2)                            # knots only: corner of the car to corner of box 0
    sc = lambda **kw: host_select(host, pool_A, pool_b, x, 1, **kw)["score"][0]
    assert np.max(np.abs(sc() - [corner, np.hypot(3.5 - 1.7, 5.3)])) < SCORE_TOL
    assert np.max(np.abs(sc(n_sub=2) - [0.2, 5.3])) < SCORE_TOL
    assert np.max(np.abs(sc(n_sub=2, x0=x0) - [0.2, 0.3])) < SCORE_TOL
    mv = dict(pool_v=v, Ts=Ts, n_sub=2)
    assert np.max(np.abs(sc(variant=np.array([6], np.int32), **mv) - [0.7, 5.3])) < SCORE_TOL      # half a step away at t = 1/2
    assert np.max(np.abs(sc(variant=np.array([4], np.int32), **mv) - [0.2, 5.3])) < SCORE_TOL


def test_moving_rows_words(host):
    """b_kk against numpy with the same operations in the same order: equal words, in the core function and in the gather"""
    rng = np.random.default_rng(7)
    B, K, E, N = 3, 6, 4, 9
    pool_A, pool_b = random_pool(rng, B, K, E)
    x, _ = random_poses(rng, B, N)
    v, Ts = rng.uniform(-2, 2, (B, K, 2)), rng.uniform(0.05, 1.7, B)
    for kk in (0, 1, 7):
        ref = rows_at(pool_A, pool_b, v, Ts, kk)
        for r in range(E):
            got = host.scene_row_b_host(_p(pool_A[1, 2]), _p(pool_b[1, 2]), _p(v[1, 2]), Ts[1], r, kk)
            assert np.float64(got).view(np.uint64) == ref[1, 2, r].view(np.uint64)
    o = host_select(host, pool_A, pool_b, x, 3, pool_v=v, Ts=Ts)
    A, b = numpy_gather(pool_A, pool_b, o["sel"], N, v, Ts)
    assert np.array_equal(words(o["A"]), words(A)) and np.array_equal(words(o["b"]), words(b))
    assert np.any(b[:, 0] != b[:, N])
    # without velocities the rows are the pool's own words at every stage
    o = host_select(host, pool_A, pool_b, x, 3)
    A, b = numpy_gather(pool_A, pool_b, o["sel"], N)
    assert np.array_equal(words(o["A"]), words(A)) and np.array_equal(words(o["b"]), words(b))


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("K,n_sel", [(1, 1), (5, 2), (5, 5), (64, 1), (64, 8), (8, 8)])
def test_selection_matches_lexsort(host, K, n_sel):
    """pools with repeated obstacles (equal scores to the last bit): ties go to the lower pool index, sel is ascending, the
    gather is fancy indexing"""
    rng = np.random.default_rng(1000 + 10 * K + n_sel)
    B, E, N = 4, 4, 2
    pool_A, pool_b = random_pool(rng, B, K, E)
    for k in range(1, K, 3):                                     # every third obstacle repeats its predecessor
        pool_A[:, k], pool_b[:, k] = pool_A[:, k - 1], pool_b[:, k - 1]
    x, x0 = random_poses(rng, B, N)
    o = host_select(host, pool_A, pool_b, x, n_sel, x0=x0, n_sub=2)
    if K > 1:
        assert np.any(o["score"][:, 1] == o["score"][:, 0])
    sel = numpy_select(o["score"], n_sel)
    assert np.array_equal(o["sel"], sel)
    assert np.all(np.diff(o["sel"], axis=1) > 0)
    A, b = numpy_gather(pool_A, pool_b, sel, N)
    assert np.array_equal(words(o["A"]), words(A)) and np.array_equal(words(o["b"]), words(b))
    assert np.all(o["ok"] == 1) and np.all(o["variant_out"] == 6) and bands_clean(o, B, K, E, N, n_sel)


# ------------------------------------------------------------------------------------------------ the loop's mechanics
def scripted_world():
    """B = 4 copies of one world: the reference runs along y = 0 from x = 0 to 5 (N = 5); six unit boxes at x = 2.5, five above
    the car at gaps 1, 2, 3, 4, 6 m (pool indices 0, 1, 2, 3, 5) and index 4 below it at a gap of 5 m"""
    B, N = 4, 5
    gaps = [1.0, 2.0, 3.0, 4.0, -5.0, 6.0]
    rows = [box_rows(2.5, np.sign(g) * (0.75 + 0.5 + abs(g)), 0.0, 0.5, 0.5) for g in gaps]
    pool_A = np.stack([np.stack([r[0] for r in rows])] * B)
    pool_b = np.stack([np.stack([r[1] for r in rows])] * B)
    xref = np.zeros((B, 3, N + 1))
    xref[:, 0] = np.arange(N + 1.0)
    return pool_A, pool_b, xref


def test_loop_mechanics_with_scripted_plans(host):
    pool_A, pool_b, xref = scripted_world()
    B, K, N = 4, 6, 5
    var = np.array([6, 6, 6, 0], np.int32)
    s0 = host_select(host, pool_A, pool_b, xref, 3, variant=var)
    assert np.array_equal(s0["sel"], np.tile([0, 1, 2], (B, 1))) and np.array_equal(s0["variant_out"], var)
    assert np.max(np.abs(s0["score"] - np.tile([1, 2, 3, 4, 5, 6.0], (B, 1)))) < SCORE_TOL
    # the "plans": instances 0, 2, 3 pass 0.1 m from obstacle 4 (left out in round 0), instance 1 follows the reference
    plan = xref.copy()
    plan[[0, 2, 3], 1] = -4.9
    status = np.array([0, 1, 3, 0], np.int32)
    s1 = host_select(host, pool_A, pool_b, plan, 3, variant=var, status=status, state=(s0["score"], s0["sel"]))
    assert np.array_equal(s1["sel"][0], [0, 1, 4])               # obstacle 4 comes in, 2 (the farthest selected) drops out
    assert np.array_equal(s1["sel"][1:], np.tile([0, 1, 2], (3, 1)))
    assert np.array_equal(s1["variant_out"], [6, 0, 0, 0]) and np.all(s1["ok"] == 1)
    assert np.max(np.abs(s1["score"][0] - [1, 2, 3, 4, 0.1, 6])) < SCORE_TOL
    assert np.array_equal(words(s1["score"][1:]), words(s0["score"][1:]))     # followed the reference / not measured
    assert np.max(np.abs(s1["min_clear"][:2] - [0.1, 1.0])) < SCORE_TOL and np.all(np.isnan(s1["min_clear"][2:]))
    A, b = numpy_gather(pool_A, pool_b, s1["sel"], N)
    assert np.array_equal(words(s1["A"]), words(A)) and np.array_equal(words(s1["b"]), words(b))
    # min_clear is this call's minimum, not the running one: back on the reference instance 0 measures 1 m again
    s2 = host_select(host, pool_A, pool_b, xref, 3, variant=var, status=status, state=(s1["score"], s1["sel"]))
    assert abs(s2["min_clear"][0] - 1.0) < SCORE_TOL and np.array_equal(words(s2["score"]), words(s1["score"]))
    # a second identical call changes nothing
    s3 = host_select(host, pool_A, pool_b, plan, 3, variant=var, status=status, state=(s1["score"], s1["sel"]))
    assert np.all(s3["variant_out"] == 0)
    for k in ("score", "sel", "A", "b", "ok"):
        assert np.array_equal(s3[k], s1[k])
    assert np.array_equal(words(s3["min_clear"]), words(s1["min_clear"])) and bands_clean(s3, B, K, 4, N, 3)


# ------------------------------------------------------------------------------------------------ unusable instances
def _spoil(cause, pool_A, pool_b, pool_v, Ts, x, x0):
    if cause == "pool_A nan":
        pool_A[1, 3, 2, 1] = np.nan
    elif cause == "pool_b inf":
        pool_b[1, 0, 0] = np.inf
    elif cause == "zero row":
        pool_A[1, 4, 1] = 0.0
    elif cause == "velocity nan":
        pool_v[1, 2, 0] = np.nan
    elif cause == "Ts inf":
        Ts[1] = -np.inf
    elif cause == "no finite pose":
        x[1, 0] = np.nan
        x0[1, 2] = np.inf


@pytest.mark.parametrize("cause", ["pool_A nan", "pool_b inf", "zero row", "velocity nan", "Ts inf", "no finite pose"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_unusable_instance(host, cause, accumulate):
    rng = np.random.default_rng(31)
    B, K, E, N, n_sel = 3, 6, 4, 4, 3
    pool_A, pool_b = random_pool(rng, B, K, E)
    x, x0 = random_poses(rng, B, N)
    v, Ts = rng.uniform(-0.5, 0.5, (B, K, 2)), rng.uniform(0.5, 1.5, B)
    good = host_select(host, pool_A, pool_b, x, n_sel, pool_v=v, Ts=Ts, x0=x0, n_sub=3)
    _spoil(cause, pool_A, pool_b, v, Ts, x, x0)
    state = None
    if accumulate:
        state = (good["score"].copy(), np.tile(np.array([1, 3, 5], np.int32), (B, 1)))
        state[0][1] = FILL_X
    o = host_select(host, pool_A, pool_b, x, n_sel, pool_v=v, Ts=Ts, x0=x0, n_sub=3, state=state)
    assert list(o["ok"]) == [1, 0, 1] and o["variant_out"][1] == 0
    assert np.array_equal(o["sel"][1], [0, 1, 2]) and np.all(o["score"][1] == FILL_X)
    assert np.all(o["A"][1] == [1.0, 0.0]) and np.all(o["b"][1] == FILL_B) and np.isnan(o["min_clear"][1])
    for k in ("A", "b", "sel", "variant_out", "ok"):
        assert not np.any(np.isnan(np.asarray(o[k], float)))
    assert not np.any(np.isnan(o["score"][[0, 2]]))
    for i in (0, 2):                                             # the neighbours are as good as without the spoilt one
        assert np.array_equal(o["sel"][i], good["sel"][i]) and np.array_equal(words(o["A"][i]), words(good["A"][i]))
    assert bands_clean(o, B, K, E, N, n_sel)


def test_selection_passed_in_must_be_a_selection(host):
    """accumulate, an instance that is not measured (status 2) keeps its selection -- unless that is no ascending list of pool
    indices, which would index outside the pool: then the instance is unusable"""
    rng = np.random.default_rng(32)
    B, K, E, N, n_sel = 4, 6, 2, 3, 3
    pool_A, pool_b = random_pool(rng, B, K, E)
    x, _ = random_poses(rng, B, N)
    score = rng.uniform(0, 5, (B, K))
    sel = np.array([[1, 2, 4], [0, 2, 6], [3, 2, 5], [-1, 0, 1]], np.int32)
    o = host_select(host, pool_A, pool_b, x, n_sel, status=np.full(B, 2, np.int32), state=(score, sel))
    assert list(o["ok"]) == [1, 0, 0, 0] and np.all(o["variant_out"] == 0)
    assert np.array_equal(o["sel"], [[1, 2, 4], [0, 1, 2], [0, 1, 2], [0, 1, 2]])
    assert np.array_equal(words(o["score"]), words(score)) and np.all(np.isnan(o["min_clear"]))
    A, b = numpy_gather(pool_A, pool_b, sel[:1], N)
    assert np.array_equal(words(o["A"][:1]), words(A[:1])) and np.array_equal(words(o["b"][:1]), words(b[:1]))
    assert np.all(o["A"][1:] == [1.0, 0.0]) and np.all(o["b"][1:] == FILL_B)


# ------------------------------------------------------------------------------------------------ refusals
REFUSED = [dict(over=dict(B=0)), dict(over=dict(K=0)), dict(over=dict(K=65)), dict(over=dict(E=0)), dict(over=dict(E=5)),
           dict(over=dict(N=0)), dict(over=dict(N=128)), dict(over=dict(n_sel=0)), dict(over=dict(n_sel=9)),
           dict(over=dict(n_sel=7)), dict(over=dict(n_sub=0)), dict(over=dict(n_sub=257)), dict(over=dict(accumulate=2)),
           dict(over=dict(accumulate=-1)), dict(null=("Ts",)), dict(ego=(1.7, np.nan, 1.7, 0.75)), dict(ego=(np.inf, 0.75, 1.7, 0.75))] + \
          [dict(null=(k,)) for k in ("ego", "pool_A", "pool_b", "x", "score", "sel", "A", "b", "variant_out", "ok")]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: repr(c.get("over") or c.get("null") or c.get("ego")))
def test_refused_calls_touch_nothing(host, case):
    rng = np.random.default_rng(33)
    B, K, E, N, n_sel = 2, 6, 4, 3, 3                           # n_sel = 7 > K = 6
    pool_A, pool_b = random_pool(rng, B, K, E)
    x, x0 = random_poses(rng, B, N)
    v, Ts = rng.uniform(-0.5, 0.5, (B, K, 2)), rng.uniform(0.5, 1.5, B)
    o = host_select(host, pool_A, pool_b, x, n_sel, pool_v=v, Ts=Ts, x0=x0, rc=E_INVAL, **case)
    for k, (_, _, fill) in out_shapes(B, K, E, N, n_sel).items():
        assert np.all(o["_whole"][k] == fill), k


def test_misaligned_rows_are_refused(host):
    """A_out takes one 16-byte store per row"""
    rng = np.random.default_rng(34)
    B, K, E, N, n_sel = 2, 6, 4, 3, 3
    pool_A, pool_b = random_pool(rng, B, K, E)
    x, _ = random_poses(rng, B, N)
    shapes = out_shapes(B, K, E, N, n_sel)
    bufs = {k: np.full(int(np.prod(s)) + 3, fill, dt) for k, (s, dt, fill) in shapes.items()}
    a0 = bufs["A"].ctypes.data
    A_odd = bufs["A"][(1 if a0 % 16 == 0 else 0):]
    assert A_odd.ctypes.data % 16 == 8
    ego = np.ascontiguousarray(EGO, float)
    rc = host.scene_select_host(_p(ego), B, K, E, N, n_sel, 1, 0, _p(pool_A), _p(pool_b), None, None, _p(x), None, None, None,
                                _p(bufs["score"]), _p(bufs["sel"]), _p(A_odd), _p(bufs["b"]), _p(bufs["variant_out"]),
                                _p(bufs["ok"]), _p(bufs["min_clear"]))
    assert rc == E_INVAL
    for k, (_, _, fill) in shapes.items():
        assert np.all(bufs[k] == fill)
