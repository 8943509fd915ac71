"""CPU tier of the staged scene-pool selection (csrc/obca_scene_core.h: the functions of obca_scene_select_staged), built for
the host from tests/native/staged_select_host.cpp.

Yardsticks.  Two identities carry most of the weight, both WORD FOR WORD against tests/test_scene_core.py's ``host_select``
(obca_scene_select's host build): with no staged slot (Kt = 0, or every stage_ok 0) every output is obca_scene_select's; and a
track that holds obca_scene_select's own stage rows (the pool's A at every stage, b from ``tsc.rows_at``, the words of
scene::row_b) gives the pool-velocity outputs, whatever pool_v the staged slots carry.  A track that turns has no such twin:
its score is held to a numpy restatement (rows interpolated entry by entry, tests/kkt_check.py's ``polytope_distance``, which
normalises each row) within ``tsc.SCORE_TOL`` = 1e-12 m, derived there for coordinates below 100 m; the worlds here are the
same corridor.  Selection and gather are exact.  The helpers are shared with tests/test_gpu_fleet_plan.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import kkt_check, native_build, test_scene_core as tsc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "staged_select_host.cpp")
E_INVAL = tsc.E_INVAL
_p = tsc._p
words = tsc.words
OUT = ("score", "sel", "A", "b", "variant_out", "ok", "min_clear")


def load_host():
    lib = native_build.build_shim("staged_select_host", [SRC])
    lib.scene_select_staged_host.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def plain():
    return tsc.load_host()


def host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=None, stage_b=None, stage_ok=None, stage_group=1, Kt=None,
                       pool_v=None, Ts=None, x0=None, variant=None, status=None, n_sub=1, state=None, ego=tsc.EGO, rc=0, null=()):
    """scene_select_staged_host on numpy arrays, as ``tsc.host_select``: a dict of the outputs (views into guard-banded buffers;
    ``_whole`` holds the buffers).  Kt is stage_ok's second axis unless told (0 without stage rows)."""
    pool_A, pool_b, x = (np.ascontiguousarray(a, float) for a in (pool_A, pool_b, x))
    B, K, E = pool_b.shape
    N = x.shape[2] - 1
    f = lambda a, dt=float: None if a is None else np.ascontiguousarray(a, dt)
    a = {"ego": np.ascontiguousarray(ego, float), "pool_A": pool_A, "pool_b": pool_b, "pool_v": f(pool_v), "Ts": f(Ts), "x": x,
         "x0": f(x0), "variant": f(variant, np.int32), "status": f(status, np.int32), "stage_A": f(stage_A), "stage_b": f(stage_b),
         "stage_ok": f(stage_ok, np.int32)}
    if Kt is None:
        Kt = 0 if a["stage_ok"] is None else a["stage_ok"].shape[1]
    o, whole = {}, {}
    for k, (shape, dt, fill) in tsc.out_shapes(B, K, E, N, n_sel).items():
        whole[k], o[k] = tsc.banded(shape, dt, fill)
    if state is not None:
        o["score"][...] = state[0]
        o["sel"][...] = state[1]
    a.update(o)
    for k in null:
        a[k] = None
    got = host.scene_select_staged_host(_p(a["ego"]), B, K, E, N, n_sel, n_sub, 0 if state is None else 1, _p(a["pool_A"]),
                                        _p(a["pool_b"]), _p(a["pool_v"]), _p(a["Ts"]), _p(a["x"]), _p(a["x0"]), _p(a["variant"]),
                                        _p(a["status"]), Kt, stage_group, _p(a["stage_A"]), _p(a["stage_b"]), _p(a["stage_ok"]),
                                        _p(a["score"]), _p(a["sel"]), _p(a["A"]), _p(a["b"]), _p(a["variant_out"]), _p(a["ok"]),
                                        _p(a["min_clear"]))
    assert got == rc
    o["_whole"] = whole
    return o


def same_outputs(o, ref):
    return all(np.array_equal(np.ascontiguousarray(o[k]).view(np.uint8), np.ascontiguousarray(ref[k]).view(np.uint8)) for k in OUT)


# ------------------------------------------------------------------------------------------------ tracks
def translation_track(pool_A, pool_b, pool_v, Ts, N, Kt):
    """stage_A [B,Kt,N+1,E,2], stage_b [B,Kt,N+1,E] (stage_group 1): obca_scene_select's own stage rows of the last Kt slots --
    A at every stage, b_kk with scene::row_b's words (``tsc.rows_at``; tests/test_scene_core.py shows they are the same)"""
    K = pool_b.shape[1]
    sb = np.stack([tsc.rows_at(pool_A, pool_b, pool_v, Ts, kk)[:, K - Kt:] for kk in range(N + 1)], axis=2)
    sA = np.stack([pool_A[:, K - Kt:]] * (N + 1), axis=2)
    return np.ascontiguousarray(sA), np.ascontiguousarray(sb)


def turning_track(rng, blocks, Kt, N, E=4, turn=0.3):
    """rectangles next to the track of ``tsc.random_poses`` that move about 0.7 m and turn by up to ``turn`` rad per stage;
    rows scaled like ``tsc.random_pool``'s"""
    sA, sb = np.zeros((blocks, Kt, N + 1, E, 2)), np.zeros((blocks, Kt, N + 1, E))
    for i in range(blocks):
        for t in range(Kt):
            c = np.array([rng.uniform(2.0, 14.0), rng.uniform(0.0, 10.0)])
            phi, hl, hw, scale = rng.uniform(-np.pi, np.pi), rng.uniform(0.5, 1.7), rng.uniform(0.3, 0.8), rng.uniform(0.5, 2.0, 4)
            for kk in range(N + 1):
                A, b = tsc.box_rows(c[0], c[1], phi, hl, hw, scale)
                sA[i, t, kk], sb[i, t, kk] = A[:E], b[:E]
                phi += rng.uniform(-turn, turn)
                c = c + rng.uniform(0.3, 1.0) * np.array([np.cos(phi), np.sin(phi)])
    return sA, sb


def numpy_score_staged(pool_A, pool_b, x, stage_A, stage_b, stage_ok, stage_group=1, pool_v=None, Ts=None, x0=None, variant=6,
                       n_sub=1, ego=tsc.EGO):
    """[B,K]: ``tsc.numpy_score`` with the staged slots replaced: x0 against stage 0, per interval the n_sub + 1 samples with A
    and b interpolated entry by entry at j / n_sub (the knots' own rows at the ends), variant 4: stage 0 at every sample"""
    out = tsc.numpy_score(pool_A, pool_b, x, pool_v=pool_v, Ts=Ts, x0=x0, variant=variant, n_sub=n_sub, ego=ego)
    B, K, E = pool_b.shape
    N = x.shape[2] - 1
    Kt = stage_ok.shape[1]
    var = np.broadcast_to(np.asarray(variant), (B,))
    for i in range(B):
        for t in range(Kt):
            if stage_ok[i, t] == 0:
                continue
            sA, sb = stage_A[i // stage_group, t], stage_b[i // stage_group, t]
            st = (lambda kk: (sA[0], sb[0])) if var[i] == 4 else (lambda kk: (sA[kk], sb[kk]))
            samples = [] if x0 is None else [(x0[i],) + st(0)]
            for s in range(N):
                (A0, b0), (A1, b1) = st(s), st(s + 1)
                for j in range(0 if s == 0 else 1, n_sub + 1):
                    u = j / n_sub
                    pose = x[i, :, s] if j == 0 else (x[i, :, s + 1] if j == n_sub else x[i, :, s] + u * (x[i, :, s + 1] - x[i, :, s]))
                    Aj = A0 if j == 0 else (A1 if j == n_sub else A0 + u * (A1 - A0))
                    bj = b0 if j == 0 else (b1 if j == n_sub else b0 + u * (b1 - b0))
                    samples.append((pose, Aj, bj))
            best = np.inf
            for pose, Aj, bj in samples:
                if np.all(np.isfinite(pose)):
                    best = min(best, kkt_check.polytope_distance(kkt_check.car_corners(pose, ego), Aj, bj))
            out[i, K - Kt + t] = best
    return out


def numpy_gather_staged(pool_A, pool_b, sel, N, stage_A, stage_b, stage_ok, stage_group=1, pool_v=None, Ts=None):
    A, b = tsc.numpy_gather(pool_A, pool_b, sel, N, pool_v, Ts)
    B, K, E = pool_b.shape
    Kt = stage_ok.shape[1]
    for i in range(B):
        for slot, k in enumerate(sel[i]):
            t = k - (K - Kt)
            if t >= 0 and stage_ok[i, t] != 0:
                A[i, :, slot * E:(slot + 1) * E] = stage_A[i // stage_group, t]
                b[i, :, slot * E:(slot + 1) * E] = stage_b[i // stage_group, t]
    return A, b


def world(rng, B, K, E, N):
    pool_A, pool_b = tsc.random_pool(rng, B, K, E, (1.0, 11.0), (1.0, 9.0))
    x, x0 = tsc.random_poses(rng, B, N)
    return pool_A, pool_b, x, x0, rng.uniform(-0.5, 0.5, (B, K, 2)), rng.uniform(0.5, 1.5, B)


# ------------------------------------------------------------------------------------------------ the two identities
@pytest.mark.parametrize("K,Kt", [(5, 0), (5, 2), (5, 5), (64, 16), (1, 1)])
def test_without_a_staged_slot_it_is_select_word_for_word(host, plain, K, Kt):
    """Kt = 0 with NULL stage pointers, and Kt > 0 with every stage_ok 0 over tracks full of NaN (never read): every output of
    both accumulate modes equals obca_scene_select's host build"""
    rng = np.random.default_rng(200 + K + Kt)
    B, E, N, n_sel = 3, 4, 4, min(3, K)
    pool_A, pool_b, x, x0, v, Ts = world(rng, B, K, E, N)
    kw = dict(pool_v=v, Ts=Ts, x0=x0, n_sub=3, variant=np.array([8, 4, 8], np.int32))
    st = {} if Kt == 0 else dict(stage_A=np.full((B, Kt, N + 1, E, 2), np.nan), stage_b=np.full((B, Kt, N + 1, E), np.nan),
                                 stage_ok=np.zeros((B, Kt), np.int32))
    ref = tsc.host_select(plain, pool_A, pool_b, x, n_sel, **kw)
    o = host_select_staged(host, pool_A, pool_b, x, n_sel, **st, **kw)
    assert same_outputs(o, ref) and tsc.bands_clean(o, B, K, E, N, n_sel)
    plan = x + rng.uniform(-0.5, 0.5, x.shape)
    status = np.array([0, 1, 2], np.int32)
    ref2 = tsc.host_select(plain, pool_A, pool_b, plan, n_sel, status=status, state=(ref["score"], ref["sel"]), **kw)
    o2 = host_select_staged(host, pool_A, pool_b, plan, n_sel, status=status, state=(o["score"], o["sel"]), **st, **kw)
    assert same_outputs(o2, ref2) and tsc.bands_clean(o2, B, K, E, N, n_sel)


@pytest.mark.parametrize("E", [1, 2, 3, 4])
@pytest.mark.parametrize("K,Kt", [(6, 2), (6, 6), (64, 16)])
def test_a_translation_track_is_the_pool_velocity_word_for_word(host, plain, E, K, Kt):
    """the track holds obca_scene_select's own stage rows of the last Kt slots; the staged call gets OTHER velocities for those
    slots (they play no part) and must give the plain call's outputs: n_sub 1 and 5, with and without x0, variant 4 beside 8,
    both accumulate modes"""
    rng = np.random.default_rng(300 + 10 * E + K + Kt)
    B, N, n_sel = 3, 4, 3
    pool_A, pool_b, x, x0, v, Ts = world(rng, B, K, E, N)
    sA, sb = translation_track(pool_A, pool_b, v, Ts, N, Kt)
    v_other = v.copy()
    v_other[:, K - Kt:] = rng.uniform(-2, 2, (B, Kt, 2))
    ok = np.ones((B, Kt), np.int32)
    ok[2, 0] = 0                                                   # one slot falls back to its pool row and velocity
    v_other[2, K - Kt] = v[2, K - Kt]
    var = np.array([8, 4, 8], np.int32)
    for n_sub in (1, 5):
        for with_x0 in (False, True):
            kw = dict(Ts=Ts, x0=x0 if with_x0 else None, n_sub=n_sub, variant=var)
            ref = tsc.host_select(plain, pool_A, pool_b, x, n_sel, pool_v=v, **kw)
            o = host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=sA, stage_b=sb, stage_ok=ok, pool_v=v_other, **kw)
            assert same_outputs(o, ref), (n_sub, with_x0)
            plan = x + rng.uniform(-0.5, 0.5, x.shape)
            status = np.array([0, 2, 1], np.int32)
            ref2 = tsc.host_select(plain, pool_A, pool_b, plan, n_sel, pool_v=v, status=status, state=(ref["score"], ref["sel"]), **kw)
            o2 = host_select_staged(host, pool_A, pool_b, plan, n_sel, stage_A=sA, stage_b=sb, stage_ok=ok, pool_v=v_other,
                                    status=status, state=(o["score"], o["sel"]), **kw)
            assert same_outputs(o2, ref2) and tsc.bands_clean(o2, B, K, E, N, n_sel)
    assert np.any(ref["b"][:, 0] != ref["b"][:, N])


# ------------------------------------------------------------------------------------------------ tracks that turn
@pytest.mark.parametrize("E", [1, 2, 4])
def test_a_turning_track_matches_numpy(host, E):
    """scores and min_clear against the numpy restatement, selection against lexsort of the host's scores, the gather the
    stage rows as they are; Kt = K and Kt < K, n_sub 1 and 5, variant 4 beside 8, x0 given and not"""
    rng = np.random.default_rng(400 + E)
    B, K, N, n_sel = 3, 5, 4, 2
    pool_A, pool_b, x, x0, v, Ts = world(rng, B, K, E, N)
    var = np.array([8, 4, 8], np.int32)
    for Kt in (2, K):
        sA, sb = turning_track(rng, B, Kt, N, E)
        ok = np.ones((B, Kt), np.int32)
        ok[1, Kt - 1] = 0
        for n_sub in (1, 5):
            for with_x0 in (False, True):
                kw = dict(pool_v=v, Ts=Ts, x0=x0 if with_x0 else None, n_sub=n_sub, variant=var)
                o = host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=sA, stage_b=sb, stage_ok=ok, **kw)
                ref = numpy_score_staged(pool_A, pool_b, x, sA, sb, ok, **kw)
                assert np.max(np.abs(o["score"] - ref)) < tsc.SCORE_TOL
                assert np.max(np.abs(o["min_clear"] - ref.min(axis=1))) < tsc.SCORE_TOL
                assert np.all(o["ok"] == 1) and np.array_equal(o["variant_out"], var)
                sel = tsc.numpy_select(o["score"], n_sel)
                assert np.array_equal(o["sel"], sel)
                A, b = numpy_gather_staged(pool_A, pool_b, sel, N, sA, sb, ok, pool_v=v, Ts=Ts)
                assert np.array_equal(words(o["A"]), words(A)) and np.array_equal(words(o["b"]), words(b))
                assert tsc.bands_clean(o, B, K, E, N, n_sel)
    # variant 4 reads stage 0 everywhere: instance 1's scores do not change when the later stages do
    sA2, sb2 = sA.copy(), sb.copy()
    sb2[:, :, 1:] += 3.0
    o2 = host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=sA2, stage_b=sb2, stage_ok=ok, **kw)
    assert np.array_equal(words(o2["score"][1]), words(o["score"][1])) and not np.array_equal(words(o2["score"][0]), words(o["score"][0]))


def cut_in_pool():
    """the reference runs along y = 0 from x = 0 to 5 (N = 5); three unit boxes above it at gaps 3, 4 and 5 m and, as the last
    slot, a unit box 12 m above it that stands still as a pool obstacle -- and whose track comes down 2.5 m per stage and
    ends 0.5 m above the car's strip at stage 4"""
    N = 5
    rows = [tsc.box_rows(2.5, 0.75 + 0.5 + g, 0.0, 0.5, 0.5) for g in (3.0, 4.0, 5.0, 12.0)]
    pool_A, pool_b = np.stack([r[0] for r in rows])[None], np.stack([r[1] for r in rows])[None]
    x = np.zeros((1, 3, N + 1))
    x[0, 0] = np.arange(N + 1.0)
    track = [tsc.box_rows(2.5, 0.75 + 0.5 + max(12.0 - 2.875 * kk, 0.5), 0.0, 0.5, 0.5) for kk in range(N + 1)]
    sA, sb = np.stack([r[0] for r in track])[None, None], np.stack([r[1] for r in track])[None, None]
    return pool_A, pool_b, x, sA, sb


def test_a_staged_slot_is_selected_where_its_pool_rows_are_not(host, plain):
    pool_A, pool_b, x, sA, sb = cut_in_pool()
    v, Ts = np.zeros((1, 4, 2)), np.ones(1)
    ref = tsc.host_select(plain, pool_A, pool_b, x, 1, pool_v=v, Ts=Ts)
    assert list(ref["sel"][0]) == [0] and abs(ref["score"][0, 3] - 12.0) < tsc.SCORE_TOL
    o = host_select_staged(host, pool_A, pool_b, x, 1, stage_A=sA, stage_b=sb, stage_ok=np.ones((1, 1), np.int32), pool_v=v, Ts=Ts)
    assert list(o["sel"][0]) == [3] and abs(o["score"][0, 3] - 0.5) < tsc.SCORE_TOL and abs(o["min_clear"][0] - 0.5) < tsc.SCORE_TOL
    assert np.array_equal(words(o["A"][0]), words(sA[0, 0])) and np.array_equal(words(o["b"][0]), words(sb[0, 0]))
    assert np.array_equal(words(o["score"][0, :3]), words(ref["score"][0, :3]))


def test_instances_of_a_group_share_one_block(host):
    """stage_group = 2: instances 2 g and 2 g + 1 read block g, each under its own stage_ok; the outputs are those of
    stage_group = 1 over the blocks repeated"""
    rng = np.random.default_rng(500)
    B, K, E, N, n_sel, Kt = 4, 5, 4, 3, 2, 3
    pool_A, pool_b, x, x0, v, Ts = world(rng, B, K, E, N)
    sA, sb = turning_track(rng, B // 2, Kt, N, E)
    ok = rng.integers(0, 2, (B, Kt)).astype(np.int32)
    ok[0], ok[1] = (1, 0, 1), (0, 1, 1)
    kw = dict(pool_v=v, Ts=Ts, x0=x0, n_sub=2)
    o = host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=sA, stage_b=sb, stage_ok=ok, stage_group=2, **kw)
    ref = host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=np.repeat(sA, 2, axis=0), stage_b=np.repeat(sb, 2, axis=0),
                             stage_ok=ok, stage_group=1, **kw)
    assert same_outputs(o, ref)
    num = numpy_score_staged(pool_A, pool_b, x, sA, sb, ok, stage_group=2, **kw)
    assert np.max(np.abs(o["score"] - num)) < tsc.SCORE_TOL


def test_accumulate_keeps_the_running_minimum_and_the_selection_of_an_unmeasured_instance(host):
    rng = np.random.default_rng(600)
    B, K, E, N, n_sel, Kt = 3, 5, 4, 4, 2, 2
    pool_A, pool_b, x, x0, v, Ts = world(rng, B, K, E, N)
    sA, sb = turning_track(rng, B, Kt, N, E)
    ok = np.ones((B, Kt), np.int32)
    kw = dict(pool_v=v, Ts=Ts, n_sub=2, stage_A=sA, stage_b=sb, stage_ok=ok)
    first = host_select_staged(host, pool_A, pool_b, x, n_sel, x0=x0, **kw)
    plan = x + rng.uniform(-0.8, 0.8, x.shape)
    status = np.array([0, 1, 2], np.int32)
    sel_in = first["sel"].copy()
    sel_in[2] = (1, 4)                                             # instance 2 is not measured: it keeps what it is given
    o = host_select_staged(host, pool_A, pool_b, plan, n_sel, status=status, state=(first["score"], sel_in), **kw)
    cur = numpy_score_staged(pool_A, pool_b, plan, sA, sb, ok, pool_v=v, Ts=Ts, n_sub=2)
    want = np.minimum(first["score"], cur)
    assert np.max(np.abs(o["score"][:2] - want[:2])) < tsc.SCORE_TOL
    assert np.array_equal(words(o["score"][2]), words(first["score"][2])) and np.isnan(o["min_clear"][2])
    assert np.max(np.abs(o["min_clear"][:2] - cur[:2].min(axis=1))) < tsc.SCORE_TOL
    sel = tsc.numpy_select(o["score"], n_sel)
    assert np.array_equal(o["sel"][:2], sel[:2]) and list(o["sel"][2]) == [1, 4] and o["variant_out"][2] == 0
    assert np.array_equal(o["variant_out"][:2] != 0, np.any(sel[:2] != first["sel"][:2], axis=1))
    A, b = numpy_gather_staged(pool_A, pool_b, o["sel"], N, sA, sb, ok, pool_v=v, Ts=Ts)       # slot 4 of instance 2: its track
    assert np.array_equal(words(o["A"]), words(A)) and np.array_equal(words(o["b"]), words(b)) and np.all(o["ok"] == 1)


# ------------------------------------------------------------------------------------------------ unusable instances
@pytest.mark.parametrize("cause", ["stage_A nan", "stage_b inf in the last stage", "zero row in one stage"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_new_unusable_causes(host, cause, accumulate):
    """a staged row word that is not finite, a staged row a = (0, 0) at one stage: instance 1 gets obca_scene_select's fill;
    the same words under stage_ok == 0 are never read"""
    rng = np.random.default_rng(700)
    B, K, E, N, n_sel, Kt = 3, 6, 4, 4, 3, 2
    pool_A, pool_b, x, x0, v, Ts = world(rng, B, K, E, N)
    sA, sb = turning_track(rng, B, Kt, N, E)
    ok = np.ones((B, Kt), np.int32)
    kw = dict(pool_v=v, Ts=Ts, x0=x0, n_sub=3)
    good = host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=sA, stage_b=sb, stage_ok=ok, **kw)
    if cause == "stage_A nan":
        sA[1, 1, 2, 3, 0] = np.nan
    elif cause == "stage_b inf in the last stage":
        sb[1, 0, N, 1] = np.inf
    else:
        sA[1, 1, 3, 2] = 0.0
    state = None
    if accumulate:
        state = (good["score"].copy(), np.tile(np.array([1, 3, 5], np.int32), (B, 1)))
        state[0][1] = tsc.FILL_X
    o = host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=sA, stage_b=sb, stage_ok=ok, state=state, **kw)
    assert list(o["ok"]) == [1, 0, 1] and o["variant_out"][1] == 0
    assert np.array_equal(o["sel"][1], [0, 1, 2]) and np.all(o["score"][1] == tsc.FILL_X)
    assert np.all(o["A"][1] == [1.0, 0.0]) and np.all(o["b"][1] == tsc.FILL_B) and np.isnan(o["min_clear"][1])
    for k in ("A", "b", "sel", "variant_out", "ok"):
        assert not np.any(np.isnan(np.asarray(o[k], float)))
    for i in (0, 2):
        assert np.array_equal(o["sel"][i], good["sel"][i]) and np.array_equal(words(o["A"][i]), words(good["A"][i]))
    assert tsc.bands_clean(o, B, K, E, N, n_sel)
    ok[1] = 0                                                      # not staged: the spoilt track is not read
    o = host_select_staged(host, pool_A, pool_b, x, n_sel, stage_A=sA, stage_b=sb, stage_ok=ok, state=state, **kw)
    assert list(o["ok"]) == [1, 1, 1]


# ------------------------------------------------------------------------------------------------ refusals
REFUSED = [dict(Kt=-1), dict(Kt=7), dict(stage_group=0), dict(stage_group=-1), dict(stage_group=3), dict(null=("stage_A",)),
           dict(null=("stage_b",)), dict(null=("stage_ok",)), dict(null=("score",)), dict(null=("pool_A",)), dict(n_sub=0)]


@pytest.mark.parametrize("case", REFUSED, ids=repr)
def test_refused_calls_touch_nothing(host, case):
    rng = np.random.default_rng(800)
    B, K, E, N, n_sel, Kt = 4, 6, 4, 3, 3, 2                    # Kt = 7 > K = 6; stage_group = 3 does not divide B = 4
    pool_A, pool_b, x, x0, v, Ts = world(rng, B, K, E, N)
    sA, sb = turning_track(rng, B, Kt, N, E)
    kw = dict(stage_A=sA, stage_b=sb, stage_ok=np.ones((B, Kt), np.int32), pool_v=v, Ts=Ts, x0=x0)
    kw.update(case)
    o = host_select_staged(host, pool_A, pool_b, x, n_sel, rc=E_INVAL, **kw)
    for k, (_, _, fill) in tsc.out_shapes(B, K, E, N, n_sel).items():
        assert np.all(o["_whole"][k] == fill), k
