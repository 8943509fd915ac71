"""obca_set_warm_start (include/obca_mpc.h) on the host build of the lane-per-instance core (csrc/obca_lpi_core.h, through
lpi_host_solve_batch_warm of tests/native/lpi_host.cpp) against numpy: what a solve stores, where a warm solve starts -- the stored
vector moved one stage forward, restated once in tests/warm_case.py:shift -- and where the warm start sits in the start ladder.
Solves that must agree iterate for iterate are cut off after K iterations: both sides then hold the K-th iterate of the same path,
and a start from another point is of order 1 away (measured: 0.74 to 1.13), not of order 1e-12.
Shapes: N = 5; obca_mpc4 with three obstacles (6 rows), obca_mpc6 / obca_mpc8 with five (14 rows); four instances each."""
import numpy as np
import pytest

from oracle import ipm_dense
from tests import warm_case as wc

VARIANTS = (4, 6, 8)
B = 4


@pytest.fixture(scope="module")
def cases():
    """per variant: the batch, its oracle Problems, the stored vectors of a cold solve [B, n_max] with that solve's outputs, and the
    perturbed vectors the truncated solves start from -- computed once, never written by a test"""
    out = {}
    for v in VARIANTS:
        b = wc.batch(v, B)
        ps = wc.problems(b)
        z, cold = wc.stored(b)
        zp = wc.perturbed(z, ps)
        for a in (z, zp):
            a.flags.writeable = False
        out[v] = (b, ps, z, cold, zp)
    return out


def _numpy_pass(p, x_start, K, mu=wc.MU):
    return ipm_dense._solve_once(p, dict(mu_init=mu, max_iter=K), x_start=x_start)


def _diff(got, i, p, r, z=True):
    """largest difference of instance i of the host's outputs from numpy's Result r: poses, inputs, step length and (z) the whole
    primal vector"""
    d = max(np.max(np.abs(got["xopt"][i] - r.xopt)), np.max(np.abs(got["uopt"][i] - r.uopt)), abs(got["ts_opt"][i] - r.Ts_opt))
    return max(d, np.max(np.abs(got["z"][i, :p.n] - r.x))) if z else d


@pytest.mark.parametrize("v", VARIANTS)
def test_store_equals_certificate(cases, v):
    """a solve that ends converged or acceptable stores the words of its certificate vector, L.n of them: the last word of a
    fixed-time row, and the whole row of an instance that is skipped, screened out or not converged, keep the pre-fill"""
    b, ps, z, cold, _ = cases[v]
    assert np.isin(cold["status"], (0, 1)).all()
    for i, p in enumerate(ps):
        assert np.array_equal(z[i, :p.n], cold["z"][i, :p.n]), i
        assert p.n == z.shape[1] - (v != 4)
        if v != 4:
            assert z[i, -1] == wc.SENTINEL and cold["z"][i, -1] == wc.SENTINEL
    # instance 1 skipped; instance 2 of obca_mpc6 with a terminal set 100 m ahead: answered by the screen, without a solve
    var = b["variant"].copy()
    var[1] = 0
    term = b["term"].copy()
    term[2, 0] += 100.0
    zs = np.full_like(z, wc.SENTINEL)
    got = wc.host(dict(b, variant=var, term=term), warm=(zs, np.zeros(B, np.int32), wc.MU))
    assert got["status"][1] == -5 and np.all(zs[1] == wc.SENTINEL)
    if v == 6:
        assert got["status"][2] == 2 and got["iters"][2] == 0 and np.all(zs[2] == wc.SENTINEL)
    for i in (0, 3) + ((2,) if v != 6 else ()):
        assert np.array_equal(zs[i], z[i]), i
    # not converged: one iteration, status -1
    zs = np.full_like(z, wc.SENTINEL)
    got = wc.host(b, warm=(zs, np.zeros(B, np.int32), wc.MU), **wc.truncated(1))
    assert got["status"].tolist() == [-1] * B and np.all(zs == wc.SENTINEL)
    assert np.all(got["z"][:, :ps[0].n] != wc.SENTINEL)                    # (the certificate vector is written all the same)


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("v", VARIANTS)
def test_warm_solve_starts_from_the_shifted_vector(cases, v, K):
    """K iterations from the stored vector: the host core holds numpy's K-th iterate from shift(z) -- measured 3.6e-15 at most at
    K = 1 and 4.2e-13 at K = 3 -- and is 0.74 to 1.13 away from numpy's K-th iterate from the vector as it was stored; the caller's
    buffer is left alone, since nothing converged"""
    b, ps, _, _, zp = cases[v]
    zw = zp.copy()
    got = wc.host(b, warm=(zw, None, wc.MU), **wc.truncated(K))
    assert np.array_equal(zw, zp)
    assert got["status"].tolist() == [-1] * B and got["iters"].tolist() == [K] * B
    for i, p in enumerate(ps):
        r = _numpy_pass(p, wc.shift(p, zp[i]), K)
        assert r.status == -1 and r.iters == K
        d = _diff(got, i, p, r)
        print("variant %d K %d instance %d: host - numpy %.2e" % (v, K, i, d))
        assert d < wc.TOL_SAME_PATH, (i, d)
        unshifted = _numpy_pass(p, zp[i, :p.n], K)
        assert np.max(np.abs(got["z"][i, :p.n] - unshifted.x)) > 1e-3, i


@pytest.mark.parametrize("v", (6, 8))
def test_dodge_passes_after_a_failed_warm_start_keep_its_answer(cases, v):
    """fixed-time solves with the dodge rung on: after the warm pass of one iteration the two (obca_mpc6) or four (obca_mpc8)
    dodge passes run, none ends feasible within one iteration, and the held answer stays the warm pass's"""
    b, _, _, _, zp = cases[v]
    off = wc.host(b, warm=(zp.copy(), None, wc.MU), **wc.truncated(1))
    on = wc.host(b, warm=(zp.copy(), None, wc.MU), **wc.truncated(1, dodge=True))
    assert on["iters"].tolist() == [3 if v == 6 else 5] * B and off["iters"].tolist() == [1] * B
    assert np.array_equal(on["z"], off["z"]) and on["status"].tolist() == [-1] * B
    for k in ("xopt", "uopt", "ts_opt"):
        assert np.array_equal(on[k], off[k]), k


@pytest.mark.parametrize("v", VARIANTS)
def test_stage_constant_vector_gives_the_x0_start(cases, v):
    """every pose x0, everything else 0, time scale 1, barrier parameter 0.1: the shift of that vector is the x0 start, and a warm
    handle keeps x0 first -- the words of a cold solve with start_order "x0\""""
    b, ps, z, _, _ = cases[v]
    zc = wc.stage_constant(ps, z.shape[1])
    warm = wc.host(b, warm=(zc, None, 0.1))
    cold = wc.host(b, start_order="x0")
    for k in wc.KEYS + ("z", "y"):
        assert np.array_equal(warm[k], cold[k]), k
    assert np.isin(cold["status"], (0, 1)).all()


@pytest.mark.parametrize("v", VARIANTS)
def test_use_mask_selects_per_instance(cases, v):
    """use = [1, 0, 1, 0]: the instances with 0 return the words of a solve with no warm buffer at all, those with 1 the words of a
    solve with use = NULL; every converged instance stores its vector, flagged or not"""
    b, ps, _, _, zp = cases[v]
    z_mask, z_all = zp.copy(), zp.copy()
    mask = wc.host(b, warm=(z_mask, np.array([1, 0, 1, 0], np.int32), wc.MU))
    every = wc.host(b, warm=(z_all, None, wc.MU))
    none = wc.host(b)
    for i in range(B):
        want = every if i % 2 == 0 else none
        for k in wc.KEYS + ("z", "y"):
            assert np.array_equal(mask[k][i], want[k][i]), (i, k)
        if mask["status"][i] in (0, 1):
            assert np.array_equal(z_mask[i, :ps[i].n], mask["z"][i, :ps[i].n])
    assert any(not np.array_equal(every["z"][i], none["z"][i]) or every["iters"][i] != none["iters"][i] for i in range(B))


WARM_MU_ORDER = 0.05        # not 0.1: the warm pass's barrier parameter is the caller's, unlike every cold pass's


def _numpy_ladder(p, x_warm, order, pat, ret, mu=WARM_MU_ORDER):
    """ipm_dense.solve's ladder chained by hand with a caller's start in it: the starts of the order one after the other, the first
    ``pat`` iterations at most, the later ones ``ret``; the point ``x_warm`` with barrier parameter ``mu`` stands where the order's
    first cold start stood (x0, or zeros under "zeros").  Returns the held pass and the iterations of all passes."""
    code = ipm_dense.ORDER_NAMES[order] or 3                     # a warm handle keeps x0 first under the default order
    warm_kind = ipm_dense.KIND_ZEROS if code == 2 else ipm_dense.KIND_X0
    held = r = None
    it = 0
    for s, kind in enumerate(ipm_dense.START_ORDERS[code]):
        if r is not None and r.status in (0, 1, ipm_dense.STATUS_BAD_BOUNDS):
            break
        for level in range(1 + len(ipm_dense.RHO_ESCALATION)):
            if level > 0 and not (r.status == ipm_dense.STATUS_INFEASIBLE and p.variant == 4):
                break
            o = dict(rho=ipm_dense.DEFAULTS["rho"] * (ipm_dense.RHO_ESCALATION[level - 1] if level else 1.0), max_iter=pat if s == 0 else ret)
            if kind == warm_kind:
                r = ipm_dense._solve_once(p, dict(o, mu_init=mu), x_start=x_warm)
            elif kind == ipm_dense.KIND_WINDOW:
                r = ipm_dense._solve_once(p, dict(o, mu_init=ipm_dense.RESTART_MU), x_start=ipm_dense.window_start(p))
            else:
                r = ipm_dense._solve_once(p, o, x_start=ipm_dense.x0_start(p) if kind == ipm_dense.KIND_X0 else None)
            it += r.iters
            r.start_index = s
            if ipm_dense._replaces(r, held):
                held = r
    return held, it


@pytest.mark.parametrize("order", ("default", "window", "zeros"))
@pytest.mark.parametrize("v", VARIANTS)
def test_where_the_warm_start_sits_in_the_order(cases, v, order):
    """three starts of two iterations each; no pass converges, so the held answer is the first pass's by ipm_dense's own rule.
    Under "zeros" and under the default order (x0 first on a warm handle) that pass is the warm one, with barrier parameter
    mu_init.  Under "window" it is the cold window pass with RESTART_MU: the case shows only that the warm vector did NOT take
    the first start -- that it takes the second is test_under_window_the_warm_start_is_the_second_start"""
    b, ps, _, _, zp = cases[v]
    got = wc.host(b, warm=(zp.copy(), None, WARM_MU_ORDER), start_order=order, patience=2, retry_iter=2, dodge=False)
    for i, p in enumerate(ps):
        held, it = _numpy_ladder(p, wc.shift(p, zp[i]), order, 2, 2)
        assert got["status"][i] == held.status and got["iters"][i] == it, (i, got["status"][i], held.status, got["iters"][i], it)
        assert held.start_index == 0 and it == 6
        d = _diff(got, i, p, held)
        print("variant %d order %s instance %d: host - numpy %.2e" % (v, order, i, d))
        assert d < wc.TOL_SAME_PATH, (i, d)


@pytest.mark.parametrize("v", VARIANTS)
def test_under_window_the_warm_start_is_the_second_start(cases, v):
    """start_order "window", two iterations for the first start, the default limit (300 + 10 N) for the later ones: the window pass
    is cut off, the warm pass in the x0 slot converges and is the held one, the third start never runs.  Against the two numpy
    passes chained by hand: status and iteration count (2 + the warm pass's) equal, the plan within 1e-9.  All starts reach one
    optimum here, so the words cannot tell them apart; the iteration count can: with the unshifted vector, with the x0 start, or
    with barrier parameter 0.1 in that slot, numpy takes another number of iterations on every instance.  Measured, warm pass:
    obca_mpc4 24 24 28 31 (unshifted 8 9 8 8, x0 56 49 61 52, mu 0.1: 19 22 25 17), obca_mpc6 33 30 28 27 (22 19 21 14, 44 45 41 36,
    29 31 30 25), obca_mpc8 42 28 25 27 (27 12 12 18, 28 25 38 24, 44 23 27 24); largest difference of the plan 1.8e-15."""
    b, ps, _, _, zp = cases[v]
    ret = ipm_dense.retry_iter(wc.N)
    got = wc.host(b, warm=(zp.copy(), None, WARM_MU_ORDER), start_order="window", patience=2, dodge=False)
    for i, p in enumerate(ps):
        held, it = _numpy_ladder(p, wc.shift(p, zp[i]), "window", 2, ret)
        assert held.start_index == 1 and held.status in (0, 1) and it == 2 + held.iters < 2 + ret
        assert got["status"][i] == held.status and got["iters"][i] == it, (i, got["status"][i], held.status, got["iters"][i], it)
        d = _diff(got, i, p, held, z=False)
        print("variant %d window, warm pass held, instance %d: %d iterations, host - numpy %.2e" % (v, i, it, d))
        assert d < wc.TOL_SAME_PATH, (i, d)
        for what, x, mu in (("unshifted", zp[i, :p.n], WARM_MU_ORDER), ("x0", ipm_dense.x0_start(p), WARM_MU_ORDER), ("mu 0.1", wc.shift(p, zp[i]), 0.1)):
            other, it_other = _numpy_ladder(p, x, "window", 2, ret, mu=mu)
            assert other.start_index == 1 and it_other != got["iters"][i], (i, what, it_other)


def test_large_shapes_of_the_gpu_tier_build_on_the_host():
    """the shapes tests/test_gpu_warm_start.py falls back to where a mode refuses the small ones -- (12, 3, 6), (20, 5, 14),
    (26, 5, 14), four instances -- through the same warm_case.case: the generator's rows fit the shape, the cold solves converge
    and store, the truncated warm solves end with status -1 after three iterations"""
    for shape in ((12, 3, 6), (20, 5, 14), (26, 5, 14)):
        c = wc.case(shape, 4)
        assert np.isin(c["cold"]["status"], (0, 1)).all(), (shape, c["cold"]["status"])
        assert c["start"]["iters"].tolist() == [3] * 4
        for i, p in enumerate(c["ps"]):
            assert p.N == shape[0] and np.array_equal(c["z"][i, :p.n], c["cold"]["z"][i, :p.n]) and not np.any(c["z"][i, :p.n] == wc.SENTINEL)


@pytest.mark.parametrize("v", VARIANTS)
def test_receding_horizon_pair_converges_like_numpy(v):
    """call 1 cold, storing; call 2 one step later (x0 = the plan's second pose, the window one stage forward) warm, full iteration
    limits, against one numpy pass from shift(z1) with barrier parameter 0.1: equal status; 1e-9 where the iteration counts
    agree, 1e-5 elsewhere, at most one instance in five there; and the warm solves take no more iterations than cold ones.
    Compared are the plan's words -- poses, inputs, step length -- as in tests/test_lpi_core_cpu.py: the multipliers lambda, mu of a
    converged point are held only to the solver's own tolerance (measured on obca_mpc4: 9.5e-10 in them, 1.8e-13 in the plan).
    Generator offsets (warm_case.RECEDING_FIRST) chosen on the host among 0, 4 .. 20 -- host core and numpy took equal iteration
    counts on every instance at every one of them; iterations of the second solve, host = numpy, and of its cold twin:
      obca_mpc4, first 0:  16 16 16 16 (cold 18 19 21 19), largest difference 1.8e-13
      obca_mpc6, first 20: 25 25 22 26 (cold 27 34 25 31), 8.9e-16
      obca_mpc8, first 0:  27 17 17 24 (cold 34 25 20 24), 8.9e-16"""
    b = wc.batch(v, B, first=wc.RECEDING_FIRST[v])
    z, first = wc.stored(b)
    assert np.isin(first["status"], (0, 1)).all()
    b2 = wc.next_step(b, first)
    z1 = z.copy()
    warm = wc.host(b2, warm=(z, None, wc.MU))
    cold = wc.host(b2)
    other = 0
    for i, p in enumerate(wc.problems(b2)):
        r = _numpy_pass(p, wc.shift(p, z1[i]), ipm_dense.options_for(v)["max_iter"])
        assert warm["status"][i] == r.status, (i, warm["status"][i], r.status)
        same = warm["iters"][i] == r.iters
        other += not same
        d = _diff(warm, i, p, r, z=False)
        print("variant %d instance %d: iterations host %d numpy %d, host - numpy %.2e" % (v, i, warm["iters"][i], r.iters, d))
        assert d < (wc.TOL_SAME_PATH if same else wc.TOL_OTHER), (i, d)
    assert other <= B / 5
    assert np.isin(warm["status"], (0, 1)).all()
    assert warm["iters"].sum() <= cold["iters"].sum(), (warm["iters"], cold["iters"])
