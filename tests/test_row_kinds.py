"""The compile-time slot trait of the solver's row loops (csrc/obca_device.h: obca_mu_slot) against a numpy restatement of the
row layout (csrc/obca_kernel.hip: obca_ipm_body, `---- layout`).  No GPU.

Thread t of an instance owns rows t, t + nt, t + 2 nt, ...: slot j is rows nt j .. nt j + nt - 1.  The trait is the first slot
that holds nothing but `mu >= 0` rows for every variant; the kernels with a compile-time shape drop the bound loads and the
equality / upper-bound / weight paths of their row loops from that slot on.  So every row of every slot from the trait on must
be a mu row -- lo = 0, up = +inf, weight 1, not an equality, not a soft row -- under each of the three variants, and the slot
before the trait must hold a row that is not one under at least one of them (otherwise the trait leaves work in)."""
import numpy as np
import pytest

import __graft_entry__ as ge
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib

# csrc/obca_device.h: OBCA_SHAPES, OBCA_MW_SHAPES (N, obstacles, half-space rows)
SHAPES = [(5, 2, 2), (5, 3, 6), (5, 4, 10), (5, 5, 14), (5, 6, 18), (6, 2, 2), (6, 3, 6), (6, 4, 10), (6, 5, 14), (20, 3, 6), (20, 5, 14)]
# the values the issue lists, at the thread count of the shape's kernel
LISTED = {(5, 3, 6, 64): 2, (6, 3, 6, 64): 3, (5, 2, 2, 64): 2, (5, 5, 14, 64): 4, (5, 6, 18, 64): 4, (20, 3, 6, 256): 2, (20, 5, 14, 256): 3}


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def layout(N, nO, M, variant):
    """row offsets as obca_ipm_body forms them"""
    free_T = variant == 4
    L = dict(r_init=0, r_dyn=3, r_term=3 + 3 * N)
    L["r_xb"] = L["r_term"] + (3 if variant == 4 else 0)
    L["r_ub"] = L["r_xb"] + 2 * (N + 1)
    L["r_acc"] = L["r_ub"] + 2 * N
    L["r_T"] = L["r_acc"] + 2 * N
    L["r_tx"] = L["r_T"] + (2 if free_T else 0)
    L["r_norm"] = L["r_tx"] + (2 if variant == 6 else 0)
    L["r_dist"] = L["r_norm"] + (N + 1) * nO
    L["r_lam"] = L["r_dist"] + (N + 1) * nO
    L["r_mu"] = L["r_lam"] + (N + 1) * M
    L["R"] = L["r_mu"] + (N + 1) * 4 * nO
    return L


def row_kinds(N, nO, M, variant):
    """per row: (lower bound is 0 and upper bound +inf, equality, soft, weight) by the rules of row_bounds / row_iseq / row_soft /
    row_w, and whether the row is a mu row; bounds that depend on the instance (boxes, terminal set, dmin) count as `not (0, inf)`"""
    L = layout(N, nO, M, variant)
    r = np.arange(L["R"])
    zero_inf = (r >= L["r_lam"]) | ((variant == 4) & (r == L["r_T"]))     # lambda >= 0, mu >= 0, the first Topt row
    iseq, soft = r < L["r_xb"], r < L["r_term"]
    w = np.where((variant == 4) & (r >= L["r_T"]) & (r < L["r_T"] + 2), N + 1.0, 1.0)
    return L, zero_inf, iseq, soft, w, r >= L["r_mu"]


def test_headline_offsets_are_the_documented_ones():
    got = {v: layout(5, 3, 6, v) for v in (4, 6, 8)}
    assert [got[v]["r_norm"] for v in (4, 6, 8)] == [55, 52, 50]
    assert [got[v]["r_mu"] for v in (4, 6, 8)] == [127, 124, 122]
    assert [got[v]["R"] for v in (4, 6, 8)] == [199, 196, 194]


@pytest.mark.parametrize("nt", [64, 256])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "s%d_%d_%d" % s)
def test_slot_trait_against_the_layout(lib, shape, nt):
    N, nO, M = shape
    j = lib.obca_internal_mu_slot(N, nO, M, nt)
    if shape + (nt,) in LISTED:
        assert j == LISTED[shape + (nt,)]
    assert j >= 1                                  # slot 0 always holds the initial-condition rows
    before_is_mixed = False
    for variant in (4, 6, 8):
        L, zero_inf, iseq, soft, w, is_mu = row_kinds(N, nO, M, variant)
        rows = np.arange(nt * j, L["R"])           # every row of the qualifying slots (none where nt j >= R: nothing changes)
        assert is_mu[rows].all()
        assert zero_inf[rows].all() and not iseq[rows].any() and not soft[rows].any() and (w[rows] == 1.0).all()
        prev = np.arange(nt * (j - 1), min(nt * j, L["R"]))
        before_is_mixed |= bool((~is_mu[prev]).any())
    assert before_is_mixed


def test_the_generic_edge_case_sits_on_a_slot_boundary(lib):
    """N = 5, m = [1, 2, 4] under obca_mpc8: r_mu = 128 = 2 * 64, the edge the trait is computed from (tests/test_gpu_row_kinds.py
    runs it on the generic kernels, which carry no trait)"""
    assert layout(5, 3, 7, 8)["r_mu"] == 128
    assert lib.obca_internal_mu_slot(5, 3, 7, 64) == 3      # obca_mpc4's r_mu = 133 decides: slot 2 is mixed for that variant


@pytest.mark.parametrize("name", ["s5_3_6_mpc4", "s5_3_6_mpc6", "s5_3_6_mpc8"])
def test_witness_instances_hold_a_double_decrease_and_a_corrected_solve(name):
    """tests/test_gpu_row_kinds.py names one instance per s5_3_6 case on which the Python oracle meets what the barrier re-check and
    the switching condition's powers touch: an iteration in which the barrier parameter falls twice or more, and a line search that
    starts a second-order correction.  Checked here from the oracle's trace (mu per iteration) and its soc_tried count; the
    iteration count is the C oracle's, which the GPU test compares the kernels with."""
    import test_gpu_row_kinds as g
    from oracle import c_oracle, ipm_dense
    from oracle.obca_nlp import Problem
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import SolverParams
    sp = SolverParams()
    b, N, variant, _, _, _ = g.CASES[name]()
    i = g.WITNESS[name]
    W = (sp.Q_free, sp.R_free, sp.P_free) if variant == 4 else (sp.Q_fix, sp.R_fix, sp.P_fix)
    p = Problem(variant, N, b["m"], b["x0"][i], b["u0"][i], b["xref"][i], b["A"][i], b["b"][i], b["Ts"][i], W[0], W[1][0], W[1][1], W[2],
                sp.xL, sp.xU, sp.uL, sp.uU, sp.ego, sp.dmin, term=b["term"][i] if variant == 6 else None)
    trace = []
    r = ipm_dense.solve(p, trace=trace)
    assert r.status in (0, 1)
    mu_floor = ipm_dense.options_for(variant)["tol"] / (ipm_dense.options_for(variant)["kappa_eps"] + 1.0)
    doubles = 0
    for a, c in zip(trace[:-1], trace[1:]):         # decreases between two iterations: the update rule applied until it meets the next mu
        m, k = a["mu"], 0
        while abs(m - c["mu"]) > 1e-15 * m and k < 10:
            m = max(mu_floor, min(0.2 * m, m ** 1.5))
            k += 1
        assert k < 10
        doubles += k >= 2
    assert doubles >= 1
    assert getattr(r, "soc_tried", 0) >= 1
    sl = slice(i, i + 1)
    ref = c_oracle.solve_batch(np.full(1, variant, np.int32), N, b["m"], b["x0"][sl], b["u0"][sl], b["xref"][sl], b["A"][sl], b["b"][sl],
                               b["Ts"][sl], b["term"][sl])
    assert ref["status"][0] in (0, 1) and ref["iters"][0] == r.iters
