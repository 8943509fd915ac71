"""The per-variant bodies of the one-wavefront compile-time-shape kernels (csrc/obca_kernel.hip: ShapeIs<N, nO, M, FT, variant>,
solve_passes: one wave-uniform branch per instance to a loop over the body compiled for its variant, whose row layout is a constant
-- csrc/obca_device.h: obca_row_layout -- and whose rolled row loops send the rounds of mu rows alone straight to the mu formula).

Two references.  The generic kernels (obca_set_shape_specialisation(h, 0): the variant, the layout and the whole kind ladder at
run time): WORD FOR WORD, every output array.  And the dense C oracle under the rule of tests/test_gpu_row_kinds.py, whose helpers
are used as they are: the feasibility class is the oracle's on every instance; where the iteration counts agree the plans agree to
1e-9, otherwise to 1e-5; where they agree the kernel's factorisation count minus the oracle's is the number of corrected solves,
never negative.  The batches are generator seeds on which the oracle converges on every instance (checked on the host), except
where a case says otherwise.  The cap on the instances at the looser bound is 0 in every case, as every cap of that file is: on
the host the structured core (csrc/obca_lpi_core.h: the kernels' rule and arithmetic) takes the oracle's iteration count on every
converging instance of every case here, and nothing in the per-variant bodies alters an arithmetic result.  Every converging case
must also hold an instance with more factorisations than iterations (refact >= 1), as there.

What each case is there for:
  mixed        96 instances, variants 4, 6, 8 interleaved (i % 3) and four masked ones (variant 0): neighbouring wavefronts take
               different copies; a masked instance keeps every output word but status / iters.  (5, 2, 2) the smallest listed shape,
               (5, 3, 6) the headline, (6, 3, 6) whose mu rounds begin at slot 3, (5, 6, 18) the largest (a ragged last round of
               59 / 56 / 54 rows).
  one variant  a batch of 32 per variant at (5, 3, 6) -- the batches of tests/test_gpu_row_kinds.py, with its witness instances
               (an iteration of two barrier decreases and a corrected solve: use_soc crosses the peeled row loops) -- and (5, 5, 14).
  later passes the driver enters a variant's copy again: patience = 10 makes the first start of every instance of the (5, 3, 6)
               batches fail, the second converges (host: 51 .. 69 iterations under obca_mpc4, 29 .. 38 under 6 / 8); with
               retry_iter = 10 too every start fails and the dodge passes of obca_mpc6 (two) and obca_mpc8 (four) run -- 30 / 50 / 70
               iterations, nothing converges (the oracle agrees: iteration limit); a terminal pose outside the road makes
               obca_mpc4 converge with elastic variables left, which is what its penalty escalation answers (the oracle: infeasible
               after ~650 iterations on each; the iteration counts differ from the kernels', the class may not).
  handle       one handle, one set of buffers: obca_mpc4, then obca_mpc8, then obca_mpc4 again gives the first call's words."""

import numpy as np
import pytest
import torch

from __graft_entry__ import host_cpus
import test_gpu_row_kinds as g
import test_gpu_shapes as gs
from oracle import c_oracle
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchResult, BatchSolver, SolverParams

pytestmark = pytest.mark.gpu

KEYS = ("xopt", "uopt", "ts_opt", "status", "iters", "info")
MASKED = (5, 40, 41, 95)                 # two neighbours among them, and the last instance
SENTINEL = -777.25
LOOSE_CAP = 0                            # instances whose iteration count may differ from the oracle's, per case (module docstring)

_cache = {}


# (5, 6, 18): worlds of the gated C3 generator (tests/test_gpu_shapes.py: _batch, its first 192).  Under obca_mpc4 most of them
# are ill-conditioned at the solution: the dense C oracle and the structured host core (csrc/obca_lpi_core.h, tests/native) --
# two CPU implementations of one rule -- take the same number of iterations on all 192 and still end up to 1.8e-8 apart (under
# obca_mpc6 / 8: 3.3e-10), which is beyond what the 1e-9 bound of the rule can tell from a wrong kernel.  The obca_mpc4 positions
# of the batch therefore take the first 32 worlds on which those two agree to 1e-10 (chosen on the host, from the two CPU
# implementations alone), the other positions the remaining worlds in order.
S5_6_18_MPC4_WORLDS = [1, 11, 14, 19, 22, 27, 28, 30, 36, 37, 45, 56, 69, 71, 81, 84, 88, 94, 95, 96, 101, 104, 112, 114, 123, 139, 143, 144,
                       148, 149, 151, 155]

S5_5_14_MPC4_WORLDS = [1, 11, 15, 19, 22, 24, 27, 30, 33, 34, 35, 36, 37, 39, 43, 45, 47, 70, 72, 74, 77, 87, 88, 92, 96, 102, 107, 109, 110, 111, 112,
                       114]


def _mixed_batch(shape):
    N, nO, M = shape
    if shape == (5, 6, 18):
        pool = gs._batch(N, nO, 192)
        rest = iter([i for i in range(192) if i not in S5_6_18_MPC4_WORLDS])
        free = iter(S5_6_18_MPC4_WORLDS)
        idx = np.array([next(free) if i % 3 == 0 else next(rest) for i in range(96)])
        b = {k: (a[idx] if isinstance(a, np.ndarray) else a) for k, a in pool.items()}
    else:
        b = gs._batch(N, nO, 96)
    if nO <= 3:
        b = g._terminal_set(b)           # the headline generator carries no terminal set
    assert sum(b["m"]) == M and len(b["m"]) == nO
    v = np.array([4, 6, 8], np.int32)[np.arange(96) % 3]
    return b, N, v


def _oracle(key, b, N, v, **prm):
    """the dense C oracle, once per case"""
    if key not in _cache:
        p = c_oracle.default_params(**prm)
        _cache[key] = c_oracle.solve_batch(v, N, b["m"], b["x0"], b["u0"], b["xref"], b["A"], b["b"], b["Ts"], b["term"], params=p,
                                           threads=min(len(v), host_cpus()))
    return _cache[key]


def _solve(s, b, v, out=None, **prm):
    o = s.solve(v, b["x0"], b["u0"], b["xref"], b["A"], b["b"], b["Ts"], b["term"], SolverParams(**prm), out=out)
    torch.cuda.synchronize()
    return {k: getattr(o, k).cpu().numpy().copy() for k in KEYS}


def _both(b, N, v, prefill=False, **prm):
    """(words of the specialised kernels, words of the generic ones); prefill: every output buffer starts at SENTINEL"""
    s = BatchSolver(N, b["m"], max_batch=len(v))
    assert s.specialised
    res = []
    for on in (True, False):
        s.set_shape_specialisation(on)
        assert bool(s.specialised) == on
        out = None
        if prefill:
            B, M = len(v), s.M
            out = BatchResult()
            out.xopt = torch.full((B, 3, N + 1), SENTINEL, dtype=torch.float64, device=s.device)
            out.uopt = torch.full((B, 2, N), SENTINEL, dtype=torch.float64, device=s.device)
            out.ts_opt = torch.full((B,), SENTINEL, dtype=torch.float64, device=s.device)
            out.status = torch.full((B,), 12345, dtype=torch.int32, device=s.device)
            out.iters = torch.full((B,), 12345, dtype=torch.int32, device=s.device)
            out.info = torch.full((B, 4), SENTINEL, dtype=torch.float64, device=s.device)
        res.append(_solve(s, b, v, out=out, **prm))
    s.close()
    return res


def _same_words(got, ref, what):
    for k in KEYS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), (what, k)


def _against_oracle(name, got, ref, pick=None, all_converge=True):
    """the rule of tests/test_gpu_row_kinds.py on the instances `pick`"""
    if pick is not None:
        got, ref = {k: a[pick] for k, a in got.items()}, {k: a[pick] for k, a in ref.items()}
    if all_converge:
        loose, dev_tight, dev_loose, refact = g.compare(got, ref)           # (asserts that the oracle converged everywhere and the class)
    else:
        ok_ref, ok = np.isin(ref["status"], (0, 1)), np.isin(got["status"], (0, 1))
        assert np.array_equal(ok, ok_ref)
        dev = np.array([max(np.abs(got["xopt"][i] - ref["xopt"][i]).max(), np.abs(got["uopt"][i] - ref["uopt"][i]).max(),
                            abs(got["ts_opt"][i] - ref["ts_opt"][i])) for i in range(len(ok))])
        same = got["iters"] == ref["iters"]
        loose, dev_tight, dev_loose = int((~same & ok).sum()), float(dev[same & ok].max(initial=0.0)), float(dev[~same & ok].max(initial=0.0))
        refact = int((got["info"][:, 3] > got["iters"]).sum())
    same = got["iters"] == ref["iters"]
    corrected = (got["info"][:, 3] - ref["info"][:, 3]).astype(int)
    print("%s: %d of %d at the looser bound, max deviation %.2e / %.2e, %d with more factorisations than iterations, corrected solves %d; %d iterations, %d factorisations (oracle: %d, %d)"
          % (name, loose, len(same), dev_tight, dev_loose, refact, corrected[same].sum(), got["iters"].sum(), got["info"][:, 3].sum(),
             ref["iters"].sum(), ref["info"][:, 3].sum()))
    assert dev_tight <= 1e-9
    assert dev_loose <= 1e-5
    assert loose <= LOOSE_CAP
    if all_converge:
        assert refact >= 1
    assert (corrected[same] >= 0).all()
    return same, corrected


@pytest.mark.parametrize("shape", [(5, 2, 2), (5, 3, 6), (6, 3, 6), (5, 6, 18)], ids=lambda s: "s%d_%d_%d" % s)
def test_mixed_variants_in_one_launch(shape):
    b, N, v = _mixed_batch(shape)
    ref = _oracle(("mixed", shape), b, N, v)
    vm = v.copy()
    vm[list(MASKED)] = 0
    got, generic = _both(b, N, vm, prefill=True)
    _same_words(got, generic, shape)
    m = np.zeros(len(v), bool)
    m[list(MASKED)] = True
    assert (got["status"][m] == _lib.STATUS_SKIPPED).all() and (got["iters"][m] == 0).all()
    for k in ("xopt", "uopt", "ts_opt", "info"):                        # a masked instance's outputs are untouched
        assert (got[k][m] == SENTINEL).all(), k
        assert not (got[k][~m] == SENTINEL).any(), k
    same, corrected = _against_oracle("mixed s%d_%d_%d" % shape, got, ref, pick=~m)
    assert got["info"][~m, 3].sum() > got["iters"][~m].sum()          # repeated factorisations / corrected solves happened
    for variant in (4, 6, 8):                                          # ... and every copy ran
        assert ((vm == variant) & np.isin(got["status"], (0, 1))).sum() >= 28


@pytest.mark.parametrize("name", ["s5_3_6_mpc4", "s5_3_6_mpc6", "s5_3_6_mpc8"])
def test_one_variant_per_launch_headline_shape(name):
    """the batches and witness instances of tests/test_gpu_row_kinds.py"""
    b, N, v, ref = g.oracle(name)
    got, generic = _both(b, N, v)
    _same_words(got, generic, name)
    same, corrected = _against_oracle(name, got, ref)
    w = g.WITNESS[name]
    assert same[w] and corrected[w] >= 1


@pytest.mark.parametrize("variant", [4, 6, 8])
def test_one_variant_per_launch_s5_5_14(variant):
    if variant == 4:                     # the rule of S5_6_18_MPC4_WORLDS on this shape's first 192 worlds (the two CPU implementations: up to 8.6e-9 apart on the first 32)
        pool = gs._batch(5, 5, 192)
        b = {k: (a[S5_5_14_MPC4_WORLDS] if isinstance(a, np.ndarray) else a) for k, a in pool.items()}
    else:
        b = gs._batch(5, 5, 32)
    v = np.full(32, variant, np.int32)
    ref = _oracle(("s5_5_14", variant), b, 5, v)
    got, generic = _both(b, 5, v)
    _same_words(got, generic, variant)
    _against_oracle("s5_5_14 variant %d" % variant, got, ref)
    assert got["info"][:, 3].sum() > got["iters"].sum()


@pytest.mark.parametrize("name", ["s5_3_6_mpc4", "s5_3_6_mpc6", "s5_3_6_mpc8"])
def test_second_start_after_a_failed_first(name):
    """patience = 10: the first start ends at its iteration limit on every instance, the driver enters the copy again"""
    b, N, v, _ = g.oracle(name)
    ref = _oracle(("patience", name), b, N, v, patience=10)
    got, generic = _both(b, N, v, patience=10)
    _same_words(got, generic, name)
    same, corrected = _against_oracle(name + " patience 10", got, ref)
    assert (got["iters"] > 10).all()                                   # more than the first start's ten
    w = g.WITNESS[name]
    assert same[w]


@pytest.mark.parametrize("name,total", [("s5_3_6_mpc4", 30), ("s5_3_6_mpc6", 50), ("s5_3_6_mpc8", 70)])
def test_every_pass_of_the_ladder_runs(name, total):
    """patience = retry_iter = 10: three starts, then the two dodge passes of obca_mpc6 / the four of obca_mpc8, ten iterations each"""
    b, N, v, _ = g.oracle(name)
    b, v = {k: (a[:8] if isinstance(a, np.ndarray) else a) for k, a in b.items()}, v[:8]
    ref = _oracle(("ladder", name), b, N, v, patience=10, retry_iter=10)
    assert (ref["iters"] == total).all() and (ref["status"] == _lib.STATUS_MAXITER).all()
    got, generic = _both(b, N, v, patience=10, retry_iter=10)
    _same_words(got, generic, name)
    assert (got["iters"] == total).all()
    _against_oracle(name + " ladder", got, ref, all_converge=False)


def test_penalty_escalation_of_obca_mpc4():
    """a terminal pose outside the road: the solve converges with elastic variables left, the same start runs again with the
    penalty x 100 and x 1000, then the next starts; infeasible in the end, as the oracle says"""
    b, N, v, _ = g.oracle("s5_3_6_mpc4")
    b, v = {k: (a[:8].copy() if isinstance(a, np.ndarray) else a) for k, a in b.items()}, v[:8]
    b["xref"][:, 1, N] = 15.0
    ref = _oracle(("escalation",), b, N, v)
    assert (ref["status"] == _lib.STATUS_INFEASIBLE).all()
    got, generic = _both(b, N, v)
    _same_words(got, generic, "escalation")
    assert (got["status"] == _lib.STATUS_INFEASIBLE).all()
    assert (got["iters"] > 100).all()                                   # several passes (one pass of this batch: ~17 .. 70 iterations)
    _against_oracle("escalation", got, ref, all_converge=False)


def test_one_handle_variant_4_then_8_then_4():
    b, N, _, _ = g.oracle("s5_3_6_mpc4")
    B = len(b["variant"])
    s = BatchSolver(N, b["m"], max_batch=B)
    assert s.specialised
    out = BatchResult()
    out.xopt = torch.zeros(B, 3, N + 1, dtype=torch.float64, device=s.device)
    out.uopt = torch.zeros(B, 2, N, dtype=torch.float64, device=s.device)
    out.ts_opt = torch.zeros(B, dtype=torch.float64, device=s.device)
    out.status = torch.zeros(B, dtype=torch.int32, device=s.device)
    out.iters = torch.zeros(B, dtype=torch.int32, device=s.device)
    out.info = torch.zeros(B, 4, dtype=torch.float64, device=s.device)
    first = _solve(s, b, np.full(B, 4, np.int32), out=out)
    other = _solve(s, b, np.full(B, 8, np.int32), out=out)
    third = _solve(s, b, np.full(B, 4, np.int32), out=out)
    s.close()
    _same_words(third, first, "4, 8, 4")
    assert not np.array_equal(other["xopt"], first["xopt"]) and (other["ts_opt"] == b["Ts"]).all()      # the fixed-time answer in between
    assert np.isin(first["status"], (0, 1)).all() and np.isin(other["status"], (0, 1)).all()
