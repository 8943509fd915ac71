"""The mu slots of the per-variant bodies read their entries of the step and of the trial point themselves (csrc/obca_kernel.hip:
mu_direct, csrc/obca_device.h: obca_mu_entry) where the rolled staging loops wrote a copy per row to S.tmp: the row steps form
dy = (dx[e] + gh[r]) * Einv[r] in the slot loop, the line search, the second-order correction's residuals and the accepted row
values read xt[e].  No arithmetic expression changes, so every output word must be the one of the staged path.

Two references, as in tests/test_gpu_variant_const.py (whose helpers are used as they are).  The generic kernels
(obca_set_shape_specialisation(h, 0)) keep the staged path for every row: WORD FOR WORD, every output array.  And the dense C
oracle under the rule of tests/test_gpu_phase_loads.py: the feasibility class is the oracle's on every instance; where the
iteration counts agree the plans agree to 1e-9, otherwise to 1e-5; the cap on the instances at the looser bound is 0, the count
tests/test_gpu_row_kinds.py measured per case with a parent build -- this change alters no arithmetic result.

The cases are the batches of tests/test_gpu_row_kinds.py (32 instances each), where the qualifying slots differ:
  s5_3_6_mpc4 / 6 / 8   slots 2 and 3, the last slot holds 7 / 4 / 2 rows
  s6_3_6                r_mu = 148 inside slot 2: only the fourth slot reads directly, 40 lanes
  s5_2_2                the qualifying slot holds 11 rows
  s5_5_14_mpc6          the fifth slot, ragged (60 lanes); a kernel that spills: the entry index is formed again at each use
plus one launch of the three variants interleaved (neighbouring wavefronts run different copies) and one in which the first start
fails and the driver enters the copy again (patience = 10).  tests/test_mu_entry.py shows on the host, from the Python oracle's
trace, that the witness instance of each case has a line search with a second trial, a started second-order correction and a
repeated factorisation -- the paths that re-enter the moved code; here the witness must take the oracle's iteration count (every
line-search decision went the oracle's way) with more factorisations than iterations."""
import numpy as np
import pytest

import test_gpu_row_kinds as g
import test_gpu_variant_const as vc
from test_mu_entry import WITNESS

pytestmark = pytest.mark.gpu

CASES = ("s5_3_6_mpc4", "s5_3_6_mpc6", "s5_3_6_mpc8", "s6_3_6", "s5_2_2", "s5_5_14_mpc6")


@pytest.mark.parametrize("name", CASES)
def test_direct_reads_give_the_staged_words(name):
    assert g.CASES[name]()[3]                     # a compile-time-shape kernel runs it
    b, N, v, ref = g.oracle(name)
    assert len(v) == g.B
    got, generic = vc._both(b, N, v)
    vc._same_words(got, generic, name)
    same, corrected = vc._against_oracle(name, got, ref)
    w = WITNESS[name]
    assert same[w] and got["info"][w, 3] > got["iters"][w]
    assert corrected[w] >= 1                      # the witness's corrected solve (the oracle does not count it, the kernels do)


def test_three_variants_in_one_launch():
    b, N, v = vc._mixed_batch((5, 3, 6))
    ref = vc._oracle(("mixed", (5, 3, 6)), b, N, v)
    got, generic = vc._both(b, N, v)
    vc._same_words(got, generic, "mixed")
    vc._against_oracle("mixed s5_3_6", got, ref)
    for variant in (4, 6, 8):
        assert ((v == variant) & np.isin(got["status"], (0, 1))).sum() == 32


def test_a_later_pass_of_the_ladder():
    """patience = 10: the first start of every instance ends at its iteration limit, the second runs the same copy from its own row
    initialisation (the staged S.tmp of the first pass is stale by then)"""
    name = "s5_3_6_mpc4"
    b, N, v, _ = g.oracle(name)
    ref = vc._oracle(("patience", name), b, N, v, patience=10)
    got, generic = vc._both(b, N, v, patience=10)
    vc._same_words(got, generic, name)
    same, _ = vc._against_oracle(name + " patience 10", got, ref)
    assert (got["iters"] > 10).all() and same[WITNESS[name]]
