"""The eight step-length guards of the rowsteps slot loop run as selects in the per-variant bodies of the shape kernels that take the
form (csrc/obca_kernel.hip: STEP_MIN, guard_selects_default): `a_max = fmin(a_max, ds < 0.0 ? v : INFINITY)`.  No arithmetic
expression changes, so every output word must be the guarded form's; a select with the wrong neutral operand, or one that let the
discarded reciprocal of a lane through, would change a step length and with it every word after that iteration.

Two references, as in tests/test_gpu_full_slots.py (the helpers of tests/test_gpu_variant_const.py are used as they are).  The
generic kernels (obca_set_shape_specialisation(h, 0)) keep the guarded form: WORD FOR WORD, every output array, zero differing
words.  And the dense C oracle under the rule of that file: the feasibility class is the oracle's on every instance; where the
iteration counts agree the plans agree to 1e-9, otherwise to 1e-5; the cap on the instances at the looser bound is 0.

A word-for-word comparison says nothing about a select that never is the minimum.  Every case therefore first runs its batch
through the structured host core (tests/native/step_guards_host.cpp, tests/test_guard_selects.py: step_guards) and asserts that
each of the eight guards -- lower and upper slack, p, n and their four multipliers -- sets the step length of at least one
iteration.  (The upper-slack pair needs a row with a finite upper bound to limit the step: the input bounds are such rows.  On
the host, per guard, iterations bound in the 64 instances of the headline batch under obca_mpc4: 49 165 100 143 417 38 29 36.)

The cases, 64 instances each:
  s5_3_6 under obca_mpc4 / 6 / 8   the headline generator (tests/test_gpu_shapes.py: _batch) with the terminal set of
                                   tests/test_gpu_row_kinds.py
  s5_3_6 mixed                     the same batch, the three variants interleaved: neighbouring wavefronts run different copies
  s5_4_10 mixed                    the first 64 of tests/test_gpu_full_slots.py: _s5_4_10_batch -- 4 / 4 / 3 full slots
  s6_2_2 mixed                     the shape with the fewest rows
  a later pass of the ladder       patience = 10 under obca_mpc6: the first start of every instance ends at its iteration limit"""
import numpy as np
import pytest

import test_gpu_full_slots as fs
import test_gpu_shapes as gs
import test_gpu_variant_const as vc
import test_guard_selects as hs

pytestmark = pytest.mark.gpu

B = 64
MIXED = np.array([4, 6, 8], np.int32)[np.arange(B) % 3]


def _batch(shape):
    if shape == (5, 4, 10):
        b, N, v = fs._s5_4_10_batch()
        return {k: (a[:B] if isinstance(a, np.ndarray) else a) for k, a in b.items()}, N
    N, nO, M = shape
    b = hs.terminal_set(gs._batch(N, nO, B))
    assert sum(b["m"]) == M and len(b["m"]) == nO
    return b, N


def _check(what, b, N, v, **prm):
    host, bound = hs.step_guards(b, N, v, **prm)
    assert (bound.sum(axis=0) > 0).all(), (what, dict(zip(hs.GUARDS, bound.sum(axis=0))))        # every guard sets a step length
    ref = vc._oracle(("guard_selects", what), b, N, v, **prm)
    got, generic = vc._both(b, N, v, **prm)
    vc._same_words(got, generic, what)
    same, _ = vc._against_oracle(what, got, ref)
    assert np.array_equal(got["iters"], host["iters"])                   # the run whose guards were counted is the kernels' run
    return got


@pytest.mark.parametrize("variant", [4, 6, 8])
def test_headline_shape_one_variant_per_launch(variant):
    b, N = _batch((5, 3, 6))
    _check("s5_3_6 variant %d" % variant, b, N, np.full(B, variant, np.int32))


@pytest.mark.parametrize("shape", [(5, 3, 6), (5, 4, 10), (6, 2, 2)], ids=lambda s: "s%d_%d_%d" % s)
def test_three_variants_in_one_launch(shape):
    b, N = _batch(shape)
    got = _check("mixed s%d_%d_%d" % shape, b, N, MIXED)
    for variant in (4, 6, 8):                                             # every copy ran, on every one of its instances
        assert ((MIXED == variant) & np.isin(got["status"], (0, 1))).sum() == (MIXED == variant).sum()


def test_a_later_pass_of_the_ladder():
    b, N = _batch((5, 3, 6))
    got = _check("s5_3_6 variant 6 patience 10", b, N, np.full(B, 6, np.int32), patience=10)
    assert (got["iters"] > 10).all()                                      # more than the first start's ten
