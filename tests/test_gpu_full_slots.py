"""The unrolled slot loops of the per-variant bodies run their FULL slots -- the slots in which every lane has a row, j below
csrc/obca_device.h: obca_full_slots -- without the test `r < R` (csrc/obca_kernel.hip: row_live).  No arithmetic expression
changes, so every output word must be the one of the masked form; a count of full slots one too large would read and write rows
that do not exist, a lane of a ragged slot run unmasked would add a row's terms to the reductions.

Two references, as in tests/test_gpu_mu_direct.py (the helpers of tests/test_gpu_variant_const.py are used as they are).  The
generic kernels (obca_set_shape_specialisation(h, 0)) keep `r < R` in every slot: WORD FOR WORD, every output array, zero
differing words.  And the dense C oracle under the rule of that file: the feasibility class is the oracle's on every instance;
where the iteration counts agree the plans agree to 1e-9, otherwise to 1e-5; the cap on the instances at the looser bound is 0.

The cases, 96 instances with the three variants interleaved unless said otherwise (neighbouring wavefronts run different copies):
  s5_3_6   three full slots under every variant, the ragged fourth holds 7 / 4 / 2 rows
  s5_4_10  259 / 256 / 254 rows: obca_mpc4 has four full slots and three rows in a fifth, obca_mpc6 four full slots and NO ragged
           row, obca_mpc8 three full slots and a fourth that is 62 rows ragged -- the shape where the count differs between the
           copies of one kernel.  The worlds are the gated C3 generator's (tests/test_gpu_shapes.py: _batch, its first 192).  Under
           obca_mpc4 the dense C oracle and the structured host core (csrc/obca_lpi_core.h) -- two CPU implementations of one rule
           -- take the same number of iterations on 191 of them and still end up to 1.1e-8 apart, beyond what the 1e-9 bound can
           tell from a wrong kernel: the obca_mpc4 positions take the first 32 worlds on which the two agree to 1e-10 (43 do),
           chosen on the host from the two CPU implementations alone -- the rule of tests/test_gpu_variant_const.py:
           S5_6_18_MPC4_WORLDS.  The other positions take the remaining worlds in order, without the four (20, 71, 76, 152) on
           which the two differ by more than 1e-10 under obca_mpc6 (they agree to 3.6e-15 on all 192 under obca_mpc8).
  s5_2_2   the fewest slots: two full ones and a third of 11 / 8 / 6 rows
  a later pass of the ladder: patience = 10, the first start of every instance ends at its iteration limit and the driver enters
           the copy again from its own row initialisation (32 instances, obca_mpc6)
  a second-order correction: the witness instances tests/test_row_kinds.py documents (an iteration of two barrier decreases and
           a started correction, from the Python oracle's trace), one batch of 32 per variant at (5, 3, 6): the witness must take
           the oracle's iteration count with at least one corrected solve -- the correction's bookkeeping and the restore of dy
           after a failed one are two of the eleven loops."""
import numpy as np
import pytest

import test_gpu_row_kinds as g
import test_gpu_shapes as gs
import test_gpu_variant_const as vc

pytestmark = pytest.mark.gpu

S5_4_10_MPC4_WORLDS = [1, 11, 15, 25, 28, 32, 35, 39, 45, 46, 65, 66, 70, 77, 78, 80, 81, 84, 87, 88, 90, 101, 102, 104, 105, 107, 120, 126, 143,
                       146, 148, 149]
S5_4_10_MPC6_APART = (20, 71, 76, 152)


def _s5_4_10_batch():
    pool = gs._batch(5, 4, 192)
    assert sum(pool["m"]) == 10 and len(pool["m"]) == 4
    rest = iter([i for i in range(192) if i not in S5_4_10_MPC4_WORLDS and i not in S5_4_10_MPC6_APART])
    free = iter(S5_4_10_MPC4_WORLDS)
    idx = np.array([next(free) if i % 3 == 0 else next(rest) for i in range(96)])
    b = {k: (a[idx] if isinstance(a, np.ndarray) else a) for k, a in pool.items()}
    return b, 5, np.array([4, 6, 8], np.int32)[np.arange(96) % 3]


def _mixed(shape):
    return _s5_4_10_batch() if shape == (5, 4, 10) else vc._mixed_batch(shape)


@pytest.mark.parametrize("shape", [(5, 3, 6), (5, 4, 10), (5, 2, 2)], ids=lambda s: "s%d_%d_%d" % s)
def test_three_variants_in_one_launch(shape):
    b, N, v = _mixed(shape)
    assert len(v) == 96
    rows = [g.rows_of(N, b["m"], variant)[0] for variant in (4, 6, 8)]
    assert rows == {(5, 3, 6): [199, 196, 194], (5, 4, 10): [259, 256, 254], (5, 2, 2): [139, 136, 134]}[shape]
    ref = vc._oracle(("full_slots" if shape == (5, 4, 10) else "mixed", shape), b, N, v)
    got, generic = vc._both(b, N, v)
    vc._same_words(got, generic, shape)
    vc._against_oracle("mixed s%d_%d_%d" % shape, got, ref)
    for variant in (4, 6, 8):                                          # every copy ran, on every one of its instances
        assert ((v == variant) & np.isin(got["status"], (0, 1))).sum() == 32


def test_a_later_pass_of_the_ladder():
    name = "s5_3_6_mpc6"
    b, N, v, _ = g.oracle(name)
    ref = vc._oracle(("patience", name), b, N, v, patience=10)
    got, generic = vc._both(b, N, v, patience=10)
    vc._same_words(got, generic, name)
    same, _ = vc._against_oracle(name + " patience 10", got, ref)
    assert (got["iters"] > 10).all() and same[g.WITNESS[name]]


@pytest.mark.parametrize("name", ["s5_3_6_mpc4", "s5_3_6_mpc6", "s5_3_6_mpc8"])
def test_a_second_order_correction(name):
    assert g.CASES[name]()[3]                     # a compile-time-shape kernel runs it
    b, N, v, ref = g.oracle(name)
    got, generic = vc._both(b, N, v)
    vc._same_words(got, generic, name)
    same, corrected = vc._against_oracle(name, got, ref)
    w = g.WITNESS[name]
    assert same[w] and corrected[w] >= 1 and got["info"][w, 3] > got["iters"][w]
