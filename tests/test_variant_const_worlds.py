"""The worlds tests/test_gpu_variant_const.py picks for its obca_mpc4 instances at (5, 5, 14) and (5, 6, 18)
(S5_5_14_MPC4_WORLDS, S5_6_18_MPC4_WORLDS), derived again on the host.  No GPU.

The stated rule: of the first worlds of the gated C3 generator (tests/test_gpu_shapes.py: _batch) under obca_mpc4, the first
32 on which the dense C oracle and the structured host core (csrc/obca_lpi_core.h through tests/native) -- two CPU
implementations of one rule -- both converge, take the same number of iterations and end within 1e-10 of each other.  And the
reason for picking at all: on the worlds left out the two differ by more than the 1e-9 of the GPU test's rule."""

import numpy as np
import pytest

from __graft_entry__ import host_cpus
import test_gpu_shapes as gs
import test_gpu_variant_const as vc
from oracle import c_oracle
from tests import native_build

POOL, AGREE = 160, 1e-10           # (the lists end at world 155; the generator's worlds do not depend on how many are drawn)


@pytest.mark.parametrize("nO,worlds", [(5, vc.S5_5_14_MPC4_WORLDS), (6, vc.S5_6_18_MPC4_WORLDS)], ids=["s5_5_14", "s5_6_18"])
def test_the_listed_worlds_are_the_first_on_which_the_cpu_implementations_agree(nO, worlds):
    b = gs._batch(5, nO, POOL)
    v = np.full(POOL, 4, np.int32)
    args = (5, b["m"], b["x0"], b["u0"], b["xref"], b["A"], b["b"], b["Ts"], b["term"])
    ref = c_oracle.solve_batch(v, *args, threads=min(POOL, host_cpus()))
    host = native_build.lpi_solve(v, *args)
    ok = np.isin(ref["status"], (0, 1)) & np.isin(host["status"], (0, 1)) & (host["iters"] == ref["iters"])
    dev = np.array([max(np.abs(host["xopt"][i] - ref["xopt"][i]).max(), np.abs(host["uopt"][i] - ref["uopt"][i]).max(),
                        abs(host["ts_opt"][i] - ref["ts_opt"][i])) for i in range(POOL)])
    good = np.nonzero(ok & (dev <= AGREE))[0]
    print("worlds that agree to %.0e: %d of %d; largest deviation among the others %.2e" % (AGREE, len(good), POOL, dev[ok & (dev > AGREE)].max()))
    assert len(worlds) == 32 and good[:32].tolist() == list(worlds)
    assert dev[:32].max() > 1e-9                             # the generator's first 32 worlds are beyond the GPU test's bound
