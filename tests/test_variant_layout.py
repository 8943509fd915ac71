"""The row layout as a constant (csrc/obca_device.h: obca_row_layout) and the slot statements the per-variant bodies of the
one-wavefront compile-time-shape kernels are built from (obca_slot_kinds, obca_own_mu_slot, obca_mixed_kinds; csrc/obca_kernel.hip:
ShapeIs<N, nO, M, FT, variant>, mixed_then_mu).  No GPU.

Field by field the constant layout must be the one the host core builds at run time (csrc/obca_lpi_core.h: make_layout, through
tests/native/variant_layout_host.cpp) -- for every listed shape and each variant -- and the library must export the same numbers
(obca_internal_row_layout, as obca_internal_mu_slot is exported).  The slot statements are checked against the kinds of the rows
64 j .. 64 j + 63 enumerated in numpy from the RUN-TIME layout: a round the kernels send straight to the mu formula holds mu rows
only, the ladder of the rounds before it carries every kind those rounds hold, and a kind it drops has no row there.  The ragged
last rounds are part of it: (5, 3, 6) ends with 7 / 4 / 2 rows under obca_mpc4 / 6 / 8, (5, 2, 2) with 11 / 8 / 6."""
import ctypes
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import native_build
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib

# csrc/obca_device.h: OBCA_SHAPES (one wavefront, 64 threads) and OBCA_MW_SHAPES (four wavefronts, 256 threads)
SHAPES = [(5, 2, 2), (5, 3, 6), (5, 4, 10), (5, 5, 14), (5, 6, 18), (6, 2, 2), (6, 3, 6), (6, 4, 10), (6, 5, 14)]
MW_SHAPES = [(20, 3, 6), (20, 5, 14)]
VARIANTS = (4, 6, 8)
FIELDS = ("r_init", "r_dyn", "r_term", "r_xb", "r_ub", "r_acc", "r_T", "r_tx", "r_norm", "r_dist", "r_lam", "r_mu", "R", "n", "free_T")
KINDS = ("init", "dyn", "term", "xb", "ub", "acc", "T", "tx", "norm", "dist", "lam", "mu")      # bit k of a kind mask
MU = 1 << KINDS.index("mu")
SRC = os.path.join(native_build.HERE, "native", "variant_layout_host.cpp")
ids = lambda s: "s%d_%d_%d" % s


@functools.lru_cache(maxsize=None)
def host():
    return native_build.build_shim("variant_layout_host", [SRC])


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def fields(fn, N, nO, M, variant):
    out = (ctypes.c_int * len(FIELDS))()
    fn(N, nO, M, variant, out)
    return dict(zip(FIELDS, out))


def kinds_of_rows(L):
    """kind index of every row of a run-time layout"""
    first = [L[k] for k in FIELDS[:12]] + [L["R"]]
    assert all(a <= b for a, b in zip(first[:-1], first[1:]))
    kind = np.empty(L["R"], int)
    for k in range(12):
        kind[first[k]:first[k + 1]] = k
    return kind


def mask(kinds):
    return int(sum(1 << int(k) for k in set(kinds.tolist())))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES + MW_SHAPES, ids=ids)
def test_constant_layout_is_the_run_time_layout(lib, shape, variant):
    N, nO, M = shape
    run = fields(host().variant_layout_host_runtime, N, nO, M, variant)
    assert fields(host().variant_layout_host_constant, N, nO, M, variant) == run
    assert fields(lib.obca_internal_row_layout, N, nO, M, variant) == run
    # the sums written out once more: variables and rows of the problem (oracle/obca_nlp.py)
    assert run["free_T"] == (1 if variant == 4 else 0)
    assert run["n"] == (N + 1) * (3 + M + 4 * nO) + 2 * N + run["free_T"]
    assert run["R"] - run["r_mu"] == (N + 1) * 4 * nO and run["r_mu"] - run["r_lam"] == (N + 1) * M
    assert run["r_xb"] - run["r_term"] == (3 if variant == 4 else 0)
    assert run["r_tx"] - run["r_T"] == (2 if variant == 4 else 0) and run["r_norm"] - run["r_tx"] == (2 if variant == 6 else 0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES + MW_SHAPES, ids=ids)
def test_slot_statements_against_the_enumerated_rows(lib, shape, variant):
    N, nO, M = shape
    nt = 64 if shape in SHAPES else 256
    run = fields(host().variant_layout_host_runtime, N, nO, M, variant)
    kind = kinds_of_rows(run)
    nslots = (run["R"] + nt - 1) // nt
    per_slot = [mask(kind[nt * j:nt * j + nt]) for j in range(nslots)]
    for j in range(nslots + 2):                      # ... and two slots beyond the rows: nothing there
        want = per_slot[j] if j < nslots else 0
        assert host().variant_layout_host_slot_kinds(N, nO, M, variant, nt, j) == want
        assert lib.obca_internal_slot_kinds(N, nO, M, variant, nt, j) == want
    own = host().variant_layout_host_own_mu_slot(N, nO, M, variant, nt)
    mixed = host().variant_layout_host_mixed_kinds(N, nO, M, variant, nt)
    assert lib.obca_internal_own_mu_slot(N, nO, M, variant, nt) == own and lib.obca_internal_mixed_kinds(N, nO, M, variant, nt) == mixed
    # "this round holds only mu rows": every round from `own` on, and the round before it does not (else work is left in)
    assert 1 <= own <= nslots
    assert all(per_slot[j] == MU for j in range(own, nslots))
    assert per_slot[own - 1] != MU
    # "these rounds cannot hold kind K": the ladder of the rounds before `own` carries exactly the kinds that have a row there
    assert mixed == mask(kind[:min(nt * own, run["R"])])
    for k, name in enumerate(KINDS):
        empty = run[FIELDS[k]] == (run[FIELDS[k + 1]] if k < 11 else run["R"])
        if empty:
            assert not mixed & (1 << k), name        # a kind the variant lacks has no test anywhere
    # the trait shared by the three variants (obca_mu_slot) is the latest of their own slots
    assert lib.obca_internal_mu_slot(N, nO, M, nt) == max(host().variant_layout_host_own_mu_slot(N, nO, M, v, nt) for v in VARIANTS)


@pytest.mark.parametrize("shape,last", [((5, 3, 6), (7, 4, 2)), ((5, 2, 2), (11, 8, 6)), ((5, 6, 18), (59, 56, 54))], ids=lambda v: str(v))
def test_ragged_last_rounds(shape, last):
    """rows of the last round per variant, and that round is a mu round"""
    N, nO, M = shape
    for variant, rows in zip(VARIANTS, last):
        run = fields(host().variant_layout_host_constant, N, nO, M, variant)
        j = (run["R"] - 1) // 64
        assert run["R"] - 64 * j == rows
        assert host().variant_layout_host_slot_kinds(N, nO, M, variant, 64, j) == MU
        assert host().variant_layout_host_own_mu_slot(N, nO, M, variant, 64) <= j


def test_headline_rounds():
    """(5, 3, 6): rows 128 .. 198 of obca_mpc4 are two rounds of mu rows alone; slot 1 holds the last norm rows, distance, lambda and the single mu row 127;
    no initial-condition, dynamics, terminal or box row lies at or beyond row 64"""
    h = host()
    assert [h.variant_layout_host_own_mu_slot(5, 3, 6, v, 64) for v in VARIANTS] == [2, 2, 2]
    bit = lambda *names: sum(1 << KINDS.index(n) for n in names)
    assert h.variant_layout_host_slot_kinds(5, 3, 6, 4, 64, 1) == bit("norm", "dist", "lam", "mu")
    assert h.variant_layout_host_slot_kinds(5, 3, 6, 4, 64, 0) == bit("init", "dyn", "term", "xb", "ub", "acc", "T", "norm")
    assert h.variant_layout_host_slot_kinds(5, 3, 6, 6, 64, 0) == bit("init", "dyn", "xb", "ub", "acc", "tx", "norm")
    assert h.variant_layout_host_slot_kinds(5, 3, 6, 8, 64, 0) == bit("init", "dyn", "xb", "ub", "acc", "norm")
