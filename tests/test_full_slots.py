"""Row slots in which every thread has a row (csrc/obca_device.h: obca_full_slots = R / nt of a variant's constant layout): the
unrolled slot loops of a body of one variant run these slots without the test `r < R` (csrc/obca_kernel.hip: row_live), so a count
one too large reads and writes rows that do not exist and a count too small only leaves work in.  No GPU.

The library exports the number the kernels are built with (obca_internal_full_slots, beside obca_internal_row_layout); it must be
R // nt of the exported layout for every listed shape, each variant, at 64 and at 256 threads -- and every slot below it must lie
below R entirely, the slot at it must not.  (5, 4, 10) is the shape where the three variants differ: 259, 256 and 254 rows, that
is 4 full slots and 3 rows behind them, 4 full slots and NO ragged one, 3 full slots and a fourth of 62 rows."""
import ctypes

import pytest

import __graft_entry__ as ge
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib

# csrc/obca_device.h: OBCA_SHAPES (one wavefront, 64 threads) and OBCA_MW_SHAPES (four wavefronts, 256 threads)
SHAPES = [(5, 2, 2), (5, 3, 6), (5, 4, 10), (5, 5, 14), (5, 6, 18), (6, 2, 2), (6, 3, 6), (6, 4, 10), (6, 5, 14)]
MW_SHAPES = [(20, 3, 6), (20, 5, 14)]
VARIANTS = (4, 6, 8)
R_FIELD = 12                     # out[12] of obca_internal_row_layout: R
ids = lambda s: "s%d_%d_%d" % s


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def rows(lib, N, nO, M, variant):
    out = (ctypes.c_int * 15)()
    lib.obca_internal_row_layout(N, nO, M, variant, out)
    return out[R_FIELD]


@pytest.mark.parametrize("nt", [64, 256])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES + MW_SHAPES, ids=ids)
def test_full_slots_is_rows_over_threads(lib, shape, variant, nt):
    N, nO, M = shape
    R = rows(lib, N, nO, M, variant)
    full = lib.obca_internal_full_slots(N, nO, M, variant, nt)
    assert full == R // nt
    assert nt * full <= R < nt * (full + 1)           # the last row of slot full - 1 exists, the last row of slot `full` does not
    # rows of the layout written out once more (oracle/obca_nlp.py): the count is not compared with itself alone
    assert R == 3 + 3 * N + (3 if variant == 4 else 0) + 2 * (N + 1) + 4 * N + (2 if variant == 4 else 0) + (2 if variant == 6 else 0) + \
        2 * (N + 1) * nO + (N + 1) * M + (N + 1) * 4 * nO


def test_the_shape_whose_variants_differ(lib):
    assert [rows(lib, 5, 4, 10, v) for v in VARIANTS] == [259, 256, 254]
    assert [lib.obca_internal_full_slots(5, 4, 10, v, 64) for v in VARIANTS] == [4, 4, 3]


def test_headline_and_smallest_shape(lib):
    assert [rows(lib, 5, 3, 6, v) for v in VARIANTS] == [199, 196, 194]
    assert [lib.obca_internal_full_slots(5, 3, 6, v, 64) for v in VARIANTS] == [3, 3, 3]
    assert [lib.obca_internal_full_slots(5, 2, 2, v, 64) for v in VARIANTS] == [2, 2, 2]
