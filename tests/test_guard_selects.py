"""The select form of the step-length guards (csrc/obca_kernel.hip: STEP_MIN, guard_selects_default) on the host.

  the neutral operands   `a = fmin(a, guard ? v : +inf)` is `if (guard) a = fmin(a, v)` only if fmin(a, +inf) is a, bit for bit,
                         over what the step lengths take: (0, 1], denormals and exact 1.0 included (they start at 1.0 and only
                         pass through fmin).  fmax(a, |0.0|) is the same statement for a non-negative running maximum that
                         starts at 0.0 -- the form tried on the complementarity guards and dropped.
  which guard binds      tests/native/step_guards_host.cpp runs the structured host core (csrc/obca_lpi_core.h) and counts, per
                         instance, the iterations in which each of the eight guards set the step length -- 0 / 1 lower / upper
                         slack, 2 / 3 p / n, 4 .. 7 their multipliers.  tests/test_gpu_guard_selects.py takes its batches from
                         here; every one of them must make all eight bind, or its word-for-word comparison proves nothing about
                         a select that is never the minimum.
  the frame table        tools/issue_census.py --frames on an assembly snippet written here: three frames that close (one with its
                         skip branch, one nested in another) and one that never does."""
import ctypes
import functools
import os
import sys

import numpy as np

from oracle import c_oracle
from tests import native_build

sys.path.insert(0, os.path.join(native_build.ROOT, "tools"))
import issue_census  # noqa: E402

SRC = os.path.join(native_build.HERE, "native", "step_guards_host.cpp")
GUARDS = ("lower slack", "upper slack", "p", "n", "zL", "zU", "zp", "zn")


@functools.lru_cache(maxsize=None)
def host():
    lib = native_build.build_shim("step_guards_host", [SRC], openmp=True)
    lib.step_guards_solve_batch.restype = ctypes.c_int
    return lib


def step_guards(b, N, v, **prm):
    """(outputs of the host core, bound [B, 8]: iterations of instance i in which guard k set the step length)"""
    B, m, P = len(v), b["m"], native_build._ptr
    out = dict(xopt=np.zeros((B, 3, N + 1)), uopt=np.zeros((B, 2, N)), ts_opt=np.zeros(B), status=np.zeros(B, np.int32),
               iters=np.zeros(B, np.int32), info=np.zeros((B, 4)))
    bound = np.zeros((B, 8), np.int32)
    arrs = [np.ascontiguousarray(b[k], float) for k in ("x0", "u0", "xref", "A", "b")]
    arrs.append(np.ascontiguousarray(np.broadcast_to(np.asarray(b["Ts"], float), (B,))))
    arrs.append(np.ascontiguousarray(b["term"], float))
    marr = (ctypes.c_int * len(m))(*[int(x) for x in m])
    rc = host().step_guards_solve_batch(N, len(m), marr, P(np.ascontiguousarray(v, np.int32)), B, *[P(a) for a in arrs],
                                        ctypes.byref(c_oracle.default_params(**prm)), *[P(out[k]) for k in ("xopt", "uopt", "ts_opt", "status", "iters", "info")],
                                        P(bound))
    assert rc == 0
    return out, bound


def terminal_set(b):
    """tests/test_gpu_row_kinds.py: _terminal_set (that module needs a GPU to import)"""
    n = len(b["variant"])
    return dict(b, term=np.stack([b["x0"][:, 0] - 1.0, np.full(n, 1.0), np.full(n, 9.0)], axis=1))


def headline_batch(B=64):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import scenarios as sc
    return terminal_set(sc.make_batch(B, 5))


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _sweep():
    tiny = np.finfo(np.float64).tiny
    return np.concatenate([[5e-324, 1e-320, tiny / 2, tiny, np.nextafter(tiny, 1.0)], np.logspace(-300, 0, 601),
                           [np.nextafter(1.0, 0.0), 1.0], np.linspace(0.0, 1.0, 257)[1:]])


def test_fmin_with_infinity_keeps_every_step_length():
    a = _sweep()
    assert a.min() > 0.0 and a.max() == 1.0 and (a == 1.0).any() and (a < np.finfo(np.float64).tiny).any()
    assert np.array_equal(_bits(np.fmin(a, np.inf)), _bits(a))
    v = a[::-1].copy()                                   # and where the guard holds the operand is the guarded expression itself
    for guard in (a > 0.3, a < 0.3):
        sel = np.fmin(a, np.where(guard, v, np.inf))
        old = a.copy()
        old[guard] = np.fmin(a[guard], v[guard])
        assert np.array_equal(_bits(sel), _bits(old))
    assert np.array_equal(_bits(np.fmin(a, np.where(a > 2.0, np.nan, np.inf))), _bits(a))     # a NaN in an unselected lane never arrives


def test_fmax_with_zero_keeps_every_running_maximum():
    a = np.concatenate([[0.0], _sweep(), np.logspace(0, 300, 301), [np.finfo(np.float64).max, np.inf]])
    assert not np.signbit(a).any()
    assert np.array_equal(_bits(np.fmax(a, np.fabs(0.0))), _bits(a))
    assert np.array_equal(_bits(np.fmax(a, np.fabs(-0.0))), _bits(a))


def test_every_guard_binds_on_the_headline_batch():
    b = headline_batch()
    for variant in (4, 6, 8):
        out, bound = step_guards(b, 5, np.full(64, variant, np.int32))
        assert np.isin(out["status"], (0, 1)).all()
        assert (bound.sum(axis=0) > 0).all(), dict(zip(GUARDS, bound.sum(axis=0)))


SNIPPET = """
	.loc	1 10 0
	v_cmp_gt_f64_e32 vcc, 0, v[2:3]
	s_and_saveexec_b64 s[4:5], vcc
	s_cbranch_execz .LBB0_2
; %bb.1:
	v_mul_f64 v[4:5], v[2:3], v[6:7]
	v_min_f64 v[0:1], v[0:1], v[4:5]
.LBB0_2:
	s_or_b64 exec, exec, s[4:5]
	.loc	1 20 0
	s_and_saveexec_b64 s[6:7], vcc
	ds_read_b64 v[8:9], v10
	s_waitcnt lgkmcnt(0)
	.loc	1 21 0
	s_andn2_saveexec_b64 s[8:9], s[10:11]
	v_add_f64 v[8:9], v[8:9], v[0:1]
	s_mov_b32 s12, 0
	s_or_b64 exec, exec, s[8:9]
	v_mov_b32_e32 v11, 0
	v_accvgpr_write_b32 a0, v11
	s_or_b64 exec, exec, s[6:7]
	.loc	1 30 0
	s_and_saveexec_b64 s[14:15], vcc
	global_store_dwordx2 v[12:13], v[0:1], off
	s_endpgm
"""


def test_frame_table_on_a_three_frame_snippet():
    fr = issue_census.frames(SNIPPET.split("\n"))
    assert len(fr) == 4
    short, outer, inner, open_ = fr
    assert (short["line"], short["op"], short["branch"], short["closed"]) == (10, "s_and_saveexec_b64", "s_cbranch_execz", True)
    assert [short[c] for c in issue_census.FRAME_COLS] == [2, 0, 0, 0, 0]          # its own skip branch is not its body
    assert (outer["line"], outer["branch"], outer["closed"]) == (20, None, True)
    assert [outer[c] for c in issue_census.FRAME_COLS] == [2, 1, 1, 3, 0]          # the nested frame's save and restore are scalar work of the outer
    assert (inner["line"], inner["op"], inner["branch"], inner["closed"]) == (21, "s_andn2_saveexec_b64", None, True)
    assert [inner[c] for c in issue_census.FRAME_COLS] == [1, 0, 0, 1, 0]
    assert not open_["closed"] and open_["other"] == 1 and open_["scalar"] == 1
    assert all(f["region"] is None for f in fr)
    regions = [(1, "first"), (15, "second")]
    assert [f["region"] for f in issue_census.frames(SNIPPET.split("\n"), regions=regions)] == ["first", "second", "second", "second"]
