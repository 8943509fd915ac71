"""CPU tier of the plan calls' shared batch (csrc/obca_plan_batch.h): the refusal table of audit::plan_batch_init, the one
validation of obca_plan_clearance, obca_plan_sweep and obca_plan_tighten, driven through the three host shims that call it
(tests/native/audit_host.cpp, plan_sweep_host.cpp, plan_tighten_host.cpp).  A refused call returns OBCA_E_INVAL and writes
nothing; the same call, unchanged, then runs.  The batch and the table are shared with tests/test_gpu_audit_edges.py."""
import ctypes

import numpy as np
import pytest

from tests import test_audit_core as core
from tests import test_plan_sweep_core as sweep_core
from tests import test_plan_tighten_core as tcore

EGO = core.EGO
SENT_F, SENT_I = -777.25, -777
N_SUB = 4
_p = core._p


def small_batch():
    """B = 5, N = 3, obstacles of 1, 4 and 2 rows; variants for the sweep and the repair, statuses for the repair"""
    x, A, b = sweep_core.translating_plans(np.random.default_rng(4242), 5, 3, (1, 4, 2))
    return dict(x=x, A=A, b=b, m=(1, 4, 2), variant=np.array([4, 6, 8, 0, 6], np.int32), status=np.array([0, 1, 0, 0, 1], np.int32))


# what plan_batch_init refuses, as replacements of the batch's arguments by name
REFUSALS = [dict(n_obs=0), dict(n_obs=9), dict(m=(1, 0, 2)), dict(m=(1, 5, 2)), dict(N=0), dict(B=0),
            dict(ego=(float("nan"), 0.75, 1.7, 0.75)), dict(ego=(1.7, 0.75, float("inf"), 0.75)),
            dict(ego=(1.7, 0.75, -1.7, 0.75)),                               # ego[0] + ego[2] = 0
            dict(ego=(-1.7, 0.75, 0.5, 0.75)),                               # ego[0] + ego[2] < 0
            dict(ego=None), dict(m=None), dict(x=None), dict(A=None), dict(b=None)]


def batch_args(c, ptr, **over):
    """the batch's arguments of a plan call in the order of the C ABI -- ego, n_obs, m, N, B, variant, x, A, b -- from the
    case c, some replaced by name; ptr turns an array (or None) into a pointer argument"""
    a = dict(ego=EGO, n_obs=len(c["m"]), m=c["m"], N=c["x"].shape[2] - 1, B=c["x"].shape[0], variant=c["variant"], x=c["x"],
             A=c["A"], b=c["b"])
    a.update(over)
    ego = None if a["ego"] is None else (ctypes.c_double * 4)(*a["ego"])
    m = None if a["m"] is None else (ctypes.c_int32 * len(a["m"]))(*a["m"])
    return [ego, a["n_obs"], m, a["N"], a["B"], ptr(a["variant"]), ptr(a["x"]), ptr(a["A"]), ptr(a["b"])]


def _host_ptr(a):
    return None if a is None else _p(a)


def _outputs(shapes):
    return {k: np.full(s, SENT_I if dt == np.int32 else SENT_F, dt) for k, (s, dt) in shapes.items()}


def _clearance(libs, c, **over):
    B, N1, n = c["x"].shape[0], c["x"].shape[2], len(c["m"])
    o = _outputs({"min_clear": (B, float), "arg_stage": (B, np.int32), "arg_obst": (B, np.int32), "stage_obst": ((B, N1, n), float)})
    h = batch_args(dict(c, variant=None), _host_ptr, **over)                  # the knot audit of the GPU test: no variant
    return libs["clearance"].audit_host_plan_clearance(*h, *[_p(v) for v in o.values()]), o


def _sweep(libs, c, **over):
    B, N = c["x"].shape[0], c["x"].shape[2] - 1
    o = _outputs({"min_clear": (B, float), "lower_bound": (B, float), "arg_interval": (B, np.int32), "arg_obst": (B, np.int32),
                  "first_collision": (B, np.int32), "interval_min": ((B, N), float), "samples": ((B, N, N_SUB + 1), float)})
    h = batch_args(c, _host_ptr, **over)
    return libs["sweep"].plan_sweep_host(*h, N_SUB, *[_p(v) for v in o.values()]), o


def _tighten(libs, c, **over):
    B, N1, n, M = c["x"].shape[0], c["x"].shape[2], len(c["m"]), sum(c["m"])
    o = _outputs({"grow": ((B, N1, n), float), "b_out": ((B, N1, M), float), "variant_out": (B, np.int32), "min_clear": (B, float),
                  "d": ((B, N1 - 1, n), float)})
    if not over:
        o["grow"][:] = 0.0                                                   # in/out: the state a first round starts from
    h = batch_args(c, _host_ptr, **over)
    rc = libs["tighten"].plan_tighten_host(*h[:6], _p(c["status"]), *h[6:], N_SUB, 0, ctypes.c_double(0.5), ctypes.c_double(1.0),
                                           ctypes.c_double(2.0), *[_p(v) for v in o.values()])
    return rc, o


@pytest.fixture(scope="module")
def libs():
    return {"clearance": core.load_host(), "sweep": sweep_core.load_host(), "tighten": tcore.load_host()}


@pytest.fixture(scope="module")
def case():
    c = small_batch()
    return dict(c, **{k: np.ascontiguousarray(c[k], float) for k in ("x", "A", "b")})


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_refused_batches_write_nothing(libs, case, bad):
    for shim in (_clearance, _sweep, _tighten):
        rc, o = shim(libs, case, **bad)
        assert rc == core.E_INVAL, shim.__name__
        for k, v in o.items():
            assert (v == (SENT_I if v.dtype == np.int32 else SENT_F)).all(), (shim.__name__, k)
        rc, o = shim(libs, case)                                             # and the same call, unchanged, runs
        assert rc == 0, shim.__name__
        for k, v in o.items():
            assert not (v == (SENT_I if v.dtype == np.int32 else SENT_F)).any(), (shim.__name__, k)

